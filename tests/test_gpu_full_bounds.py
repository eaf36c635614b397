"""GPU: every circuit kernel on operands that FILL their static bounds (tests/synth.py), bit-exact
against the model circuits that test_synth_reference.py pins to the C oracle on the CPU.

The other parity tests feed the engine genuine fresh encryptions, whose bits have degree at most
d + d' whatever bound their batch was allocated with; here the polynomials are synthetic (uploaded
with Ciphered.from_host) and as long as their bounds allow, so the LDS slices, workspace slots,
tile widths, chunk counts and plan limits the host derives from the bounds are met by data that
reaches them.  Every case compares limbs and degree words, checks out.bound against the Python
restatement of the bound rules and ends on a clean ctx.synchronize().  There is no tolerance.

Each case is named for a path; the path assertion itself is evaluated on the CPU from the model's
integers (synth.check_*_path, run by test_synth_reference.py) and quoted in the test's docstring
with the expression of capi.cpp or of the kernel it comes from.
"""
import numpy as np
import pytest

import borrow_model as bm
import synth
from helpers import as_bytes, assert_batches_equal, bit_ints, keys, masks, plain

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import homomorph
    homomorph.lib()  # loud failure if the engine is not built
    return homomorph


@pytest.fixture(scope="module")
def world(H):
    """One seeded context per parameter set (the keys only matter for validation and decryption)."""
    cache = {}

    def get(params=synth.PARAMS):
        if params not in cache:
            ctx = H.Context(H.Parameters(*params))
            ctx.seed_rng(synth.SEED)
            ctx.generate_secret_key()
            ctx.generate_public_key()
            cache[params] = ctx
        return cache[params]
    return get


def upload(H, ctx, family, name):
    c = synth.inputs(family, name)
    la, da, lb, db = synth.packed(family, name)
    a = H.Ciphered.from_host(la, da, c["ba"], c["n"], ctx.device, None)
    b = H.Ciphered.from_host(lb, db, c["bb"], c["n"], ctx.device, None)
    return c, a, b


def same(out, ob, rl, rd, n, what):
    assert np.array_equal(out.bound, ob), what
    gl, gd = out.to_host()
    assert_batches_equal(gl, gd, rl, rd, ob, n, what)


def unsupported(H, fn):
    from homomorph import _lib
    with pytest.raises(H.EngineError) as ei:
        fn()
    assert ei.value.status == _lib.ERR_UNSUPPORTED


# ------------------------------------------------------------------ gates
@pytest.mark.parametrize("op", synth.GATE_OPS)
@pytest.mark.parametrize("name", list(synth.GATE_CASES))
def test_gates(H, world, name, op):
    """gate_kernel (kernels.hip): AND / OR run wave_mul<kQSmall = 10, 8>(a_i, na, b_i, nb, ...)
    with nout = na + nb words, a tile width W = ceil(nout / 64) up to 8 and MULTI tiles past 512
    words; OR keeps x_i in T's tail at Xs = T + na + nb + 2.  u8, 8 scheduled values + 2 FULL /
    bound - 1 pairs.  Paths (synth.check_gate_path, words of a_i + b_i):
      chunks            700 / 700    22 + 22   nu = 22: ceil(22 / kQSmall) = 3 uniform chunks
      w1_edge           1023 / 1023  32 + 32   nout = 64, the last W = 1 product
      w2_edge           1023 / 1055  32 + 33   nout = 65, the first W = 2 product
      one_tile          8191 / 8191  256 + 256 nout = 512 = 64 * 8: exactly one W = 8 tile
      multi_tile        8191 / 8223  256 + 257 nout = 513: a second, MULTI tile of one word
      lopsided          40 / 9000    2 + 282   nu = 2 against nv = 282 (and swapped: nu = 282)
      per_bit           a: 64 i + 63, b: 1000 - 97 i: capacities distinct within each operand,
                        no offset shared, every slot filled
    XOR and NOT run wave_xor over the same slices (G.oA, G.oB, G.oT of hm_gate_batch)."""
    ctx = world()
    c, a, b = upload(H, ctx, "gate", name)
    ob, _, rl, rd = synth.gate_reference(name, op)
    opcls = {"and": H.HomomorphicAndGate, "or": H.HomomorphicOrGate,
             "xor": H.HomomorphicXorGate, "not": H.HomomorphicNotGate}[op]
    out = ctx.apply1(opcls, a) if op == "not" else ctx.apply2(opcls, a, b)
    ctx.synchronize()
    same(out, ob, rl, rd, c["n"], f"{name} {op}")


# ------------------------------------------------------------------ subtraction, comparisons
def _cmp(H, op):
    return {"eq": H.HomomorphicEqual, "ne": H.HomomorphicNotEqual, "lt": H.HomomorphicLessThan,
            "le": H.HomomorphicLessEqual, "gt": H.HomomorphicGreaterThan,
            "ge": H.HomomorphicGreaterEqual}[op]


@pytest.mark.parametrize("what", ["sub", "unsigned", "signed"])
@pytest.mark.parametrize("name", list(synth.BORROW_CASES))
def test_sub_and_comparisons(H, world, name, what):
    """borrow_kernel (kernels.hip) in plan_borrow's LDS layout (circuit_host.h: SA, SB, SX = 2 cap
    words, two borrow buffers of cw = SX + chain / 32 + 3): the generate product wave_mul<kQSmall, 8>(a_i,
    na, b_i, nb, ...) and the propagate product wave_mul<kQSmall, 8>(p_i, np, w_i, nw, ...).
    Paths (synth.check_borrow_path):
      u8_b700       uniform 700: na = 22 (3 kQSmall chunks), p_i of 22 words = its slot SX, and
                    the last product p_7 w_7 of 198 words, as long as the bounds allow
      u16_per_bit   bounds 63 .. 1100, on every bit one operand near 1100 and the other on a
                    ladder from 63 (a uniform spread cannot pass 512 words: synth.
                    _u16_borrow_bounds): every slot filled, and p_15 w_15 spans more than 512
                    words, a MULTI tile
      u8_pair_b255  FULL / bound - 1 at 255: every degree on its limb's last bit, na = np = 8 =
                    the slot
    Subtraction, then the six comparisons unsigned and signed, against borrow_model."""
    ctx = world()
    c, a, b = upload(H, ctx, "borrow", name)
    if what == "sub":
        ob, _, rl, rd = synth.borrow_reference(name, "sub")
        out = ctx.apply2(H.HomomorphicSubtraction, a, b)
        ctx.synchronize()
        same(out, ob, rl, rd, c["n"], f"{name} sub")
        return
    signed = what == "signed"
    for op in bm.COMPARISONS:
        ob, _, rl, rd = synth.borrow_reference(name, op, signed)
        out = ctx.apply2(_cmp(H, op), a, b, signed=signed)
        assert out.nbits == 8 and out.n == c["n"]
        same(out, ob, rl, rd, c["n"], f"{name} {op} signed={signed}")
    ctx.synchronize()


def test_chained_gates_then_borrow(H, world, oracle):
    """Genuine ciphertexts through a chain: sub(and(a, b), or(a, b)) and lt of the same pair.
    Every intermediate bound comes from the previous out.bound (fresh 128 -> 256 for both gates,
    the borrow over 256 / 256), the intermediates are products as long as those bounds, and every
    stage is bit-exact against the model; the decryptions equal the oracle's of the model's
    output."""
    ctx = world()
    sk, pk, _ = keys(*synth.PARAMS, synth.SEED)
    n = 8
    av, bv = plain(n, np.uint8, 1), plain(n, np.uint8, 2)
    ma, mb = masks(n, 8, 64, 3), masks(n, 8, 64, 4)
    fresh = synth.uniform(8, 128)
    a, b = ctx.encrypt(av, masks=ma, bound=fresh), ctx.encrypt(bv, masks=mb, bound=fresh)
    la, da = oracle.encrypt_batch(pk, as_bytes(av), ma, fresh)
    lb, db = oracle.encrypt_batch(pk, as_bytes(bv), mb, fresh)
    A = [bit_ints(la, da, fresh, e) for e in range(n)]
    B = [bit_ints(lb, db, fresh, e) for e in range(n)]
    x = ctx.apply2(H.HomomorphicAndGate, a, b)
    y = ctx.apply2(H.HomomorphicOrGate, a, b)
    X = [synth.gate_circuit("and", p, q) for p, q in zip(A, B)]
    Y = [synth.gate_circuit("or", p, q) for p, q in zip(A, B)]
    for out, vals, op in ((x, X, "and"), (y, Y, "or")):
        ob = synth.gate_bounds(op, fresh, fresh)
        same(out, ob, *bm.pack(vals, ob), n, f"chain {op}")
    s = ctx.apply2(H.HomomorphicSubtraction, x, y)
    r = ctx.apply2(H.HomomorphicLessThan, x, y, signed=False)
    sb = bm.sub_bounds(x.bound, y.bound)
    rb = bm.compare_bounds("lt", x.bound, y.bound)
    sl, sd = bm.pack([bm.sub_circuit(p, q) for p, q in zip(X, Y)], sb)
    rl, rd = bm.pack([bm.bool_value(bm.compare_circuit("lt", p, q)) for p, q in zip(X, Y)], rb)
    same(s, sb, sl, sd, n, "chain sub")
    same(r, rb, rl, rd, n, "chain lt")
    ds = ctx.decrypt_bytes(s).cpu().numpy()
    dr = ctx.decrypt_bytes(r).cpu().numpy()
    ctx.synchronize()
    assert np.array_equal(ds, oracle.decrypt_batch(sk, sl, sd, sb, 8, n))
    assert np.array_equal(dr, oracle.decrypt_batch(sk, rl, rd, rb, 8, n))


# ------------------------------------------------------------------ addition
def _add(H, world, name, chain, refused=False):
    ctx = world()
    c, a, b = upload(H, ctx, "add", name)
    ctx.set_add_options(chain)
    try:
        if refused:
            unsupported(H, lambda: ctx.apply2(H.HomomorphicAddition, a, b))
            ctx.synchronize()
            return
        out = ctx.apply2(H.HomomorphicAddition, a, b)
        ctx.synchronize()
    finally:
        ctx.set_add_options("auto")
    ob, _, rl, rd = synth.add_reference(name)
    same(out, ob, rl, rd, c["n"], f"{name}/{chain}")


@pytest.mark.parametrize("chain", ["valu", "auto", "mfma"])
@pytest.mark.parametrize("B", synth.ADD_UNIFORM)
def test_add_plan_limits(H, world, B, chain):
    """hm_add_batch's plan limits (capi.cpp), at them and one past them: uniform bound B, u8, 8
    scheduled values + 4 FULL / bound - 1 pairs whose P_i = x_i (1 + a_i b_i) has degree 3 B - 1.
    The widest P_i over the batch (synth.check_add_path; maxPw = words_of_bound(3 B)):
      B     P_i words   plan
      138   13          maxPw <= 2 * 7 - 1: the 7-chunk MFMA chain's last bound
      139   14          the 13-chunk chain
      266   25          maxPw <= 2 * 13 - 1, and PAD's maxPw <= 25 (kQBig): both limits
      267   26          the 25-chunk chain; the VALU chain leaves PAD / staged
      522   49          maxPw <= 2 * 25 - 1: the last bound any MFMA chain takes
      523   50          no MFMA plan: "mfma" is HM_ERR_UNSUPPORTED, "auto" runs the VALU chain
    "valu" and "auto" are bit-exact at all six."""
    _add(H, world, f"u8_b{B}", chain, refused=(chain == "mfma" and B == 523))


@pytest.mark.parametrize("chain", ["valu", "auto", "mfma"])
@pytest.mark.parametrize("name", ["u16_b266", "u32_b266"])
def test_add_wmax_classes(H, world, name, chain):
    """B = 266 at three widths: the PAD chain's tile width wmax steps with SC (capi.cpp: SC = the
    widest words(P_i) + words(carry bound) + 2, need_w = ceil(SC / 64), wmax the next of 4, 8,
    12, 16, 24).  u8 (test_add_plan_limits): SC = 169, need_w = 3, wmax = 4;  u16: SC = 368,
    need_w = 6, wmax = 8;  u32 (n = 4): SC = 767, need_w = 12, wmax = 12.  The widest product of
    the data is within a word of SC - 2 (synth.check_add_path)."""
    _add(H, world, name, chain)


@pytest.mark.parametrize("chain", ["valu", "auto", "mfma"])
@pytest.mark.parametrize("top", [1023, 1024])
def test_add_last_bit_wide(H, world, top, chain):
    """The MFMA plan's x-width rule cntX <= 32 (capi.cpp; the chain XORs x into sum words 0 .. 31
    only), accept side and one past it: all bounds 128 except ba[7] = top, a_7 of degree exactly
    top in the pairs.  1023: x_7 has 32 live words, the forced MFMA chain runs and every one of
    them is in the sum.  1024: 33 words, "mfma" is refused and "auto" / "valu" equal the model."""
    _add(H, world, f"last_{top}", chain, refused=(chain == "mfma" and top == 1024))


@pytest.mark.parametrize("chain", ["valu", "auto", "mfma"])
def test_add_per_bit_bounds_filled(H, world, chain):
    """Per-bit bounds drawn in [64, 266], different per operand (the "random" skew of
    test_add_skewed_bounds) with data that fills every slot: cntX, cntP, cntAB and the per-bit
    offsets of the prep workspace are all met at their bounds."""
    _add(H, world, "per_bit", chain)


# ------------------------------------------------------------------ multiplication
@pytest.mark.parametrize("products", ["mfma", "valu"])
@pytest.mark.parametrize("name", list(synth.MUL_CASES))
def test_mul(H, world, name, products):
    """The carry-save multiplier (mul_columns, mul_host.cpp) on non-fresh operands: the scheduled
    kinds put a NULL and a UNIT partial product and an all-ones operand in every column
    (synth.check_mul_path), per-bit bounds in [64, 200] make the plan's slots and offsets
    non-uniform, and mul_low(k = 4) reads the low 4 bits of u16 operands in place from such a
    layout (reference: the 4-bit circuit on helpers.low_bits)."""
    ctx = world()
    c, a, b = upload(H, ctx, "mul", name)
    _, _, signed, k, _, _ = synth.MUL_CASES[name]
    ctx.set_mul_products(products)
    try:
        if k:
            out = ctx.mul_low(a, b, k)
        else:
            out = ctx.apply2(H.HomomorphicMultiplication, a, b, signed=signed)
        ctx.synchronize()
    finally:
        ctx.set_mul_products("auto")
    ob, _, rl, rd = synth.mul_reference(name)
    same(out, ob, rl, rd, c["n"], f"{name}/{products}")


@pytest.mark.parametrize("products", ["mfma", "valu"])
@pytest.mark.parametrize("name", list(synth.MUL_CLASS_CASES))
def test_mul_classes(H, world, name, products):
    """Every product class of the multiplier at its size edges, and the degree ladders that walk
    the kernels' inner paths.  build_plan (mul_host.cpp) picks the launches from the static
    bounds; the kernels pick their path from each operand's word count nu (from its degree).
    u8 operands, uniform bounds a / b unless noted, mul_low(4) unless noted; paths from the
    planner's own census (synth.check_mul_class_path, test_synth_reference.py):
      ppv_12w        383          `P.ppv = max(ppg_umax, ppg_vmax) <= kPPVWords`: 12 words, the last
      ppg_tiny_13w   384          grouped launch; launch_mul_ppg `a.umax <= kMfTinyWords`:
      ppg_tiny_20w   639          mul_ppg_kernel<11> at its first and last size
      ppg_gen_21w    640          mul_ppg_kernel<kMfG + 1>, first size; narrow carries U = 44
      ppg_gen_33w    1055         33 words = 17 chunks, the last `max(wa, wb) <= kMfPPGWords`
      w34_1056, w34_1087          34 words = 18 chunks, one more than mul_ppg_kernel's `switch
                                  (nu / 2 + 1)` has: per-column launches (ppm, umax 36) since
                                  kMfPPGWords = 33; carries narrow at U = 68
      ppm_35w        1088         ppm umax 36 on the narrow instance; carries narrow at U = 72 =
                                  kMfNarrowWords, the class's last size
      wide_76        1152         `uw <= kMfNarrowWords ? 1 : 2`: carries wide (windowed,
                                  mul_mfma_kernel<false, true, true>) at U = 76, its first size
      ppm_wide       2304, k = 3  ppm umax 76: launch_mul_mfma's last branch, mul_mfma_kernel<false>
      ppm_narrow_2303  2303, k = 3  ... and umax 72 beside it, narrow
      rows_v36       287          rows_ok `uw <= kRowsU && vw <= kRowsV`: column 2 has 3 row
                                  products, rows_uw 20, rows_vw 36, rows_qw 18
      tiny_v40       288, 319     column 2's third product has V = 40 > kRowsV: one span on the tiny
                                  MFMA instance (U = 20), rows_qw 19 and 20 beside it
      narrow_24      320          U = 24 > kRowsU: no rows, narrow
      ppg_lopsided   127 / 1055   ppg_umax 4 against ppg_vmax 33 on mul_ppg_kernel<11>, and swapped
                                  (33 against 4, mul_ppg_kernel<17>)
      tiny_under_wide_prefix  a = [1200, 100, ..], b = 100: ppm umax 4 / vmax 40 on the tiny
                                  instance, tiny carries U = 8, V = 44
      u8_b640_full, i8_b640_full  640, the full circuit: general ppg, narrow + wide launches in
                                  columns 3..6, four Karatsuba programs on both lanes in column 6
                                  (leaves 192 and 256, mul_mfma_kernel<true>); signed: the two
                                  flipped VALU partial products of column 7 beside the ppg launch
      u8_b703_ka224  703, full, set_mul_options(224, 224): 224-word leaves on both lanes on the
                                  lean leaf instance (run_ka: `a.umax <= kMfLeanLeafWords &&
                                  a.umax >= kMfLeanLeafMin`, mul_mfma_kernel<true, true>)
    Ladders (synth.ladder: value e's a_i has e + 1 words, b FULL, mul_low(3), one carry product
    U = a_0 b_1 in column 1):
      ladder_ppv 383 x 12      nu = 1..12 in mul_ppv_kernel's rows
      ladder_ppg_tiny 639 x 20 `switch (nu / 2 + 1)`: 1..11
      ladder_ppg_gen 1055 x 33 ... 1..17; the narrow carry's U at 34..66 words
      ladder_w34 1087 x 34, ladder_ppm 1088 x 35   mf_item's groups through ppm: 1..18 chunks (every
                               tail 1..17, then 16 + 2); the narrow carry's U at 35..68 words: 18..35
                               chunks, every tail after one full group and after two
      ladder_rows 287 x 9      mul_rows_kernel's U at 10..18 words against rows_qw = 18
    "valu" runs the same cases with every product off the matrix cores.  Bit-exact against
    gf2_model.mul_circuit (limbs, degree words, out.bound)."""
    ctx = world()
    c, a, b = upload(H, ctx, "mulc", name)
    spec = synth.MUL_CLASS_CASES[name]
    ctx.set_mul_products(products)
    if spec["ka"]:
        ctx.set_mul_options(*spec["ka"])
    try:
        if spec["k"]:
            out = ctx.mul_low(a, b, spec["k"])
        else:
            out = ctx.apply2(H.HomomorphicMultiplication, a, b, signed=spec["signed"])
        ctx.synchronize()
    finally:
        ctx.set_mul_products("auto")
        ctx.set_mul_options()
    ob, _, rl, rd = synth.mul_class_reference(name)
    same(out, ob, rl, rd, c["n"], f"{name}/{products}")


# ------------------------------------------------------------------ decryption
@pytest.mark.parametrize("name", list(synth.DEC_CASES))
def test_decrypt(H, world, oracle, name):
    """hm_decrypt_batch (capi.cpp): D.ucap = the common capacity when every bit's is equal and at
    most 8 limbs, else 0 (the general path).  u8, n = 64, scheduled kinds then random ones, the
    secret key of (128, 128, 1, 128).  Paths (synth.check_dec_path):
      b511_ucap  uniform 511: capacity 8, the last bound on the ucap path
      b512       uniform 512: capacity 9, the first off it
      per_bit    63 .. 3000: capacities 1 .. 47, all distinct, every one reached by a polynomial
                 (maxcap > 32: launch_decrypt's one-wave-per-value decrypt_kernel)
      per_bit_cap32  63 .. 2047: the same with maxcap = 32, the last on decrypt_bits_kernel
    Against oracle.decrypt_batch and the model's decipher_bit."""
    ctx = world(synth.DEC_PARAMS)
    c, a, _ = upload(H, ctx, "dec", name)
    got = ctx.decrypt(a, np.uint8)
    ctx.synchronize()
    sk, _, _ = keys(*synth.DEC_PARAMS, synth.SEED)
    la, da, _, _ = synth.packed("dec", name)
    assert np.array_equal(got, oracle.decrypt_batch(sk, la, da, c["ba"], 8, c["n"]).reshape(-1))
    assert np.array_equal(got, synth.dec_reference(name).reshape(-1))
