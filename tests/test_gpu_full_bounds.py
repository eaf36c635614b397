"""GPU: every circuit kernel on operands that FILL their static bounds (tests/synth.py), bit-exact
against the model circuits that test_synth_reference.py pins on the CPU (to the C oracle, or for
select, min / max, lookup, shift, the bit counts and the array circuits to a second evaluation).

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
    the kernels' inner paths.  build_plan (mul_plan.h) picks the launches from the static
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


# ------------------------------------------------------------------ select, min / max
def _from_host(H, ctx, limbs, deg, bound, n):
    return H.Ciphered.from_host(limbs, deg, bound, n, ctx.device, None)


@pytest.mark.parametrize("name", list(synth.SELECT_CASES))
def test_select(H, world, name):
    """select_kernel (kernels.hip): wave_mul<kQSmall = 10, 8>(X, nx, C, nc, Bb, nb, T) per bit, x_i
    = a_i + b_i the uniform operand, the condition c the per-lane one, b_i added: nout = max(nx +
    nc, nb) words, W = ceil(nout / 64) up to 8, MULTI tiles past 512, x_i read in chunks of 10
    words.  u8; 8 scheduled values whose condition cycles through the kinds (NULL: a null product,
    an exact copy of b_i; UNIT: nc = 1), then a FULL against b one below its bound and the other
    way round under a FULL condition.  Paths (synth.check_select_path; condition / a, b bounds):
      w1_edge        1023 / 1023   nx + nc = 32 + 32 = 64, the last W = 1 product
      w2_edge        1023 / 1055   33 + 32 = 65, the first W = 2
      one_tile       8191 / 8191   256 + 256 = 512: exactly one W = 8 tile
      multi_tile     8191 / 8223   257 + 256 = 513: a MULTI tile of one word
      chunks_10_11   500 / 319, 320   nx = 10 and 11: one and two uniform chunks
      chunks_20_21   500 / 639, 640   nx = 20 and 21: two and three
      lopsided       9000 / 40     nx = 2 against nc = 282; swapped (40 / 9000): nx = 282, 29
                                   chunks, against nc = 2
      per_bit        500 / a: 64 i + 63, b: 1000 - 97 i   capacities distinct within each operand,
                     every slot filled; two more values with x_i of one word under a one-word
                     condition: nb > nx + nc, nout = nb, at every bit but bit 0
    Every slot of plan_select (SC, SA, SB, SX and T = SC + SX + 2) is filled to the last word its
    bound allows and every output bit reaches hm_select_out_bounds."""
    ctx = world()
    c = synth.inputs("select", name)
    la, da, lb, db, lc, dc = synth.packed("select", name)
    a = _from_host(H, ctx, la, da, c["ba"], c["n"])
    b = _from_host(H, ctx, lb, db, c["bb"], c["n"])
    cond = _from_host(H, ctx, lc, dc, c["bc"], c["n"])
    out = ctx.select(cond, a, b)
    ctx.synchronize()
    ob, _, rl, rd = synth.select_reference(name)
    same(out, ob, rl, rd, c["n"], f"select {name}")


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("name", list(synth.MINMAX_CASES))
def test_min_max(H, world, name, signed):
    """minmax_kernel (kernels.hip): phase 1 is borrow_step through the top bit (the paths of
    test_sub_and_comparisons, on the operands of every synth.BORROW_CASES entry); phase 2 is
    wave_mul<kQSmall, 8>(X, nx, W, nw, is_max ? Ab : Bb, ..., Wn) with W = w_n kept in a borrow
    buffer of cw = SX + chain / 32 + 3 words (plan_borrow with chain = wb_L).  Paths
    (synth.check_minmax_path):
      u8_b700, u16_per_bit, u8_pair_b255   the borrow cases' operands (u16_per_bit with one all-FULL
                     value more: x_15 w_16 spans more than 512 words, a MULTI tile)
      p2_one_tile    uniform 1632: nw = 460, nx = 52, nx + nw = 512 = one W = 8 tile
      p2_multi_tile  uniform 1636: nw = 461, nx + nw = 513
      null_borrow    uniform 255: a = b bit for bit over {0, 1} and b null under a of every kind
                     leave w_n null: phase 2's product is null over nout = max(nx, nadd) words and
                     the operand is copied through Add (min: b, max: a)
    The borrow buffer is filled to the last word the bounds allow; every output bit reaches
    hm_minmax_out_bounds (bit 0 under ba_0 = bb_0: one below, the most any data can).  Min and
    max, unsigned and signed, against select_model."""
    ctx = world()
    c, a, b = upload(H, ctx, "minmax", name)
    for op, cls in (("min", H.HomomorphicMin), ("max", H.HomomorphicMax)):
        out = ctx.apply2(cls, a, b, signed=signed)
        ob, _, rl, rd = synth.minmax_reference(name, op, signed)
        same(out, ob, rl, rd, c["n"], f"{op} {name} signed={signed}")
    ctx.synchronize()


# ------------------------------------------------------------------ lookup
@pytest.mark.parametrize("which", synth.LOOKUP_TABLES)
@pytest.mark.parametrize("name", list(synth.LOOKUP_CASES))
def test_lookup(H, world, name, which):
    """lookup_kernel (kernels.hip) in plan_lookup's layout (lookup_host.h: one slot per monomial at
    off[], the inner sum I of cI words, two accumulators of cP = even(cI + cH) + 2): the monomials
    by doubling, wave_mul<kQSmall, 8>(a_i, nb, M[s], ..) with a_i uniform, then per output bit
    lookup_inner_sum's cI loop and the accumulate wave_mul(MH[t], nh, I, ni, P, np, Pn).  Tables:
    all = t[0] = 1 (every ANF coefficient set), top = t[2^k - 1] = 1 (the top monomial alone),
    random = seeded.  8 scheduled values (a NULL index bit nulls every monomial above it: `if
    (!nh) continue` and the N[id] = 0 flows; a UNIT bit makes the product a copy) + 2 all-FULL.
    Paths (synth.check_lookup_path; k, index bounds):
      w1_edge        2; 1023, 1023   accumulate nh + ni = 32 + 32 = 64
      w2_edge        2; 1023, 1055   33 + 32 = 65
      one_tile       8; 2040 x 8     256 + 256 = 512: one W = 8 tile; every doubling slot, cI, cH
                                     and cP filled (5416 of 10 240 LDS words)
      multi_tile     8; a_7 = 2072   257 + 256 = 513: a MULTI tile
      chunks_319 .. chunks_640   4; uniform   the doubling's uniform a_i at 10, 11, 20, 21 words
      odd_split_per_bit  5 (kl = 3, kh = 2); 63 + 97 i, the low 5 bits of a u16 batch: distinct
                     slot sizes per monomial; the `need` mask under the random table
      wide_out       3; 700; a u32 table   32 output bits, P / Pn exchanged in every one (all and
                     top set all 32 bits of their one entry)
    Bit-exact against lookup_model."""
    ctx = world()
    c, a, _ = upload(H, ctx, "lookup", name)
    out = ctx.lookup(a, synth.lookup_table(name, which), in_bits=c["k"])
    ctx.synchronize()
    ob, _, rl, rd = synth.lookup_reference(name, which)
    same(out, ob, rl, rd, c["n"], f"lookup {name} {which}")


# ------------------------------------------------------------------ shift
@pytest.mark.parametrize("mode", synth.shm.MODES, ids=lambda m: m[0] + ("_signed" if m[1] else ""))
@pytest.mark.parametrize("name", list(synth.SHIFT_CASES))
def test_shift(H, world, name, mode):
    """shift_kernel (kernels.hip) in plan_shift's layout (shift_host.h: in-place slots off[i] of
    even(need[i] / 32 + 2) words, the X / T buffers at the widest slot, the rotates' save area
    sv[t] at "amount bounds above t + widest a"): stages from t = L - 1 down to `last`, per product
    wave_mul<kQSmall, 8>(S, ns, V, nv, xi, ni, T) with s_t uniform and V = x_i + x_src; the last
    stage stores from T.  The amount's bits cycle through the kinds (a NULL s_t is a skipped stage).
    Paths (synth.check_shift_path; amount bounds / value bounds; all five modes):
      w1_edge        255 x 3 / 1279   final product ns + nv = 8 + 56 = 64
      w2_edge        255 x 3 / 1311   8 + 57 = 65
      one_tile       255 x 3 / 15615  8 + 504 = 512; the rotates' sv[2] area (4 x 490) filled;
                                      7144 of 10 240 LDS words
      multi_tile     255 x 3 / 15647  8 + 505 = 513
      chunks         319, 320, 639 / 200 + 7 i   s_t at 10, 11 and 20 words in the three stages
      per_bit        63, 700, 320 / 63 .. 511 .. 127   per-bit need[i] slots (prefix maxima for
                     SHL, suffix maxima for SHR), each filled as far as the stages above the last
                     can fill it
      stage_subsets  255 x 3 / 300 + 5 i   value e has s_t NULL iff bit t of e is clear: last = -1
                     (the copy-out), 0, 1, 2 and a skipped middle stage, FULL values
      u32_headline_shape  256 x 5 / 256 x 32, parameters (128, 128, 1, 128): five stages, 32 slots
                     at 1536
    Uniform value bounds end on values with one FULL bit and the others one below (equal tops
    cancel by parity).  Bit-exact against shift_model."""
    op, signed = mode
    c = synth.inputs("shift", name)
    ctx = world(c["params"])
    _, a, s = upload(H, ctx, "shift", name)
    cls = {"shl": H.HomomorphicShiftLeft, "shr": H.HomomorphicShiftRight,
           "rotl": H.HomomorphicRotateLeft, "rotr": H.HomomorphicRotateRight}[op]
    out = ctx.shift(cls, a, s, signed=signed)
    ctx.synchronize()
    ob, _, rl, rd = synth.shift_reference(name, op, signed)
    same(out, ob, rl, rd, c["n"], f"{op} {name} signed={signed}")


# ------------------------------------------------------------------ counts, runs, array
@pytest.mark.parametrize("name", list(synth.COUNT_CASES))
def test_bit_counts(H, world, name):
    """bitcount_kernel and bitrun_kernel (kernels.hip) in plan_bitcount's layout (bitcount_host.h:
    the slots E_1 .. E_J or the runs' accumulators at off[], T, the running product's D / Dn of cD
    words; a wave's slice within 2560 words): every product wave_mul<kQSmall, 8>(U, nu, P, np, ..)
    with the literal uniform.  u8, 8 scheduled values, then all FULL and seven FULL with bit 3 one
    below (equal tops cancel by parity in a symmetric sum).  Paths (synth.check_count_path), all six
    ops unless noted:
      w1_edge        255 x 8       the last running product u_8 (u_1 .. u_7): 8 + 56 = 64 words
      w2_edge_top    bit 7 at 287  9 + 56 = 65 for the counts and the trailing runs (8 + 57 for the
                                   leading runs, whose last literal is bit 0)
      w2_edge_low    bit 0 at 287  9 + 56 = 65 for the leading runs (8 + 57 for the others)
      chunks_319, chunks_320       the literal at 10 and 11 words: one and two uniform chunks
      one_tile       2047 x 8      counts only (the planner refuses the runs there): 64 + 448 = 512
                                   = one W = 8 tile; 2006 of 2560 LDS words
      multi_tile     bit 7 at 2079 counts only: 65 + 448 = 513, a MULTI tile
    Every output's slot or accumulator and D / Dn are filled to the last word their bounds allow.
    Bit-exact against bitcount_model."""
    import bitcount_model as bcm
    ctx = world()
    c, a, _ = upload(H, ctx, "count", name)
    for op in synth.COUNT_CASES[name][1]:
        cls = getattr(H, "Homomorphic" + "".join(w.title() for w in op.split("_")))
        out = ctx.bit_count(cls, a)
        ob, _, rl, rd = synth.count_reference(name, op)
        same(out, ob, rl, rd, c["n"], f"{op} {name}")
    assert set(synth.COUNT_CASES[name][1]) <= set(bcm.OPS)
    ctx.synchronize()


@pytest.mark.parametrize("what", ["read", "write"])
@pytest.mark.parametrize("name", list(synth.ARRAY_CASES))
def test_array(H, world, name, what):
    """array_read_kernel and array_write_kernel (kernels.hip) in plan_array_read's / plan_array_write's
    layouts (array_host.h; a wave's slice within 2560 words).  Read: a level-t join is
    wave_mul<kQSmall, 8>(s_t, ns, V, nv, Add, nadd, ..) with V = L + R; write: wave_mul(X, nx, Q0,
    nind, T, nt, O) with X = x_j + T_j uniform and Q0 the element's indicator.  8 scheduled arrays
    (element v's kinds shifted by v, the index bits and the written value on schedules of their
    own), then one FULL element among elements one below their bound, then all FULL under an x one
    below.  Paths (synth.check_array_path):
      w1_edge        count 4, index 255 x 2, elements and x at 1535: the read's level-1 product
                     8 + 56 = 64 words, the write's ind (x + T) 16 + 48 = 64
      w2_edge        ... at 1567: 8 + 57 = 65 and 16 + 49 = 65
      count5_per_bit count 5 (k = 3, no power of two: the last element rises alone), elements
                     63 + 97 i, x 700 - 83 i
    Every level's node buffer, the root's included, and the write's X and O are filled.  Bit-exact
    against array_model."""
    ctx = world()
    c = synth.inputs("array", name)
    la, da, ls, ds, lx, dx = synth.packed("array", name)
    arr = _from_host(H, ctx, la, da, c["ba"], c["n"] * c["count"])
    idx = _from_host(H, ctx, ls, ds, c["bb"], c["n"])
    if what == "read":
        out = ctx.array_read(arr, idx, c["count"])
        nout = c["n"]
    else:
        x = _from_host(H, ctx, lx, dx, c["bc"], c["n"])
        out = ctx.array_write(arr, idx, x, c["count"])
        nout = c["n"] * c["count"]
    ctx.synchronize()
    ob, _, rl, rd = synth.array_reference(name, what)
    same(out, ob, rl, rd, nout, f"array {what} {name}")
