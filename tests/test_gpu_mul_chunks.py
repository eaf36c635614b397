"""GPU: the carry-save multiplier's chunk loop, its staging checks and its plans with K > 32.

mul_columns (mul_host.cpp) cuts a batch into chunks of `budget / per_value` values that share one
workspace; on an otherwise empty device every batch the suite runs is one chunk, so MulBase::e0
was always 0 and MulBase::nv always n.  hm_ctx_set_mul_chunk (a test hook) caps the chunk; here
the cases and cached references of tests/synth.py run chunked and must give the unchunked
reference bit for bit (limbs, degree words, out.bound: no tolerance), a chunk of short or null
values follows a chunk of full ones in an arena nothing clears, corrupted operands are refused with
HM_ERR_BAD_INPUT by both staging kernels at e0 > 0, and bound-0 u64 operands reach
mul_stage_kernel and the plans with K = 33, 40 and 64 (paths: synth.check_mul_wide_path, pinned to
integer arithmetic by test_synth_reference.py).
"""
import numpy as np
import pytest

import synth
from helpers import assert_batches_equal, plain

pytestmark = pytest.mark.gpu

PRODUCTS = ("mfma", "valu")


@pytest.fixture(scope="module")
def H():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import homomorph
    homomorph.lib()  # loud failure if the engine is not built
    return homomorph


def make_ctx(H, params=synth.PARAMS):
    ctx = H.Context(H.Parameters(*params))
    ctx.seed_rng(synth.SEED)
    ctx.generate_secret_key()
    ctx.generate_public_key()
    return ctx


@pytest.fixture(scope="module")
def ctx(H):
    return make_ctx(H)


def from_host(H, ctx, packed, bound, n):
    return H.Ciphered.from_host(packed[0], packed[1], bound, n, ctx.device, None)


def same(out, ob, rl, rd, n, what):
    assert np.array_equal(out.bound, ob), what
    gl, gd = out.to_host()
    assert_batches_equal(gl, gd, rl, rd, ob, n, what)


def multiply(H, ctx, a, b, spec, products="auto", chunk=0):
    """One multiply under the case's options, synchronized; every option is put back."""
    ctx.set_mul_products(products)
    ctx.set_mul_chunk(chunk)
    if spec.get("ka"):
        ctx.set_mul_options(*spec["ka"])
    try:
        if spec["k"]:
            out = ctx.mul_low(a, b, spec["k"])
        else:
            out = ctx.apply2(H.HomomorphicMultiplication, a, b, signed=spec["signed"])
        ctx.synchronize()
    finally:
        ctx.set_mul_products("auto")
        ctx.set_mul_chunk(0)
        ctx.set_mul_options()
    return out


# ------------------------------------------------------------------ B1: chunked = unchunked
@pytest.mark.parametrize("chunk", [1, 3, 4])
@pytest.mark.parametrize("products", PRODUCTS)
@pytest.mark.parametrize("case", synth.CHUNK_CASES, ids=lambda c: c[1])
def test_chunked_equals_reference(H, ctx, case, products, chunk):
    """The smallest case per launch family of test_gpu_full_bounds.py (n = 10 each), cut into 10
    chunks of 1, into 3 + 3 + 3 + 1 (a last block with one live wave after blocks with three) and
    into 4 + 4 + 2, against the case's unchunked reference (synth.mul_reference,
    mul_class_reference):
      u8_b128, i8_b128    the full circuit; the signed column's flipped VALU partial products
      u16_low4_per_bit    operand stride different from the slot sizes, K < L
      ppv_12w, ppg_tiny_13w, ppg_gen_33w   the three grouped partial-product launches
      rows_v36, ppm_wide  mul_rows_kernel; per-column partial products on the wide MFMA instance
      u8_b640_full        four Karatsuba programs on both lanes: the fork to the auxiliary stream
                          and the join once per column per chunk, the next chunk's memset and
                          staging behind the join
      u8_b703_ka224       lean Karatsuba leaves
    Every output limb and degree word is addressed with e0 + e, every deg1 row with the chunk's own
    nv.  All ten cases run at all three chunk sizes (the slowest, u8_b703_ka224 at chunk 1, takes
    well under a second)."""
    family, name = case
    spec, reference = synth.mul_spec(family, name)
    c = synth.inputs(family, name)
    assert c["n"] == 10
    la, da, lb, db = synth.packed(family, name)
    a, b = from_host(H, ctx, (la, da), c["ba"], c["n"]), from_host(H, ctx, (lb, db), c["bb"], c["n"])
    out = multiply(H, ctx, a, b, spec, products, chunk)
    ob, _, rl, rd = reference(name)
    same(out, ob, rl, rd, c["n"], f"{name}/{products}/chunk {chunk}")


@pytest.mark.parametrize("products", PRODUCTS)
def test_chunked_split_karatsuba_plan(H, products):
    """test_gpu_properties.py::test_mul_karatsuba_split_plans_equal_whole's plan at its own size
    (u32 mul_low(16) of 4 fresh values at d = d' = 128, scratch limit 2^18 words: every Karatsuba
    product above it planned one subtree at a time), unchunked and then in chunks of 1 and of 3
    (3 + 1): identical ciphertexts.  (n = 4, so a chunk of 4 would be the unchunked run.)"""
    params, n, k = (128, 128, 1, 128), 4, 16
    ctx = make_ctx(H, params)
    a, b = plain(n, np.uint32, 142), plain(n, np.uint32, 143)
    ca, cb = ctx.encrypt(a), ctx.encrypt(b)
    ctx.set_mul_scratch(1 << 18)
    spec = dict(k=k, signed=False)
    whole = multiply(H, ctx, ca, cb, spec, products, 0)
    wl, wd = whole.to_host()
    for chunk in (1, 3):
        got = multiply(H, ctx, ca, cb, spec, products, chunk)
        same(got, whole.bound, wl, wd, n, f"split plan/{products}/chunk {chunk}")


# ------------------------------------------------------------------ B2: a stale arena
@pytest.mark.parametrize("chunk", [1, 4])
@pytest.mark.parametrize("products", PRODUCTS)
@pytest.mark.parametrize("name", synth.STALE_LADDERS)
def test_descending_ladders(H, ctx, name, products, chunk):
    """The arena is not cleared between chunks and mul_scan_kernel reads every item slot at its
    static width, so every producer must zero-fill its slot whatever the value's degrees are.  The
    degree ladders (value e's a_i has e + 1 words) with the widest value FIRST, operands and
    reference rows permuted alike (synth.descending): every chunk after the first meets slots last
    written by longer operands, through the general grouped launch (ladder_ppg_gen, 33 values), the
    per-column MFMA partial products (ladder_ppm, 35) and mul_rows_kernel (ladder_rows, 9)."""
    c = synth.inputs("mulc", name)
    la, da, lb, db, ob, rl, rd = synth.descending(name)
    a, b = from_host(H, ctx, (la, da), c["ba"], c["n"]), from_host(H, ctx, (lb, db), c["bb"], c["n"])
    out = multiply(H, ctx, a, b, synth.MUL_CLASS_CASES[name], products, chunk)
    same(out, ob, rl, rd, c["n"], f"{name} descending/{products}/chunk {chunk}")


@pytest.mark.parametrize("chunk", [1, 4])
@pytest.mark.parametrize("products", PRODUCTS)
@pytest.mark.parametrize("name", synth.STALE_LADDERS)
def test_full_then_null_or_unit_chunks(H, ctx, name, products, chunk):
    """synth.interleaved: over each ladder case's bounds, blocks of 4 values: all FULL; a or b all
    NULL under a FULL other operand (every partial product, prefix and carry null); all FULL; a
    and b UNIT, or one of them UNIT (products of one word, or copies).  In chunks of 4 every null
    or short chunk runs in the slots a full chunk filled; in chunks of 1 value 4 follows value 3.
    Then the same hazard across calls, which exists without any chunk limit: the FULL block and
    then the NULL block and the UNIT block as three unchunked multiplies on the one context."""
    c = synth.interleaved(name)
    spec = synth.MUL_CLASS_CASES[name]
    a, b = from_host(H, ctx, c["a"], c["ba"], c["n"]), from_host(H, ctx, c["b"], c["bb"], c["n"])
    out = multiply(H, ctx, a, b, spec, products, chunk)
    rl, rd = c["ref"]
    same(out, c["ob"], rl, rd, c["n"], f"{name} interleaved/{products}/chunk {chunk}")
    if chunk != 1:
        return
    stride = int((c["ob"] // 64 + 1).sum())
    for lo in (0, 4, 12):  # FULL, then NULL, then UNIT: successive calls, unchunked
        hi = lo + synth.STALE_BLOCK
        got = multiply(H, ctx, H.value_slice(a, lo, hi), H.value_slice(b, lo, hi), spec, products, 0)
        same(got, c["ob"], rl[lo * stride: hi * stride], rd[lo * spec["k"]: hi * spec["k"]],
             synth.STALE_BLOCK, f"{name} successive calls/{products}/values {lo}..{hi}")


# ------------------------------------------------------------------ B3: in a captured graph
def test_chunked_graph_replay_equals_direct_call(H, ctx):
    """hm_mul_batch with a chunk of 3 (3 + 3 + 3 + 1 on u8_b128) captured into a graph: the replay
    into buffers prefilled with -1 writes every limb and degree word and equals the direct call
    and the reference."""
    import torch
    c = synth.inputs("mul", "u8_b128")
    la, da, lb, db = synth.packed("mul", "u8_b128")
    a, b = from_host(H, ctx, (la, da), c["ba"], c["n"]), from_host(H, ctx, (lb, db), c["bb"], c["n"])
    ob, _, rl, rd = synth.mul_reference("u8_b128")
    ctx.set_mul_chunk(3)
    try:
        direct = ctx.apply2(H.HomomorphicMultiplication, a, b, signed=False)
        got = H.Ciphered.empty(c["n"], direct.bound, ctx.device, None)
        g = ctx.graph(lambda: H.mul_into(ctx, a, b, got))
        got.limbs.fill_(-1)
        got.degree.fill_(-1)
        torch.cuda.synchronize()  # the fills ran on torch's stream, the replay on the engine's
        g.replay()
        ctx.synchronize()
    finally:
        ctx.set_mul_chunk(0)
    wl, wd = direct.to_host()
    same(got, direct.bound, wl, wd, c["n"], "graph replay vs direct call")
    same(got, ob, rl, rd, c["n"], "graph replay vs reference")


# ------------------------------------------------------------------ B4: the workspace's size
def test_chunk_limit_sizes_the_workspace(H):
    """set_mul_chunk(2), then u8_b128's 10 values on a fresh context: the workspace is sized for
    the chunk, not the batch.  The ABI exposes no workspace size; hm_ctx_generation advances
    whenever a workspace is replaced, which bounds it from both sides: an unchunked multiply of 2
    values of the same plan then leaves the generation alone (the workspace holds 2 values), and
    one of 3 values advances it (it did not hold 3)."""
    ctx = make_ctx(H)
    c = synth.inputs("mul", "u8_b128")
    la, da, lb, db = synth.packed("mul", "u8_b128")
    a, b = from_host(H, ctx, (la, da), c["ba"], c["n"]), from_host(H, ctx, (lb, db), c["bb"], c["n"])
    ob, _, rl, rd = synth.mul_reference("u8_b128")
    spec = dict(k=None, signed=False)
    stride = int((ob // 64 + 1).sum())
    out = multiply(H, ctx, a, b, spec, "auto", 2)
    same(out, ob, rl, rd, c["n"], "chunk 2")
    gen = ctx.generation()
    for n, grows in ((2, False), (3, True)):
        got = multiply(H, ctx, H.value_slice(a, 0, n), H.value_slice(b, 0, n), spec, "auto", 0)
        same(got, ob, rl[:n * stride], rd[:n * 8], n, f"unchunked, {n} values")
        assert (ctx.generation() != gen) == grows, (n, gen, ctx.generation())


# ------------------------------------------------------------------ C: staging validation
def _refused(H, ctx, launch, what):
    from homomorph import _lib
    launch()
    with pytest.raises(H.EngineError) as ei:
        ctx.synchronize()
    assert ei.value.status == _lib.ERR_BAD_INPUT, what


@pytest.mark.parametrize("operand", ["a", "b"])
@pytest.mark.parametrize("how", synth.CORRUPTIONS)
def test_mul_staging_refuses_corrupted_operands(H, ctx, how, operand):
    """mul_stage_value_kernel carries its own restatement of load_bit's validation (degree above
    bound, bits above the degree, top coefficient clear, nonzero limbs past the degree's limb).
    u8 at the uniform bound 383, the 8 scheduled values (synth.stage_inputs); one corruption
    (synth.corrupt, inside the bit's own limbs and degree word) in a value with index >= 3
    (synth.corruption_site), the batch rebuilt with Ciphered.from_host: mul_low(4) and the full
    multiply raise HM_ERR_BAD_INPUT at synchronize, unchunked and in chunks of 3, where the
    corrupted value is read at e0 > 0.  A clean multiply on the same context afterwards equals the
    reference: the flag was cleared and the workspace is usable.  degree_above_bound sets the
    degree word to exactly bound + 1."""
    c = synth.stage_inputs()
    X = c[operand.upper()]
    e, i = synth.corruption_site(X, c["ba"], how, range(4))
    assert e >= synth.STAGE_CHUNK
    bad = synth.corrupt(*c[operand], c["ba"], c["n"], e, i, how)
    if how == "degree_above_bound":
        assert bad[1].reshape(c["n"], 8)[e, i] == synth.STAGE_BOUND + 1
    good = {"a": from_host(H, ctx, c["a"], c["ba"], c["n"]),
            "b": from_host(H, ctx, c["b"], c["bb"], c["n"])}
    ops = dict(good)
    ops[operand] = from_host(H, ctx, bad, c["ba"], c["n"])
    try:
        for chunk in (0, synth.STAGE_CHUNK):
            ctx.set_mul_chunk(chunk)
            what = f"{how} in {operand}[{e}][{i}], chunk {chunk}"
            _refused(H, ctx, lambda: ctx.mul_low(ops["a"], ops["b"], 4), "mul_low(4): " + what)
            _refused(H, ctx, lambda: ctx.apply2(H.HomomorphicMultiplication, ops["a"], ops["b"],
                                                signed=False), "full: " + what)
            for ref, k in (("low4", 4), ("full", None)):
                out = multiply(H, ctx, good["a"], good["b"], dict(k=k, signed=False), "auto", chunk)
                ob, _, rl, rd = synth.stage_reference(ref)
                same(out, ob, rl, rd, c["n"], f"clean {ref} after {what}")
    finally:
        ctx.set_mul_chunk(0)


@pytest.mark.parametrize("operand", ["a", "b"])
def test_mul_low_does_not_read_bits_at_or_above_k(H, ctx, operand):
    """hm_mul_low_batch(k = 4) on the 8-bit operands stages input bits 0..3 only: each of the four
    corruptions in bit 5 is not looked at, and the result equals the reference (as
    test_gpu_shift.py::test_corrupted_degree_words shows for the amount's high bits)."""
    c = synth.stage_inputs()
    ob, _, rl, rd = synth.stage_reference("low4")
    good = {"a": from_host(H, ctx, c["a"], c["ba"], c["n"]),
            "b": from_host(H, ctx, c["b"], c["bb"], c["n"])}
    for how in synth.CORRUPTIONS:
        e, i = synth.corruption_site(c[operand.upper()], c["ba"], how, [5])
        ops = dict(good)
        ops[operand] = from_host(H, ctx, synth.corrupt(*c[operand], c["ba"], c["n"], e, i, how),
                                 c["ba"], c["n"])
        for chunk in (0, synth.STAGE_CHUNK):
            out = multiply(H, ctx, ops["a"], ops["b"], dict(k=4, signed=False), "auto", chunk)
            same(out, ob, rl, rd, c["n"], f"{how} in {operand}[{e}][5], chunk {chunk}")


@pytest.mark.parametrize("how", synth.CORRUPTIONS)
def test_gates_refuse_corrupted_operands(H, ctx, how):
    """gate_kernel reads its operands through load_bit (dev_common.h): hm_gate_batch refuses the
    same four corruptions, AND in a bit of a and in a bit of b, NOT in a bit of a, and a clean gate
    on the same context afterwards equals the reference."""
    c = synth.stage_inputs()
    for op, cls, operand in (("and", H.HomomorphicAndGate, "a"), ("and", H.HomomorphicAndGate, "b"),
                             ("not", H.HomomorphicNotGate, "a")):
        e, i = synth.corruption_site(c[operand.upper()], c["ba"], how, range(8))
        ops = {"a": from_host(H, ctx, c["a"], c["ba"], c["n"]),
               "b": from_host(H, ctx, c["b"], c["bb"], c["n"])}
        ops[operand] = from_host(H, ctx, synth.corrupt(*c[operand], c["ba"], c["n"], e, i, how),
                                 c["ba"], c["n"])
        what = f"{op}: {how} in {operand}[{e}][{i}]"
        if op == "not":
            _refused(H, ctx, lambda: ctx.apply1(cls, ops["a"]), what)
        else:
            _refused(H, ctx, lambda: ctx.apply2(cls, ops["a"], ops["b"]), what)
        a, b = from_host(H, ctx, c["a"], c["ba"], c["n"]), from_host(H, ctx, c["b"], c["bb"], c["n"])
        out = ctx.apply1(cls, a) if op == "not" else ctx.apply2(cls, a, b)
        ctx.synchronize()
        ob, _, rl, rd = synth.stage_reference(op)
        same(out, ob, rl, rd, c["n"], "clean after " + what)


# ------------------------------------------------------------------ D: plans with K > 32
def _wide_spec(name):
    K, signed = synth.WIDE_CASES[name]
    return dict(k=K if K < 64 else None, signed=signed)


@pytest.mark.parametrize("chunk", [0, 4])
@pytest.mark.parametrize("products", PRODUCTS)
@pytest.mark.parametrize("name", list(synth.WIDE_CASES))
def test_wide_plans(H, ctx, name, products, chunk):
    """u64 operands whose every bit has bound 0 (null or unit polynomials), n = 6: all NULL, all
    UNIT, alternating bits, two random patterns, 2^63 + 1 (synth.wide_values).  mul_low at K = 33
    and 40, the full K = 64 multiply unsigned and signed.  2 K > 64, so launch_mul_stage takes
    mul_stage_kernel (one wave per (value, bit)) with MulStageArgs up to K = 64; column i's scan
    has 1 + i (i + 1) / 2 items, 2017 in the last (synth.check_mul_wide_path, from the planner's
    census); every column meets null and unit short-circuits.  The reference, gf2_model.mul_circuit,
    equals the integer product mod 2^K there (test_synth_reference.py).  Unchunked, and in chunks
    of 4 + 2."""
    c = synth.wide_inputs()
    a, b = from_host(H, ctx, c["a"], c["ba"], c["n"]), from_host(H, ctx, c["b"], c["bb"], c["n"])
    out = multiply(H, ctx, a, b, _wide_spec(name), products, chunk)
    ob, _, rl, rd = synth.wide_reference(name)
    same(out, ob, rl, rd, c["n"], f"{name}/{products}/chunk {chunk}")


@pytest.mark.parametrize("how", synth.CORRUPTIONS)
def test_wide_staging_refuses_corrupted_operands(H, ctx, how):
    """stage_one (mul_stage_kernel) carries the same validation.  At bound 0 a bit has one limb and
    nothing past its degree's limb, so the K = 33 plan runs with a_32 at bound 64 (two limbs;
    synth.wide_stage_inputs: degrees 0 .. 64 there; the plan's census:
    test_synth_reference.py::test_wide_stage_reference): a clean run equals the model, and each
    corruption of a_32 in a value with index >= 4 is refused, unchunked and in chunks of 4 (e0 > 0),
    with a clean run after it."""
    c = synth.wide_stage_inputs()
    i = synth.WIDE_STAGE_BIT
    e, _ = synth.corruption_site(c["A"], c["ba"], how, [i], first=4)
    a, b = from_host(H, ctx, c["a"], c["ba"], c["n"]), from_host(H, ctx, c["b"], c["bb"], c["n"])
    bad = from_host(H, ctx, synth.corrupt(*c["a"], c["ba"], c["n"], e, i, how), c["ba"], c["n"])
    rl, rd = c["ref"]
    try:
        for chunk in (0, 4):
            ctx.set_mul_chunk(chunk)
            _refused(H, ctx, lambda: ctx.mul_low(bad, b, c["K"]), f"{how} in a[{e}][{i}], chunk {chunk}")
            out = multiply(H, ctx, a, b, dict(k=c["K"], signed=False), "auto", chunk)
            same(out, c["ob"], rl, rd, c["n"], f"clean K = 33 after {how}, chunk {chunk}")
    finally:
        ctx.set_mul_chunk(0)
