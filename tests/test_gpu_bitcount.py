"""GPU: homomorphic bit counts (hm_bitcount_batch: count_ones, count_zeros, leading / trailing
zeros / ones) against the model circuits (tests/bitcount_model.py over oracle/gf2_model.py),
bit-exact.

The pattern of tests/test_gpu_shift.py: both sides get identical seeded keys, masks and
plaintexts; every case checks the limbs and the degree words against the model, the bounds against
the model, the decrypted results against int.bit_count and bit scans, and a clean
ctx.synchronize().  Shapes are the smallest that reach each path of the kernels:
a count with and without the running product past its slots (a power of two, 24 and 3 bits), both
ends of a run, the zeros literals, null and unit literals (every skip and the early end of a run),
operands that fill their bounds, a batch that is no multiple of a block's four waves.
"""
import ctypes

import numpy as np
import pytest

import bitcount_model as bcm
import synth
from circuit_gpu import encrypt_both, load_engine, make_world
from helpers import assert_batches_equal, plain

gpu = pytest.mark.gpu

U8, U16, U32 = (64, 64, 1, 64), (64, 32, 1, 32), (128, 128, 1, 128)
SEED = 2027
OPS = tuple(bcm.OPS)


@pytest.fixture(scope="module")
def H():
    return load_engine()


@pytest.fixture(scope="module")
def world(H, oracle):
    return make_world(H, SEED)


def marker(H, op):
    return {"count_ones": H.HomomorphicCountOnes, "count_zeros": H.HomomorphicCountZeros,
            "leading_zeros": H.HomomorphicLeadingZeros, "leading_ones": H.HomomorphicLeadingOnes,
            "trailing_zeros": H.HomomorphicTrailingZeros,
            "trailing_ones": H.HomomorphicTrailingOnes}[op]


def assert_equals_model(out, values, what):
    """The device batch against the model's bit polynomials per value, limbs and degree words."""
    el, ed = bcm.pack(values, out.bound)
    gl, gd = out.to_host()
    assert_batches_equal(gl, gd, el, ed, out.bound, out.n, what)


def check_count(H, ctx, op, a, A, ints=None, what=""):
    """bit_count(op, a) of a device batch (model polynomials A; ints: the plaintext integers, or
    None when a does not decrypt to anything meaningful)."""
    out = ctx.bit_count(marker(H, op), a)
    assert out.nbits == 8 and out.n == a.n and out.plain_dtype == np.dtype(np.uint8)
    assert np.array_equal(out.bound, bcm.bitcount_bounds(op, a.bound)), what
    assert_equals_model(out, [bcm.circuit(op, A[e]) for e in range(a.n)], what)
    if ints is not None:
        got = ctx.decrypt(out)
        assert got.dtype == np.uint8
        assert got.tolist() == [bcm.int_count(op, int(x), a.nbits) for x in ints], what
    ctx.synchronize()
    return out


def synthetic(H, ctx, values, bound, dtype=None):
    """A device batch of the model polynomials `values` at the per-bit bounds."""
    bound = np.asarray(bound, dtype=np.uint32)
    return H.Ciphered.from_host(*bcm.pack(values, bound), bound, len(values), ctx.device, dtype)


FIVE = np.array([0x00, 0xFF, 0x80, 0x01, plain(1, np.uint8, 3)[0]], np.uint8)


@pytest.fixture(scope="module")
def five(H, oracle, world):
    """The first case's batch, shared and left unchanged: u8 values at (64,64,1,64); five is no
    multiple of the four waves of a block."""
    return encrypt_both(H, oracle, world, U8, FIVE, 11)


@gpu
@pytest.mark.parametrize("op", OPS)
def test_u8_five_values(H, world, five, op):
    ctx, _ = world(U8)
    a, A = five
    out = check_count(H, ctx, op, a, A, FIVE, what=f"u8 {op}")
    # apply1 routes the markers to ctx.bit_count
    via = ctx.apply1(marker(H, op), a)
    assert_batches_equal(*via.to_host(), *out.to_host(), out.bound, 5, f"apply1 {op}")


@gpu
@pytest.mark.parametrize("op", OPS)
def test_u8_equals_the_lookup(H, world, five, op):
    """The multilinear form of a function of a byte is unique, so the count circuits and the
    existing table lookup give the same polynomials: limb for limb, degree for degree."""
    ctx, _ = world(U8)
    a, _ = five
    out = ctx.bit_count(marker(H, op), a)
    ref = ctx.lookup(a, bcm.table(op))
    # (the widest monomial of every output bit is the circuit's own widest term: equal bounds)
    assert np.array_equal(out.bound, ref.bound) and ref.plain_dtype == out.plain_dtype
    assert_batches_equal(*out.to_host(), *ref.to_host(), out.bound, 5, f"{op}: against the lookup")
    assert np.array_equal(ctx.decrypt(out), ctx.decrypt(ref))
    ctx.synchronize()


@gpu
def test_u16_skewed_bounds(H, oracle, world):
    """n = 4 at (64,32,1,32), a's bounds fresh + 37 i: a count's bit k takes the 2^k LARGEST
    bounds, not the first; a run sums them in its own order (at a power of two every output bit of
    a run reaches the last literal, so both ends have the sum of all; the 24-bit case below has
    ends that differ)."""
    ctx, _ = world(U16)
    fresh = U16[0] + U16[1]
    av = np.concatenate([np.array([0x8001, 0xFFFF], np.uint16), plain(2, np.uint16, 31)])
    bound = (fresh + 37 * np.arange(16)).astype(np.uint32)
    a, A = encrypt_both(H, oracle, world, U16, av, 33, bound=bound)
    outs = {op: check_count(H, ctx, op, a, A, av, what=f"u16 skew {op}") for op in OPS}
    c = outs["count_ones"].bound
    assert c.tolist() == [int(np.sort(bound)[::-1][:1 << k].sum()) for k in range(5)] + [0] * 3
    assert c[2] != bound[:4].sum() and c[2] == bound[12:].sum()
    for op in OPS[2:]:
        assert outs[op].bound.tolist() == [int(bound.sum())] * 5 + [0] * 3


U32_VALUES = np.array([0x80000001, 0xFFFFFFFF, plain(1, np.uint32, 5)[0]], np.uint32)


@pytest.fixture(scope="module")
def u32_batches(H, oracle, world):
    """Shared and left unchanged: three u32 values, and 0 as a batch of its own."""
    return (encrypt_both(H, oracle, world, U32, U32_VALUES, 21),
            encrypt_both(H, oracle, world, U32, np.zeros(1, np.uint32), 22))


@gpu
@pytest.mark.parametrize("op", OPS)
def test_u32_headline_parameters(H, world, u32_batches, op):
    """(128,128,1,128): three values, and 0 in a call of its own."""
    ctx, _ = world(U32)
    (a, A), (z, Z) = u32_batches
    out = check_count(H, ctx, op, a, A, U32_VALUES, what=f"u32 {op}")
    if bcm.OPS[op][0]:
        assert out.bound.tolist() == [32 * 256] * 6 + [0, 0]
    else:
        assert out.bound[5] == 32 * 256 and out.bound.tolist() == [256 << k for k in range(6)] + [0, 0]
    check_count(H, ctx, op, z, Z, [0], what=f"u32 {op} of 0")


@gpu
@pytest.mark.parametrize("nbits", [3, 24])
def test_widths_that_are_no_power_of_two(H, oracle, world, nbits):
    """The low 3 and 24 bits of encrypted u32 values as batches of their own (synthetic, skewed
    bounds): a count without the running product (its top target 2 or 16 is a slot), runs whose
    output bits end at different literals.  The u8 output still decrypts."""
    ctx, _ = world(U8)
    fresh = U8[0] + U8[1]
    av = np.concatenate([np.array([0xFFFFFF, 0x800001, 0], np.uint32), plain(2, np.uint32, 41)])
    bound = (fresh + 11 * np.arange(32)).astype(np.uint32)
    _, A = encrypt_both(H, oracle, world, U8, av, 42, bound=bound)
    A = [v[:nbits] for v in A]
    a = synthetic(H, ctx, A, bound[:nbits])
    ints = [int(x) & ((1 << nbits) - 1) for x in av]
    outs = {op: check_count(H, ctx, op, a, A, ints, what=f"{nbits} bits {op}") for op in OPS}
    lead, trail = outs["leading_zeros"].bound, outs["trailing_zeros"].bound
    assert not np.array_equal(lead, trail)
    if nbits == 24:
        b = bound[:24].astype(np.int64)
        # bit 4 of a run sums t_16 only; a count's bit 4 is e_16
        assert lead[4] == b[8:].sum() and trail[4] == b[:16].sum() and lead[3] == b.sum()
        assert outs["count_ones"].bound[4] == b[8:].sum()
        e = 3
        t16 = bcm.run_circuit(A[e], False, True)[4]
        prod = 1
        for x in A[e][:7:-1]:
            prod = bcm.model.clmul_fast(prod, x)
        assert t16 == prod
    else:
        assert lead.tolist() == [int(bound[:3].sum()), int(bound[1:3].sum())] + [0] * 6
        assert trail.tolist() == [int(bound[:3].sum()), int(bound[:2].sum())] + [0] * 6


@gpu
def test_trivial_ciphertexts(H, world):
    """Synthetic values whose bits are null or unit polynomials (plaintext bits): all null, all
    unit, a null in the middle of units, a unit in the middle of nulls, and one fresh-looking bit
    among them.  Every product is skipped or ends the run early; the zeros ops exchange the
    roles.  The outputs are the plain bits of the integer result."""
    ctx, _ = world(U8)
    bound = np.full(8, 128, np.uint32)
    pats = [0x00, 0xFF, 0xEF, 0x10, 0xF7, 0x7F, 0xFE]
    vals = [[(p >> i) & 1 for i in range(8)] for p in pats]
    a = synthetic(H, ctx, vals, bound, np.dtype(np.uint8))
    for op in OPS:
        out = check_count(H, ctx, op, a, vals, pats, what=f"trivial {op}")
        want = [[(bcm.int_count(op, p, 8) >> k) & 1 for k in range(8)] for p in pats]
        assert_equals_model(out, want, f"trivial {op}: plain bits")
    # a non-trivial polynomial in the middle of trivial ones, and after a null (never multiplied)
    rng = np.random.default_rng(5)
    x = synth.poly("FULL", 128, rng)
    mixed = [[1, 1, x, 1, 1, 1, 1, 1], [1, 0, x, 1, 1, 1, 0, 1], [0, 0, x, 0, 0, 0, 0, 0],
             [x, 1, 1, 1, 1, 1, 1, x]]
    m = synthetic(H, ctx, mixed, bound)
    for op in OPS:
        check_count(H, ctx, op, m, mixed, what=f"mixed {op}")


@gpu
def test_one_word_literals(H, world):
    """Bits of degree 1..31 (one 32-bit word that is neither the unit polynomial nor null) at a
    bound below 32, next to null and unit bits, at both ends of the value and in its middle.  A
    zeros op flips coefficient 0: 0b11 becomes 0b10, still one word and not null; only the unit
    polynomial becomes null."""
    ctx, _ = world(U8)
    bound = np.full(8, 31, np.uint32)
    top = (1 << 31) | 1
    vals = [[0b11, 0b10, 0b111, 1, 0, 0b101, top, 0b11],
            [0b11] * 8,
            [0b10, 0b11, 1, 1, 0b110, 1, 0b11, 0b10],
            [1, 0b11, 0b11, 0, 0b11, 0b11, 0b111, 1],
            [top, 1 << 31, 0b11, 0b11, 0b11, 0b11, 1 << 31, top]]
    a = synthetic(H, ctx, vals, bound)
    for op in OPS:
        check_count(H, ctx, op, a, vals, what=f"one word {op}")
    # the zeros ops' literal of 0b11 is 0b10: the run goes on through it, e_8 is their product
    out = ctx.bit_count(H.HomomorphicCountZeros, a)
    _, od = out.to_host()
    assert od.reshape(5, 8)[1, 3] == 8  # (X)^8


@gpu
@pytest.mark.parametrize("op", OPS)
def test_u8_below_one_word(H, oracle, world, op):
    """(17,8,1,8), the edge of a u8's requirement: d + d' = 25, every fresh bit is one word and
    about half of them have the constant term 1."""
    P = (17, 8, 1, 8)
    ctx, _ = world(P)
    av = np.concatenate([FIVE, plain(4, np.uint8, 81)])
    a, A = encrypt_both(H, oracle, world, P, av, 82)
    assert sum(p & 1 and p > 1 for v in A for p in v) >= 8  # literals the flip leaves one word
    check_count(H, ctx, op, a, A, av, what=f"(17,8,1,8) {op}")


@gpu
@pytest.mark.parametrize("nbits,base", [(16, 256), (32, 200)])
def test_operands_that_fill_their_bounds(H, world, nbits, base):
    """Exact degree = bound at every bit (strictly increasing bounds, so that the widest term of
    every output is unique and cannot cancel): every output reaches its bound exactly, which a
    short slot or buffer would cut."""
    ctx, _ = world(U32)
    bound = (base + np.arange(nbits)).astype(np.uint32)
    rng = np.random.default_rng(nbits)
    vals = [[synth.poly(kind, b, rng) for b in bound] for kind in ("FULL", "ONES")]
    a = synthetic(H, ctx, vals, bound)
    for op in ("count_ones", "leading_zeros"):
        out = check_count(H, ctx, op, a, vals, what=f"full {nbits} {op}")
        _, od = out.to_host()
        K = nbits.bit_length()
        for e in range(2):
            assert od.reshape(2, 8)[e, :K].tolist() == out.bound[:K].tolist(), (op, e)


@gpu
def test_single_value_and_empty_batch(H, oracle, world):
    ctx, _ = world(U8)
    av = plain(1, np.uint8, 61)
    a, A = encrypt_both(H, oracle, world, U8, av, 62)
    check_count(H, ctx, "count_ones", a, A, av, what="n=1")
    check_count(H, ctx, "trailing_zeros", a, A, av, what="n=1")
    e = H.Ciphered.empty(0, a.bound, ctx.device, np.dtype(np.uint8))
    out = ctx.bit_count(H.HomomorphicLeadingOnes, e)
    assert out.n == 0 and out.nbits == 8
    ctx.synchronize()


@gpu
def test_graph_replay_equals_direct_call(H, world, five):
    """Replays into buffers prefilled with -1: every limb and degree word is written."""
    import torch
    ctx, _ = world(U8)
    a, _ = five
    for op in (H.HomomorphicCountZeros, H.HomomorphicLeadingZeros):
        direct = ctx.bit_count(op, a)
        got = H.Ciphered.empty(5, direct.bound, ctx.device, np.dtype(np.uint8))
        g = ctx.graph(lambda: H.bitcount_into(ctx, op, a, got))
        got.limbs.fill_(-1)
        got.degree.fill_(-1)
        torch.cuda.synchronize()  # the fills ran on torch's stream, the replay on the engine's
        g.replay()
        ctx.synchronize()
        gl, gd = got.to_host()
        wl, wd = direct.to_host()
        assert_batches_equal(gl, gd, wl, wd, direct.bound, 5, "graph replay")
        assert np.array_equal(ctx.decrypt(got), ctx.decrypt(direct))


@gpu
def test_argument_errors(H, world, five):
    """Each returns the documented status and writes nothing."""
    import torch
    from homomorph import _lib
    ctx, _ = world(U8)
    a, _ = five
    INV = _lib.ERR_INVALID_ARGUMENT

    def call(which, a, out):
        ca, co = a._c(), out._c()
        return _lib.lib().hm_bitcount_batch(ctx._h, which, ctypes.byref(ca), ctypes.byref(co))

    need = H.bitcount_out_bounds(H.HomomorphicCountOnes, a.bound)
    out = H.Ciphered.empty(5, need, ctx.device)
    out.limbs.fill_(-1)
    out.degree.fill_(-1)
    torch.cuda.synchronize()
    # out->nbits != 8
    assert call(_lib.OP_COUNT_ONES, a, H.Ciphered.empty(5, np.full(16, 2048, np.uint32), ctx.device)) == INV
    assert call(_lib.OP_COUNT_ONES, a, H.Ciphered.empty(5, need[:4], ctx.device)) == INV
    # n mismatch
    assert call(_lib.OP_COUNT_ONES, a, H.Ciphered.empty(4, need, ctx.device)) == INV
    # an out bound one below need, in bit 0 and in the top bit that is not null
    for k in (0, 3):
        low = need.copy()
        low[k] -= 1
        short = H.Ciphered(out.limbs, out.degree, low, 8, 5)
        assert call(_lib.OP_COUNT_ONES, a, short) == INV
    # a which outside the six
    for which in (_lib.OP_ROTR, _lib.OP_LOOKUP, _lib.OP_NOT, 28):
        assert call(which, a, out) == INV
    # null batches
    ca, co = a._c(), out._c()
    assert _lib.lib().hm_bitcount_batch(ctx._h, _lib.OP_COUNT_ONES, None, ctypes.byref(co)) == INV
    assert _lib.lib().hm_bitcount_batch(ctx._h, _lib.OP_COUNT_ONES, ctypes.byref(ca), None) == INV
    ctx.synchronize()
    torch.cuda.synchronize()
    assert bool((out.limbs == -1).all()) and bool((out.degree == -1).all())  # nothing was written
    # out overlapping a: its limbs, or its degree words alone; a is left as it was
    al, ad = a.to_host()
    other = H.Ciphered.empty(5, need, ctx.device)
    assert call(_lib.OP_COUNT_ONES, a, H.Ciphered(a.limbs, other.degree, need, 8, 5)) == INV
    assert call(_lib.OP_COUNT_ONES, a, H.Ciphered(other.limbs, a.degree, need, 8, 5)) == INV
    ctx.synchronize()
    assert_batches_equal(*a.to_host(), al, ad, a.bound, 5, "a after refused calls")
    # larger out bounds are accepted
    assert call(_lib.OP_COUNT_ONES, a, H.Ciphered.empty(5, need + 70, ctx.device)) == _lib.OK
    assert call(_lib.OP_COUNT_ONES, a, out) == _lib.OK
    ctx.synchronize()
    # the Python layer
    with pytest.raises(ValueError):
        ctx.bit_count(H.HomomorphicNotGate, a)


@gpu
def test_requirement(H):
    """2m + 1 with m = 2^floor(log2 n) for a count and n for a run."""
    from homomorph import _lib
    L = _lib.lib()
    av = np.array([0x80, 0xFF, 0x5A, 0], np.uint8)
    ctx = H.Context(H.Parameters(32, 16, 1, 8))
    ctx.seed_rng(5)
    ctx.generate_secret_key()
    ctx.generate_public_key()
    a = ctx.encrypt(av)
    for op in OPS:  # u8 needs 17: passes, and decrypts
        got = ctx.decrypt(ctx.bit_count(marker(H, op), a))
        assert got.tolist() == [bcm.int_count(op, int(x), 8) for x in av], op
    ctx.synchronize()
    a16 = ctx.encrypt(np.array([1, 2], np.uint16))
    for op in OPS:  # u16 needs 33
        with pytest.raises(H.OperationError) as ei:
            ctx.bit_count(marker(H, op), a16)
        assert ei.value.required_min_d_over_delta == 33
        assert (ei.value.actual_d, ei.value.actual_delta) == (32, 1)
    tight = H.Context(H.Parameters(32, 16, 2, 8))  # d / delta = 16: one short of a u8's 17
    tight.seed_rng(6)
    tight.generate_secret_key()
    tight.generate_public_key()
    with pytest.raises(H.OperationError) as ei:
        tight.bit_count(H.HomomorphicCountOnes, tight.encrypt(av))
    assert ei.value.required_min_d_over_delta == 17
    assert (ei.value.actual_d, ei.value.actual_delta) == (32, 2)
    out = H.Ciphered.empty(2, H.bitcount_out_bounds(H.HomomorphicCountOnes, a16.bound), ctx.device)
    with pytest.raises(H.EngineError) as ei:
        H.bitcount_into(ctx, H.HomomorphicCountOnes, a16, out)
    assert ei.value.status == _lib.ERR_INVALID_PARAMETERS
    ctx.synchronize()
    # u32 at (64,64,1,64) requires 65
    c64 = H.Context(H.Parameters(64, 64, 1, 64))
    for op in OPS:
        with pytest.raises(H.OperationError) as ei:
            c64.validate_operation(marker(H, op), 32)
        assert ei.value.required_min_d_over_delta == 65
    # the engine's numbers
    wide = H.Context(H.Parameters(300, 64, 1, 8))  # no keys: validation needs none
    req = ctypes.c_uint16()
    for op in OPS:
        which = bcm.CODES[op]
        assert L.hm_validate_operation(wide._h, which, ctypes.byref(req)) == _lib.ERR_INVALID_ARGUMENT
        for nbits, want in ((8, 17), (16, 33), (32, 65), (64, 129), (1, 3),
                            (24, 49 if bcm.OPS[op][0] else 33)):
            assert L.hm_validate_operation_bits(wide._h, which, nbits, ctypes.byref(req)) == _lib.OK
            assert req.value == want, (op, nbits)
        for nbits in (0, 129):
            assert L.hm_validate_operation_bits(wide._h, which, nbits, None) == _lib.ERR_INVALID_ARGUMENT
    wide.validate_operation(H.HomomorphicLeadingZeros, 64)
    with pytest.raises(ValueError):
        wide.validate_operation(H.HomomorphicLeadingZeros)


@gpu
def test_lds_limit_is_refused_before_any_launch(H):
    """A u64 count_ones at (136,120,1,8), fresh bound 256, would keep E_1 .. E_32: refused, the
    output buffer left as it was."""
    import torch
    from homomorph import _lib
    ctx = H.Context(H.Parameters(136, 120, 1, 8))
    ctx.seed_rng(7)
    ctx.generate_secret_key()
    ctx.generate_public_key()
    a = ctx.encrypt(np.array([3, 1 << 63], np.uint64))
    assert (a.bound == 256).all()
    need = H.bitcount_out_bounds(H.HomomorphicCountOnes, a.bound)
    assert need.tolist() == [256 << k for k in range(7)] + [0]
    out = H.Ciphered.empty(2, need, ctx.device, np.dtype(np.uint8))
    out.limbs.fill_(-1)
    out.degree.fill_(-1)
    torch.cuda.synchronize()
    with pytest.raises(H.EngineError) as ei:
        H.bitcount_into(ctx, H.HomomorphicCountOnes, a, out)
    assert ei.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(H.EngineError) as ei:
        ctx.bit_count(H.HomomorphicCountOnes, a)
    assert ei.value.status == _lib.ERR_UNSUPPORTED
    ctx.synchronize()
    torch.cuda.synchronize()
    assert bool((out.limbs == -1).all()) and bool((out.degree == -1).all())


@gpu
def test_corrupted_degree_word(H, oracle, world):
    """A corrupted degree word in any bit of a is flagged at synchronise, for a count and for a
    run from either end; afterwards the flag is clear."""
    from homomorph import _lib
    ctx, _ = world(U16)
    av = plain(4, np.uint16, 71)
    a, _ = encrypt_both(H, oracle, world, U16, av, 73)
    ctx.synchronize()
    for op, bit in (("count_ones", 9), ("leading_zeros", 0), ("trailing_ones", 15)):
        a.degree[2, bit] += 1  # the limbs have no coefficient there (or it is past the bound)
        ctx.bit_count(marker(H, op), a)
        with pytest.raises(H.EngineError) as ei:
            ctx.synchronize()
        assert ei.value.status == _lib.ERR_BAD_INPUT
        a.degree[2, bit] -= 1
        got = ctx.decrypt(ctx.bit_count(marker(H, op), a))
        ctx.synchronize()  # clean: the flag was cleared by the check
        assert got.tolist() == [bcm.int_count(op, int(x), 16) for x in av]
