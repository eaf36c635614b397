"""GPU: homomorphic shifts and rotates by an encrypted amount (hm_shift_batch) against the model
circuit (tests/shift_model.py over oracle/gf2_model.py), bit-exact.

The pattern of tests/test_gpu_lookup.py: both sides get identical seeded keys, masks and
plaintexts; every case checks the limbs and the degree words against the model, the bounds against
the model, the decrypted results against numpy, and a clean ctx.synchronize().  Shapes are the
smallest that reach each path of the kernel: every source map and walking
order, the saved bits of the rotates, null and unit amount bits (skipped stages, the copy-out
path, a last stage that is not stage 0), an amount read in place from a wider batch, more bits
than lanes, a batch that is no multiple of a block's four waves.
"""
import ctypes
import functools

import numpy as np
import pytest

import circuit_gpu
import shift_model as sm
from circuit_gpu import load_engine, make_world
from helpers import assert_batches_equal, bit_ints, plain

gpu = pytest.mark.gpu

U8, U16, U32 = (64, 64, 1, 64), (64, 32, 1, 32), (128, 128, 1, 128)
U64, U128 = (32, 16, 1, 16), (24, 8, 1, 8)
SEED = 2026


@pytest.fixture(scope="module")
def H():
    return load_engine()


@pytest.fixture(scope="module")
def world(H, oracle):
    return make_world(H, SEED)


def marker(H, op):
    return {"shl": H.HomomorphicShiftLeft, "shr": H.HomomorphicShiftRight,
            "rotl": H.HomomorphicRotateLeft, "rotr": H.HomomorphicRotateRight}[op]


encrypt_both = functools.partial(circuit_gpu.encrypt_both, wide=True)  # (u64, u128 as bytes)


def assert_equals_model(out, values, what):
    """The device batch against the model's bit polynomials per value, limbs and degree words."""
    el, ed = sm.pack(values, out.bound)
    gl, gd = out.to_host()
    assert_batches_equal(gl, gd, el, ed, out.bound, out.n, what)


def unsigned(v):
    return v.view(np.dtype(f"u{v.dtype.itemsize}"))


def check_shift(H, ctx, op, a, A, av, s, S, sv, signed=None, what=""):
    """shift(op, a, s) of device batches (model polynomials A, S; plaintexts av, sv).  signed is
    passed on as given; the model and numpy use what it resolves to."""
    out = ctx.shift(marker(H, op), a, s, signed=signed)
    sgn = (a.plain_dtype is not None and np.issubdtype(a.plain_dtype, np.signedinteger)
           if signed is None else signed)
    L = sm.stages(a.nbits)
    assert out.nbits == a.nbits and out.n == a.n and out.plain_dtype == a.plain_dtype
    assert np.array_equal(out.bound, sm.shift_bounds(op, a.bound, s.bound[:L])), what
    assert_equals_model(out, [sm.shift_circuit(op, A[e], S[e][:L], sgn) for e in range(a.n)], what)
    got = ctx.decrypt(out)
    if av.ndim == 1:
        assert got.dtype == av.dtype
        assert np.array_equal(unsigned(got), sm.numpy_shift(op, unsigned(av), sv, sgn)), what
    else:  # wider than numpy's integers: little-endian bytes
        for e in range(a.n):
            x = int.from_bytes(av[e].tobytes(), "little")
            want = sm.int_shift(op, x, int(sv[e]), a.nbits, sgn)
            assert int.from_bytes(got[e].tobytes(), "little") == want, (what, e)
    ctx.synchronize()
    return out


FIVE = np.concatenate([np.array([0x80, 0xFF, 0x01], np.uint8), plain(2, np.uint8, 3)])
FIVE_S = np.array([0, 7, 8, 255, plain(1, np.uint8, 4)[0]], np.uint8)


@pytest.fixture(scope="module")
def five(H, oracle, world):
    """The first case's batches, shared and left unchanged: u8 values and amounts at (64,64,1,64);
    five is no multiple of the four waves of a block."""
    return (encrypt_both(H, oracle, world, U8, FIVE, 11),
            encrypt_both(H, oracle, world, U8, FIVE_S, 12))


@gpu
@pytest.mark.parametrize("op,signed", sm.MODES)
def test_u8_five_values(H, world, five, op, signed):
    ctx, _ = world(U8)
    (a, A), (s, S) = five
    check_shift(H, ctx, op, a, A, FIVE, s, S, FIVE_S, signed=signed, what=f"u8 {op} {signed}")


@gpu
def test_signedness_defaults_from_the_plaintext_dtype(H, world, five):
    """signed=None on an i8 batch is the arithmetic >>, on u8 the logical one."""
    ctx, _ = world(U8)
    (a, A), (s, S) = five
    i8 = H.Ciphered(a.limbs, a.degree, a.bound, 8, a.n, np.dtype(np.int8))
    out = check_shift(H, ctx, "shr", i8, A, FIVE.view(np.int8), s, S, FIVE_S, what="i8 >>")
    assert np.array_equal(ctx.decrypt(out), FIVE.view(np.int8) >> (FIVE_S % 8).astype(np.int8))
    out = check_shift(H, ctx, "shr", a, A, FIVE, s, S, FIVE_S, what="u8 >>")
    assert np.array_equal(ctx.decrypt(out), FIVE >> (FIVE_S % 8))
    # apply2 routes the markers to ctx.shift
    via = ctx.apply2(H.HomomorphicShiftRight, i8, s)
    assert np.array_equal(ctx.decrypt(via), FIVE.view(np.int8) >> (FIVE_S % 8).astype(np.int8))
    ctx.synchronize()


@gpu
@pytest.mark.parametrize("op,signed", sm.MODES)
def test_u32_headline_parameters_u8_amount(H, oracle, world, op, signed):
    """(128,128,1,128), n = 3: the amount is a Ciphered<u8> whose low 5 bits are read."""
    ctx, _ = world(U32)
    av = np.array([0x80000001, 0xFFFFFFFF, plain(1, np.uint32, 5)[0]], np.uint32)
    sv = np.array([0, 31, 33], np.uint8)
    a, A = encrypt_both(H, oracle, world, U32, av, 21)
    s, S = encrypt_both(H, oracle, world, U32, sv, 22)
    out = check_shift(H, ctx, op, a, A, av, s, S, sv, signed=signed, what=f"u32 {op}")
    assert (out.bound == 6 * 256).all() and out.stride == 800


@gpu
def test_u16_skewed_bounds_amount_read_in_place(H, oracle, world):
    """n = 4 at (64,32,1,32): a's bounds fresh + 37 i; the amount is the low 4 bits of a u16 batch
    read in place (degree stride 16) with bounds fresh + 11 t.  SHL and SHR have different bounds
    per bit."""
    ctx, _ = world(U16)
    fresh = U16[0] + U16[1]
    av = np.concatenate([np.array([0x8001, 0xFFFF], np.uint16), plain(2, np.uint16, 31)])
    sv = np.array([1, 15, 0xFFF0 | 9, plain(1, np.uint16, 32)[0]], np.uint16)
    a, A = encrypt_both(H, oracle, world, U16, av, 33,
                        bound=(fresh + 37 * np.arange(16)).astype(np.uint32))
    s, S = encrypt_both(H, oracle, world, U16, sv, 34,
                        bound=(fresh + 11 * np.arange(16)).astype(np.uint32))
    outs = {}
    for op, signed in sm.MODES:
        outs[op, signed] = check_shift(H, ctx, op, a, A, av, s, S, sv, signed=signed,
                                       what=f"u16 skew {op}")
    shl, shr = outs["shl", False].bound, outs["shr", False].bound
    S4 = 4 * fresh + 11 * 6
    assert shl.tolist() == [S4 + fresh + 37 * i for i in range(16)]
    assert shr.tolist() == [S4 + fresh + 37 * 15] * 16
    assert np.array_equal(outs["shr", True].bound, shr)


@gpu
def test_u64_and_u128(H, oracle, world):
    """6 and 7 stages, more bits than lanes: u64 at (32,16,1,16), n = 2; u128 at (24,8,1,8),
    n = 1 (its plaintexts as little-endian bytes)."""
    ctx, _ = world(U64)
    av = np.array([0x8000000000000001, plain(1, np.uint64, 41)[0]], np.uint64)
    sv = np.array([63, 64 + 17], np.uint8)
    a, A = encrypt_both(H, oracle, world, U64, av, 42)
    s, S = encrypt_both(H, oracle, world, U64, sv, 43)
    for op, signed in sm.MODES:
        check_shift(H, ctx, op, a, A, av, s, S, sv, signed=signed, what=f"u64 {op}")
    ctx, _ = world(U128)
    raw = np.random.default_rng(44).integers(0, 256, size=(1, 16), dtype=np.uint8)
    raw[0, 15] |= 0x80
    sv = np.array([128 + 77], np.uint8)
    a, A = encrypt_both(H, oracle, world, U128, raw, 45)
    s, S = encrypt_both(H, oracle, world, U128, sv, 46)
    for op, signed in sm.MODES:
        check_shift(H, ctx, op, a, A, raw, s, S, sv, signed=signed, what=f"u128 {op}")


@gpu
def test_u64_and_u128_at_the_headline_bound(H, oracle, world):
    """One value each at D = 256: the widest shapes of the LDS rule (u128: 150 KB a block, one
    block a CU), on a rotate, whose wide stages save the most bits."""
    ctx, _ = world(U32)
    av = np.array([0x8123456789ABCDEF], np.uint64)
    sv = np.array([37], np.uint8)
    a, A = encrypt_both(H, oracle, world, U32, av, 47)
    s, S = encrypt_both(H, oracle, world, U32, sv, 48)
    check_shift(H, ctx, "rotl", a, A, av, s, S, sv, what="u64 D=256")
    raw = np.random.default_rng(49).integers(0, 256, size=(1, 16), dtype=np.uint8)
    sv = np.array([128 + 93], np.uint8)
    a, A = encrypt_both(H, oracle, world, U32, raw, 50)
    s, S = encrypt_both(H, oracle, world, U32, sv, 51)
    check_shift(H, ctx, "rotr", a, A, raw, s, S, sv, what="u128 D=256")


@gpu
def test_trivial_ciphertexts(H, oracle, world):
    """All-zero masks.  A trivial amount has unit and null bits: the output is a's polynomials
    renumbered (or null), limb for limb; amount 0 gives a itself through the copy-out path.  A
    trivial a under a fresh amount is checked against the model."""
    ctx, _ = world(U8)
    (a, A), (s, S) = (encrypt_both(H, oracle, world, U8, FIVE, 11),
                      encrypt_both(H, oracle, world, U8, FIVE_S, 12))
    tv = np.array([0, 7, 6, 4, 3], np.uint8)  # 6: stages 2 and 1 only; 4: stage 2 alone
    t, T = encrypt_both(H, oracle, world, U8, tv, 51, zero_masks=True)
    assert all(p in (0, 1) for v in T for p in v)
    for op, signed in sm.MODES:
        out = check_shift(H, ctx, op, a, A, FIVE, t, T, tv, signed=signed, what=f"trivial s {op}")
        want = []
        for e in range(5):
            k, x = int(tv[e]) % 8, A[e]
            want.append({"shl": [0] * k + x[:8 - k], "rotl": x[8 - k:] + x[:8 - k],
                         "rotr": x[k:] + x[:k],
                         "shr": x[k:] + [x[7] if signed else 0] * k}[op])
        assert_equals_model(out, want, f"{op}: a's polynomials renumbered")
        assert np.array_equal(out.bound, 3 * 128 + a.bound)
    z, Z = encrypt_both(H, oracle, world, U8, np.zeros(5, np.uint8), 52, zero_masks=True)
    out = check_shift(H, ctx, "rotl", a, A, FIVE, z, Z, np.zeros(5, np.uint8), what="amount 0")
    assert_equals_model(out, A, "amount 0: a itself")
    c, C = encrypt_both(H, oracle, world, U8, FIVE, 53, zero_masks=True)
    for op, signed in sm.MODES:
        check_shift(H, ctx, op, c, C, FIVE, s, S, FIVE_S, signed=signed, what=f"trivial a {op}")


@gpu
@pytest.mark.parametrize("op,signed", sm.MODES)
def test_equals_the_composition_of_selects(H, world, five, op, signed):
    """Stage by stage with the existing select kernel, y = select(s_t, moved x, x): the same
    ciphertexts limb for limb.  The operands are permuted on the host; the condition is a
    Ciphered<bool> whose bit 0 is s_t."""
    ctx, _ = world(U8)
    (a, A), (s, S) = five
    fused = ctx.shift(marker(H, op), a, s, signed=signed)
    n = a.n
    x, X = a, A  # the running value: device batch and its polynomials
    for t in range(3):
        cond = H.Ciphered.from_host(*sm.pack([[S[e][t]] + [0] * 7 for e in range(n)], s.bound),
                                    s.bound, n, ctx.device, np.dtype(np.bool_))
        src = [sm.source(op, 8, 1 << t, i, signed) for i in range(8)]
        moved = [[X[e][j] if j is not None else 0 for j in src] for e in range(n)]
        m = H.Ciphered.from_host(*sm.pack(moved, x.bound), x.bound, n, ctx.device, a.plain_dtype)
        x = ctx.select(cond, m, x)
        gl, gd = x.to_host()
        X = [bit_ints(gl, gd, x.bound, e) for e in range(n)]
    assert np.array_equal(x.bound, fused.bound)
    fl, fd = fused.to_host()
    xl, xd = x.to_host()
    assert_batches_equal(fl, fd, xl, xd, fused.bound, n, f"{op}: fused against selects")
    ctx.synchronize()


@gpu
def test_single_value_and_empty_batch(H, oracle, world):
    ctx, _ = world(U8)
    av, sv = plain(1, np.uint8, 61), np.array([5], np.uint8)
    a, A = encrypt_both(H, oracle, world, U8, av, 62)
    s, S = encrypt_both(H, oracle, world, U8, sv, 63)
    check_shift(H, ctx, "shl", a, A, av, s, S, sv, what="n=1")
    e = H.Ciphered.empty(0, a.bound, ctx.device, np.dtype(np.uint8))
    out = ctx.shift(H.HomomorphicRotateRight, e, e)
    assert out.n == 0 and out.nbits == 8
    ctx.synchronize()


@gpu
def test_graph_replay_equals_direct_call(H, world, five):
    """Replays into buffers prefilled with -1: every limb and degree word is written."""
    import torch
    ctx, _ = world(U8)
    (a, _), (s, _) = five
    for op in (H.HomomorphicShiftRight, H.HomomorphicRotateLeft):
        direct = ctx.shift(op, a, s)
        got = H.Ciphered.empty(5, direct.bound, ctx.device, np.dtype(np.uint8))
        g = ctx.graph(lambda: H.shift_into(ctx, op, a, s, got))
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
    from homomorph import _lib
    ctx, _ = world(U8)
    (a, _), (s, S) = five

    def call(which, a, s, out, signed=0):
        ca, cs, co = a._c(), s._c(), out._c()
        return _lib.lib().hm_shift_batch(ctx._h, which, ctypes.byref(ca), ctypes.byref(cs), signed,
                                         ctypes.byref(co))

    need = H.shift_out_bounds(H.HomomorphicShiftLeft, a.bound, s.bound)
    out = H.Ciphered.empty(5, need, ctx.device)
    assert call(_lib.OP_SHL, a, s, out) == _lib.OK
    # a 24-bit a
    b24 = np.full(24, 128, np.uint32)
    a24 = H.Ciphered.empty(5, b24, ctx.device)
    o24 = H.Ciphered.empty(5, np.full(24, 4096, np.uint32), ctx.device)
    assert call(_lib.OP_SHL, a24, s, o24) == _lib.ERR_INVALID_ARGUMENT
    # an amount with fewer than L bits
    s2 = H.Ciphered.empty(5, s.bound[:2], ctx.device)
    assert call(_lib.OP_SHL, a, s2, out) == _lib.ERR_INVALID_ARGUMENT
    # ... exactly L bits are enough, and give what the low bits of the byte give
    s3 = H.Ciphered.from_host(*sm.pack([v[:3] for v in S], s.bound[:3]), s.bound[:3], 5, ctx.device)
    out3 = H.Ciphered.empty(5, need, ctx.device)
    assert call(_lib.OP_SHL, a, s3, out3) == _lib.OK
    ctx.synchronize()  # (raw calls are not ordered with torch's stream)
    assert_batches_equal(*out3.to_host(), *out.to_host(), need, 5, "a 3-bit amount")
    # mismatched n, in the amount and in the output; a mismatched width of the output
    assert call(_lib.OP_SHL, a, H.Ciphered.empty(4, s.bound, ctx.device), out) == _lib.ERR_INVALID_ARGUMENT
    assert call(_lib.OP_SHL, a, s, H.Ciphered.empty(4, need, ctx.device)) == _lib.ERR_INVALID_ARGUMENT
    wide = H.Ciphered.empty(5, np.full(16, 1024, np.uint32), ctx.device)
    assert call(_lib.OP_SHL, a, s, wide) == _lib.ERR_INVALID_ARGUMENT
    # short output bounds, in bit 0 and in the top bit; larger ones are accepted
    for k in (0, 7):
        low = need.copy()
        low[k] -= 1
        assert call(_lib.OP_SHL, a, s, H.Ciphered.empty(5, low, ctx.device)) == _lib.ERR_INVALID_ARGUMENT
    assert call(_lib.OP_SHL, a, s, H.Ciphered.empty(5, need + 70, ctx.device)) == _lib.OK
    # the output may not overlap a or the amount: their limbs, or their degree words alone
    other = H.Ciphered.empty(5, need, ctx.device)
    for x in (a, s):
        assert call(_lib.OP_SHL, a, s, H.Ciphered(x.limbs, other.degree, need, 8, 5)) \
            == _lib.ERR_INVALID_ARGUMENT
        assert call(_lib.OP_SHL, a, s, H.Ciphered(other.limbs, x.degree, need, 8, 5)) \
            == _lib.ERR_INVALID_ARGUMENT
    assert call(_lib.OP_SHL, a, s, other) == _lib.OK
    # which outside the four
    for which in (_lib.OP_SELECT, _lib.OP_LOOKUP, 22):
        assert call(which, a, s, out) == _lib.ERR_INVALID_ARGUMENT
    # null batches
    ca, co = a._c(), out._c()
    assert _lib.lib().hm_shift_batch(ctx._h, _lib.OP_SHL, ctypes.byref(ca), None, 0,
                                     ctypes.byref(co)) == _lib.ERR_INVALID_ARGUMENT
    # the Python layer
    with pytest.raises(ValueError):
        ctx.shift(H.HomomorphicSelect, a, s)
    with pytest.raises((ValueError, H.EngineError)):
        ctx.shift(H.HomomorphicShiftLeft, a24, s)
    ctx.synchronize()


@gpu
def test_requirement_is_2_log2_n_plus_3(H):
    """A u8 shift needs d >= 9 delta: (8,8,1,8) fails with required 9, (9,8,1,8) passes and
    decrypts (its model is checked in test_shift_host.py)."""
    from homomorph import _lib
    av = np.array([0x80, 0xFF, 0x5A, 77], np.uint8)
    sv = np.array([0, 7, 9, 3], np.uint8)
    for d, ok in ((8, False), (9, True)):
        ctx = H.Context(H.Parameters(d, 8, 1, 8))
        ctx.seed_rng(5)
        ctx.generate_secret_key()
        ctx.generate_public_key()
        a, s = ctx.encrypt(av), ctx.encrypt(sv)
        if ok:
            for op, signed in sm.MODES:
                got = ctx.decrypt(ctx.shift(marker(H, op), a, s, signed=signed))
                assert np.array_equal(got, sm.numpy_shift(op, av, sv, signed)), op
            ctx.synchronize()
            continue
        with pytest.raises(H.OperationError) as ei:
            ctx.shift(H.HomomorphicShiftLeft, a, s)
        assert ei.value.required_min_d_over_delta == 9
        assert (ei.value.actual_d, ei.value.actual_delta) == (8, 1)
        out = H.Ciphered.empty(4, H.shift_out_bounds(H.HomomorphicShiftLeft, a.bound, s.bound),
                               ctx.device)
        with pytest.raises(H.EngineError) as ei:
            H.shift_into(ctx, H.HomomorphicShiftLeft, a, s, out)
        assert ei.value.status == _lib.ERR_INVALID_PARAMETERS
        ctx.synchronize()


@gpu
def test_validate_entries(H):
    from homomorph import _lib
    L = _lib.lib()
    ctx = H.Context(H.Parameters(300, 64, 1, 8))  # no keys: validation needs none
    req = ctypes.c_uint16()
    for which in (_lib.OP_SHL, _lib.OP_SHR, _lib.OP_ROTL, _lib.OP_ROTR):
        assert L.hm_validate_operation(ctx._h, which, ctypes.byref(req)) == _lib.ERR_INVALID_ARGUMENT
        for nbits, want in ((2, 5), (8, 9), (16, 11), (32, 13), (64, 15), (128, 17)):
            assert L.hm_validate_operation_bits(ctx._h, which, nbits, ctypes.byref(req)) == _lib.OK
            assert req.value == want
        for nbits in (0, 1, 24, 129, 256):
            assert (L.hm_validate_operation_bits(ctx._h, which, nbits, None)
                    == _lib.ERR_INVALID_ARGUMENT)
    ctx.validate_operation(H.HomomorphicShiftLeft, 32)
    with pytest.raises(ValueError):
        ctx.validate_operation(H.HomomorphicShiftLeft)
    tight = H.Context(H.Parameters(12, 8, 1, 8))
    with pytest.raises(H.OperationError) as ei:
        tight.validate_operation(H.HomomorphicRotateRight, 32)
    assert ei.value.required_min_d_over_delta == 13
    tight.validate_operation(H.HomomorphicRotateRight, 16)


@gpu
def test_corrupted_degree_words(H, oracle, world):
    """A corrupted degree word in a bit of a, or in an amount bit below L, is flagged at
    synchronise; the same corruption in an amount bit at or above L is not looked at."""
    from homomorph import _lib
    ctx, _ = world(U16)
    av, sv = plain(4, np.uint16, 71), plain(4, np.uint16, 72)
    a, _ = encrypt_both(H, oracle, world, U16, av, 73)
    s, _ = encrypt_both(H, oracle, world, U16, sv, 74)
    ctx.synchronize()
    op = H.HomomorphicRotateLeft
    s.degree[2, 4] += 1  # not read: L = 4
    s.degree[1, 15] += 1
    assert np.array_equal(ctx.decrypt(ctx.shift(op, a, s)), sm.numpy_shift("rotl", av, sv))
    ctx.synchronize()
    s.degree[2, 3] += 1  # the limbs have no coefficient there (or it is past the bound)
    ctx.shift(op, a, s)
    with pytest.raises(H.EngineError) as ei:
        ctx.synchronize()
    assert ei.value.status == _lib.ERR_BAD_INPUT
    s.degree[2, 3] -= 1
    ctx.shift(op, a, s)
    ctx.synchronize()  # clean: the flag was cleared by the check
    a.degree[3, 9] += 1
    ctx.shift(op, a, s)
    with pytest.raises(H.EngineError) as ei:
        ctx.synchronize()
    assert ei.value.status == _lib.ERR_BAD_INPUT


@gpu
def test_lds_limit_is_refused_before_any_launch(H, world):
    """A u32 at bound 20 000 per bit: 32 slots of 3 752 words per wave."""
    from homomorph import _lib
    ctx, _ = world(U8)
    big = H.Ciphered.empty(1, np.full(32, 20000, np.uint32), ctx.device, np.dtype(np.uint32))
    amount = H.Ciphered.empty(1, np.full(8, 20000, np.uint32), ctx.device, np.dtype(np.uint8))
    with pytest.raises(H.EngineError) as ei:
        ctx.shift(H.HomomorphicShiftLeft, big, amount)
    assert ei.value.status == _lib.ERR_UNSUPPORTED
    ctx.synchronize()
