"""GPU: homomorphic select, min and max (hm_select_batch, hm_minmax_batch) against the model
circuits (tests/select_model.py over tests/borrow_model.py and oracle/gf2_model.py), bit-exact.

The pattern and the parameter sets of tests/test_gpu_compare.py: both sides get identical seeded
keys, masks and plaintexts; every case checks the limbs and the degree words against the model,
the decrypted results against numpy, and a clean ctx.synchronize().  Shapes are the smallest that
reach each path of the kernels.
"""
import ctypes

import numpy as np
import pytest

import borrow_model as bm
import select_model as sm
from circuit_gpu import encrypt_both, load_engine, make_world
from helpers import assert_batches_equal, plain

pytestmark = pytest.mark.gpu

U8, U16, U32, U64 = (64, 64, 1, 64), (64, 32, 1, 32), (128, 128, 1, 128), (256, 64, 1, 64)
SIGNED = {np.dtype(np.uint8): np.int8, np.dtype(np.uint16): np.int16,
          np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
SEED = 2025


@pytest.fixture(scope="module")
def H():
    return load_engine()


@pytest.fixture(scope="module")
def world(H, oracle):
    return make_world(H, SEED)


def edge_pairs(udt):
    """Seven value pairs as bit patterns of the unsigned dtype: equal, off by one, differing only
    in bit 0, only in the top bit, 0 against max, signed min against signed max, -1 against 0."""
    info = np.iinfo(udt)
    top = 1 << (info.bits - 1)
    v = int(plain(1, udt, 99, 2, info.max - 2)[0]) & ~1
    rows = [(v, v), (v | 1, (v | 1) + 1), (v, v | 1), (v & ~top, v | top), (0, info.max),
            (top, top - 1), (info.max, 0)]
    return np.array([r[0] for r in rows], udt), np.array([r[1] for r in rows], udt)


def assert_equals_model(out, values, what):
    """The device batch against the model's bit polynomials per value, limbs and degree words."""
    el, ed = bm.pack(values, out.bound)
    gl, gd = out.to_host()
    assert_batches_equal(gl, gd, el, ed, out.bound, out.n, what)


def check_select(H, ctx, c, C, cv, a, A, av, b, B, bv, what):
    """select(c, a, b) of device batches (model polynomials C = the condition's bit 0 per value;
    plaintexts cv, av, bv)."""
    out = ctx.select(c, a, b)
    assert out.nbits == a.nbits and out.n == a.n and out.plain_dtype == a.plain_dtype
    assert np.array_equal(out.bound, sm.select_bounds(c.bound[0], a.bound, b.bound))
    assert_equals_model(out, [sm.select_circuit(C[e], A[e], B[e]) for e in range(a.n)], what)
    assert np.array_equal(ctx.decrypt(out, av.dtype), np.where(cv, av, bv)), what
    return out


def check_all(H, world, params, a, A, av, b, B, bv, what):
    """min and max, unsigned and signed, and the select of a < b, of device batches a, b (model
    polynomials A, B; plaintexts av, bv as the unsigned dtype)."""
    ctx, _ = world(params)
    n, udt = a.n, av.dtype
    sdt = SIGNED[udt]
    for signed, dt in ((False, udt), (True, sdt)):
        x, y = av.view(dt), bv.view(dt)
        for op, circuit, ref in ((H.HomomorphicMin, sm.min_circuit, np.minimum),
                                 (H.HomomorphicMax, sm.max_circuit, np.maximum)):
            tag = f"{what} {op.__name__} signed={signed}"
            out = ctx.apply2(op, a, b, signed=signed)
            assert out.nbits == a.nbits and out.n == n
            assert np.array_equal(out.bound, sm.minmax_bounds(a.bound, b.bound))
            assert_equals_model(out, [circuit(A[e], B[e], signed) for e in range(n)], tag)
            assert np.array_equal(ctx.decrypt(out, dt), ref(x, y)), tag
    lt = ctx.apply2(H.HomomorphicLessThan, a, b, signed=False)
    LT = [sm.less_than(A[e], B[e]) for e in range(n)]
    check_select(H, ctx, lt, LT, av < bv, a, A, av, b, B, bv, f"{what} select(lt)")
    ctx.synchronize()


def test_u8_every_edge_pair(H, oracle, world):
    """(64,64,1,64): one-word-per-lane tiles only; all seven edge pairs and one random pair, and
    the select under a comparison's, a fresh and the two trivial conditions."""
    ctx, _ = world(U8)
    ea, eb = edge_pairs(np.uint8)
    av = np.concatenate([ea, plain(1, np.uint8, 1)])
    bv = np.concatenate([eb, plain(1, np.uint8, 2)])
    a, A = encrypt_both(H, oracle, world, U8, av, 11)
    b, B = encrypt_both(H, oracle, world, U8, bv, 12)
    check_all(H, world, U8, a, A, av, b, B, bv, "u8")
    cv = np.array([1, 0, 0, 1, 1, 0, 1, 0], np.uint8)
    c, C = encrypt_both(H, oracle, world, U8, cv, 13)
    assert c.nbits == 8
    check_select(H, ctx, c, [v[0] for v in C], cv.astype(bool), a, A, av, b, B, bv, "u8 fresh c")
    # zero-mask conditions are the null and the unit polynomial: b's or a's bits themselves
    z, Z = encrypt_both(H, oracle, world, U8, cv, 14, zero_masks=True)
    assert [v[0] for v in Z] == cv.tolist()
    out = check_select(H, ctx, z, [v[0] for v in Z], cv.astype(bool), a, A, av, b, B, bv,
                       "u8 trivial c")
    assert_equals_model(out, [A[e] if cv[e] else B[e] for e in range(8)], "u8 trivial c: operand")
    ctx.synchronize()


def test_u32_five_values(H, oracle, world):
    """The headline parameters: n = 5 is no multiple of the 4 waves per block, and the product
    w_n x_i is 5 words per lane."""
    ea, eb = edge_pairs(np.uint32)
    pick = [0, 1, 3, 5]  # equal, off by one, top bit only, signed min against max
    av = np.concatenate([ea[pick], plain(1, np.uint32, 1)])
    bv = np.concatenate([eb[pick], plain(1, np.uint32, 2)])
    a, A = encrypt_both(H, oracle, world, U32, av, 21)
    b, B = encrypt_both(H, oracle, world, U32, bv, 22)
    check_all(H, world, U32, a, A, av, b, B, bv, "u32")


def test_u64_two_values(H, oracle, world):
    """(256,64,1,64): x_i is 11 words (two kQSmall chunks) and w_n reaches 651 words, so the
    phase-2 product needs more than one 512-word tile."""
    ea, eb = edge_pairs(np.uint64)
    av = np.array([ea[4], plain(1, np.uint64, 1)[0]], np.uint64)  # 0 against max, random
    bv = np.array([eb[4], plain(1, np.uint64, 2)[0]], np.uint64)
    a, A = encrypt_both(H, oracle, world, U64, av, 31)
    b, B = encrypt_both(H, oracle, world, U64, bv, 32)
    check_all(H, world, U64, a, A, av, b, B, bv, "u64")


def test_u16_skewed_bounds(H, oracle, world):
    """Per-bit input bounds fresh + 37 i on one side: capacities, offsets and output bounds differ
    bit by bit."""
    ea, eb = edge_pairs(np.uint16)
    pick = [2, 6, 1]  # bit 0 only, -1 against 0, off by one
    av = np.concatenate([ea[pick], plain(1, np.uint16, 1)])
    bv = np.concatenate([eb[pick], plain(1, np.uint16, 2)])
    skew = (U16[0] + U16[1] + 37 * np.arange(16)).astype(np.uint32)
    a, A = encrypt_both(H, oracle, world, U16, av, 41, bound=skew)
    b, B = encrypt_both(H, oracle, world, U16, bv, 42)
    check_all(H, world, U16, a, A, av, b, B, bv, "u16 skew a")
    check_all(H, world, U16, b, B, bv, a, A, av, "u16 skew b")


def test_same_batch_object(H, oracle, world):
    """Both operands the same batch: x_i = 0, so every output bit equals the input bit."""
    ctx, _ = world(U8)
    av = plain(3, np.uint8, 5)
    a, A = encrypt_both(H, oracle, world, U8, av, 51)
    check_all(H, world, U8, a, A, av, a, A, av, "same")
    lt = ctx.apply2(H.HomomorphicLessThan, a, a)
    for out in (ctx.apply2(H.HomomorphicMin, a, a), ctx.apply2(H.HomomorphicMax, a, a, signed=True),
                ctx.select(lt, a, a)):
        assert_equals_model(out, A, "same: the operand")
    ctx.synchronize()


@pytest.mark.parametrize("which", ["a", "b", "both"])
def test_trivial_ciphertexts(H, oracle, world, which):
    """All-zero masks: every bit is the null or the unit polynomial, so x_i and the borrow may be
    null."""
    ea, eb = edge_pairs(np.uint8)
    av, bv = ea[[0, 1, 4, 6]], eb[[0, 1, 4, 6]]
    a, A = encrypt_both(H, oracle, world, U8, av, 61, zero_masks=which in ("a", "both"))
    b, B = encrypt_both(H, oracle, world, U8, bv, 62, zero_masks=which in ("b", "both"))
    check_all(H, world, U8, a, A, av, b, B, bv, f"trivial {which}")


def test_single_value(H, oracle, world):
    av, bv = plain(1, np.uint16, 71), plain(1, np.uint16, 72)
    a, A = encrypt_both(H, oracle, world, U16, av, 73)
    b, B = encrypt_both(H, oracle, world, U16, bv, 74)
    check_all(H, world, U16, a, A, av, b, B, bv, "n=1")


def test_fused_equals_composed(H, oracle, world):
    """min(a, b) is select(a < b, a, b) and max(a, b) is select(a < b, b, a), bit for bit, and
    apply_n routes the select."""
    ctx, _ = world(U8)
    ea, eb = edge_pairs(np.uint8)
    a, _ = encrypt_both(H, oracle, world, U8, ea, 75)
    b, _ = encrypt_both(H, oracle, world, U8, eb, 76)
    for signed in (False, True):
        lt = ctx.apply2(H.HomomorphicLessThan, a, b, signed=signed)
        for op, args in ((H.HomomorphicMin, [lt, a, b]), (H.HomomorphicMax, [lt, b, a])):
            fused = ctx.apply2(op, a, b, signed=signed)
            composed = ctx.apply_n(H.HomomorphicSelect, args)
            assert np.array_equal(fused.bound, composed.bound)
            fl, fd = fused.to_host()
            cl, cd = composed.to_host()
            assert_batches_equal(fl, fd, cl, cd, fused.bound, 7, f"{op.__name__} signed={signed}")
    ctx.synchronize()


def test_signedness_defaults_from_the_plaintext_dtype(H, world):
    """apply2 takes `signed` from the operand's plaintext dtype, as for comparisons, and the
    result keeps that dtype."""
    ctx, _ = world(U8)
    av, bv = np.array([-1, 5, -128, 7], np.int8), np.array([0, -3, 127, 7], np.int8)
    for dt in (np.int8, np.uint8):
        x, y = av.view(dt), bv.view(dt)
        a, b = ctx.encrypt(x), ctx.encrypt(y)
        for op, ref in ((H.HomomorphicMin, np.minimum), (H.HomomorphicMax, np.maximum)):
            got = ctx.decrypt(ctx.apply2(op, a, b))
            assert got.dtype == dt and np.array_equal(got, ref(x, y)), (op, dt)
        pick = ctx.decrypt(ctx.select(ctx.apply2(H.HomomorphicGreaterEqual, a, b), a, b))
        assert pick.dtype == dt and np.array_equal(pick, np.maximum(x, y))
    ctx.synchronize()


def test_graph_replay_equals_direct_call(H, oracle, world):
    """Replays into buffers prefilled with -1: every limb and degree word is written."""
    ctx, _ = world(U8)
    av, bv = plain(6, np.uint8, 81), plain(6, np.uint8, 82)
    a, _ = encrypt_both(H, oracle, world, U8, av, 83)
    b, _ = encrypt_both(H, oracle, world, U8, bv, 84)
    c = ctx.apply2(H.HomomorphicLessEqual, a, b, signed=True)
    ds = ctx.select(c, a, b)
    dm = ctx.apply2(H.HomomorphicMax, a, b, signed=True)
    gs = H.Ciphered.empty(6, ds.bound, ctx.device, np.dtype(np.uint8))
    gm = H.Ciphered.empty(6, dm.bound, ctx.device, np.dtype(np.uint8))

    def step():
        H.select_into(ctx, c, a, b, gs)
        H.minmax_into(ctx, H.HomomorphicMax, a, b, gm, signed=True)
    g = ctx.graph(step)
    for t in (gs, gm):
        t.limbs.fill_(-1)
        t.degree.fill_(-1)
    import torch
    torch.cuda.synchronize()  # the fills ran on torch's stream, the replay runs on the engine's
    g.replay()
    ctx.synchronize()
    for got, want in ((gs, ds), (gm, dm)):
        gl, gd = got.to_host()
        wl, wd = want.to_host()
        assert_batches_equal(gl, gd, wl, wd, want.bound, 6, "graph replay")
    x, y = av.view(np.int8), bv.view(np.int8)
    assert np.array_equal(ctx.decrypt(gs, np.int8), np.where(x <= y, x, y))
    assert np.array_equal(ctx.decrypt(gm, np.int8), np.maximum(x, y))


def test_argument_errors(H, oracle, world):
    ctx, _ = world(U8)
    from homomorph import _lib
    av = plain(4, np.uint8, 91)
    a, _ = encrypt_both(H, oracle, world, U8, av, 92)
    b, _ = encrypt_both(H, oracle, world, U8, av, 93)
    short, _ = encrypt_both(H, oracle, world, U8, av[:3], 94)
    c = ctx.apply2(H.HomomorphicLessThan, a, b)
    sneed = H.select_out_bounds(c.bound[0], a.bound, b.bound)
    mneed = H.minmax_out_bounds(a.bound, b.bound)
    Min = H.HomomorphicMin

    def status(fn):
        with pytest.raises(H.EngineError) as ei:
            fn()
        return ei.value.status

    out = H.Ciphered.empty(4, sneed, ctx.device)
    # the condition is a Ciphered<bool>: 8 bits
    wide = H.Ciphered.empty(4, np.concatenate([c.bound, [0]]), ctx.device)
    assert status(lambda: H.select_into(ctx, wide, a, b, out)) == _lib.ERR_INVALID_ARGUMENT
    # short output bounds
    for k in (0, 7):
        low = sneed.copy()
        low[k] -= 1
        bad = H.Ciphered.empty(4, low, ctx.device)
        assert status(lambda: H.select_into(ctx, c, a, b, bad)) == _lib.ERR_INVALID_ARGUMENT
        low = mneed.copy()
        low[k] -= 1
        bad = H.Ciphered.empty(4, low, ctx.device)
        assert status(lambda: H.minmax_into(ctx, Min, a, b, bad)) == _lib.ERR_INVALID_ARGUMENT
    # mismatched n, in an operand and in the condition
    assert status(lambda: H.select_into(ctx, c, a, short, out)) == _lib.ERR_INVALID_ARGUMENT
    cshort = H.Ciphered.empty(3, c.bound, ctx.device)
    assert status(lambda: H.select_into(ctx, cshort, a, b, out)) == _lib.ERR_INVALID_ARGUMENT
    out = H.Ciphered.empty(4, mneed, ctx.device)
    assert status(lambda: H.minmax_into(ctx, Min, a, short, out)) == _lib.ERR_INVALID_ARGUMENT
    # hm_minmax_batch takes HM_OP_MIN or HM_OP_MAX only
    assert (status(lambda: H.minmax_into(ctx, H.HomomorphicLessThan, a, b, out))
            == _lib.ERR_INVALID_ARGUMENT)
    # the output may not overlap an input
    same = H.Ciphered(a.limbs, a.degree, a.bound, 8, 4)
    wide_a = ctx.encrypt(av, bound=mneed)
    alias = H.Ciphered(wide_a.limbs, wide_a.degree, mneed, 8, 4)
    assert status(lambda: H.minmax_into(ctx, Min, wide_a, b, alias)) == _lib.ERR_INVALID_ARGUMENT
    assert status(lambda: H.minmax_into(ctx, Min, a, b, same)) == _lib.ERR_INVALID_ARGUMENT
    ctx.synchronize()


def test_requirement_depends_on_width(H):
    """u8 min: m = 10, so d >= 21 delta: (62,64,3,64) fails with required 21, (63,64,3,64)
    passes (its model is checked in test_select_host.py)."""
    av = np.array([3, 200], np.uint8)
    bv = np.array([7, 100], np.uint8)
    for d, ok in ((62, False), (63, True)):
        ctx = H.Context(H.Parameters(d, 64, 3, 64))
        ctx.seed_rng(5)
        ctx.generate_secret_key()
        ctx.generate_public_key()
        a, b = ctx.encrypt(av), ctx.encrypt(bv)
        if ok:
            assert np.array_equal(ctx.decrypt(ctx.apply2(H.HomomorphicMin, a, b)),
                                  np.minimum(av, bv))
            assert np.array_equal(ctx.decrypt(ctx.apply2(H.HomomorphicMax, a, b)),
                                  np.maximum(av, bv))
            ctx.synchronize()
        else:
            for op in (H.HomomorphicMin, H.HomomorphicMax):
                with pytest.raises(H.OperationError) as ei:
                    ctx.apply2(op, a, b)
                assert ei.value.required_min_d_over_delta == 21
                assert (ei.value.actual_d, ei.value.actual_delta) == (62, 3)


def test_validate_entries_empty_batch_and_lds_limit(H):
    from homomorph import _lib
    L = _lib.lib()
    ctx = H.Context(H.Parameters(300, 64, 1, 8))  # no keys: the operations need none
    req = ctypes.c_uint16()
    # select has no width: both entries give 5
    assert L.hm_validate_operation(ctx._h, _lib.OP_SELECT, ctypes.byref(req)) == _lib.OK
    assert req.value == 5
    for nbits in (1, 32, 128):
        req = ctypes.c_uint16()
        assert L.hm_validate_operation_bits(ctx._h, _lib.OP_SELECT, nbits, ctypes.byref(req)) == _lib.OK
        assert req.value == 5
    # min and max need one
    for code in (_lib.OP_MIN, _lib.OP_MAX):
        assert L.hm_validate_operation(ctx._h, code, ctypes.byref(req)) == _lib.ERR_INVALID_ARGUMENT
        for nbits, want in ((8, 21), (16, 37), (32, 69), (64, 133), (128, 261)):
            assert L.hm_validate_operation_bits(ctx._h, code, nbits, ctypes.byref(req)) == _lib.OK
            assert req.value == want
        for nbits in (0, 129):
            assert (L.hm_validate_operation_bits(ctx._h, code, nbits, None)
                    == _lib.ERR_INVALID_ARGUMENT)
    ctx.validate_operation(H.HomomorphicMax, 64)
    ctx.validate_operation(H.HomomorphicSelect)
    with pytest.raises(ValueError):
        ctx.validate_operation(H.HomomorphicMax)
    tight = H.Context(H.Parameters(68, 64, 1, 8))
    with pytest.raises(H.OperationError) as ei:
        tight.validate_operation(H.HomomorphicMin, 32)
    assert ei.value.required_min_d_over_delta == 69
    tight.validate_operation(H.HomomorphicLessThan, 32)
    # n = 0 is fine and launches nothing
    b32 = np.full(32, 364, np.uint32)
    e = H.Ciphered.empty(0, b32, ctx.device, np.dtype(np.uint32))
    ce = H.Ciphered.empty(0, np.full(8, 364, np.uint32), ctx.device, np.dtype(np.bool_))
    assert ctx.apply2(H.HomomorphicMin, e, e).n == 0
    assert ctx.apply2(H.HomomorphicMax, e, e).n == 0
    assert ctx.select(ce, e, e).n == 0
    # a value that does not fit a wave's share of LDS is refused before any launch: u128 at bound
    # 2000 has a last borrow of 129 * 2000 / 32 words, twice in either kernel's slice
    big = H.Ciphered.empty(1, np.full(128, 2000, np.uint32), ctx.device, None)
    for op in (H.HomomorphicMin, H.HomomorphicMax):
        with pytest.raises(H.EngineError) as ei:
            ctx.apply2(op, big, big, signed=False)
        assert ei.value.status == _lib.ERR_UNSUPPORTED
    cbig = H.Ciphered.empty(1, H.compare_out_bounds(H.HomomorphicLessThan, big.bound, big.bound),
                            ctx.device, np.dtype(np.bool_))
    with pytest.raises(H.EngineError) as ei:
        ctx.select(cbig, big, big)
    assert ei.value.status == _lib.ERR_UNSUPPORTED
    ctx.synchronize()


def test_corrupted_degree_word_is_flagged(H, oracle, world):
    from homomorph import _lib
    ctx, _ = world(U8)
    av = plain(4, np.uint8, 95)
    a, _ = encrypt_both(H, oracle, world, U8, av, 96)
    b, _ = encrypt_both(H, oracle, world, U8, av, 97)
    c, _ = encrypt_both(H, oracle, world, U8, np.array([1, 0, 1, 0], np.uint8), 98)
    good = ctx.encrypt(av)
    ctx.synchronize()
    c.degree[2, 0] += 1  # the limbs have no coefficient there (or it is past the bound)
    a.degree[2, 5] += 1
    for fn in (lambda: ctx.select(c, good, b), lambda: ctx.select(ctx.encrypt(av), a, b),
               lambda: ctx.apply2(H.HomomorphicMin, a, b),
               lambda: ctx.apply2(H.HomomorphicMax, b, a)):
        fn()
        with pytest.raises(H.EngineError) as ei:
            ctx.synchronize()
        assert ei.value.status == _lib.ERR_BAD_INPUT
    c.degree[2, 1] += 1  # bits 1..7 of the condition are not read
    c.degree[2, 0] -= 1
    ctx.select(c, good, b)
    ctx.synchronize()  # clean: the flag was cleared by the checks
