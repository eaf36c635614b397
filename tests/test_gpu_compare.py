"""GPU: homomorphic subtraction and comparisons (hm_sub_batch, hm_compare_batch) against the model
circuits (tests/borrow_model.py over oracle/gf2_model.py), bit-exact.

Both sides get identical seeded keys, masks and plaintexts (the pattern of smoke()); every case
runs the subtraction and all six comparisons, unsigned and signed, and checks the limbs and the
degree words against the model, the decrypted results against numpy, and a clean
ctx.synchronize().  Shapes are the smallest that reach each path of the kernel.
"""
import numpy as np
import pytest

import borrow_model as bm
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


def op_class(H, op):
    return {"eq": H.HomomorphicEqual, "ne": H.HomomorphicNotEqual, "lt": H.HomomorphicLessThan,
            "le": H.HomomorphicLessEqual, "gt": H.HomomorphicGreaterThan,
            "ge": H.HomomorphicGreaterEqual}[op]


def edge_pairs(udt):
    """The seven value pairs of the issue, as bit patterns of the unsigned dtype: equal, off by
    one, differing only in bit 0, only in the top bit, 0 against max, signed min against signed
    max, -1 against 0."""
    info = np.iinfo(udt)
    top = 1 << (info.bits - 1)
    v = int(plain(1, udt, 99, 2, info.max - 2)[0]) & ~1
    rows = [(v, v), (v | 1, (v | 1) + 1), (v, v | 1), (v & ~top, v | top), (0, info.max),
            (top, top - 1), (info.max, 0)]
    return np.array([r[0] for r in rows], udt), np.array([r[1] for r in rows], udt)


def check_all(H, world, params, a, A, av, b, B, bv, what):
    """Subtraction and the six comparisons, unsigned and signed, of device batches a, b (model
    polynomials A, B; plaintexts av, bv as the unsigned dtype)."""
    ctx, _ = world(params)
    n, udt = a.n, av.dtype
    sdt = SIGNED[udt]
    out = ctx.apply2(H.HomomorphicSubtraction, a, b)
    assert np.array_equal(out.bound, bm.sub_bounds(a.bound, b.bound))
    el, ed = bm.pack([bm.sub_circuit(A[e], B[e]) for e in range(n)], out.bound)
    gl, gd = out.to_host()
    assert_batches_equal(gl, gd, el, ed, out.bound, n, f"{what} sub")
    with np.errstate(over="ignore"):
        want = (av - bv).astype(udt)
    assert np.array_equal(ctx.decrypt(out, udt), want)
    assert np.array_equal(ctx.decrypt(out, sdt), want.view(sdt))
    for signed, dt in ((False, udt), (True, sdt)):
        for op in bm.COMPARISONS:
            r = ctx.apply2(op_class(H, op), a, b, signed=signed)
            assert r.nbits == 8 and r.n == n
            assert np.array_equal(r.bound, bm.compare_bounds(op, a.bound, b.bound))
            el, ed = bm.pack([bm.bool_value(bm.compare_circuit(op, A[e], B[e], signed))
                              for e in range(n)], r.bound)
            gl, gd = r.to_host()
            assert_batches_equal(gl, gd, el, ed, r.bound, n, f"{what} {op} signed={signed}")
            dec = ctx.decrypt(r)
            assert dec.dtype == np.bool_
            assert np.array_equal(dec, bm.NUMPY_OPS[op](av.view(dt), bv.view(dt))), (op, signed)
    ctx.synchronize()


def test_u8_every_edge_pair(H, oracle, world):
    """(64,64,1,64): one-word-per-lane tiles only; all seven edge pairs and one random pair."""
    ea, eb = edge_pairs(np.uint8)
    av = np.concatenate([ea, plain(1, np.uint8, 1)])
    bv = np.concatenate([eb, plain(1, np.uint8, 2)])
    a, A = encrypt_both(H, oracle, world, U8, av, 11)
    b, B = encrypt_both(H, oracle, world, U8, bv, 12)
    check_all(H, world, U8, a, A, av, b, B, bv, "u8")


def test_u32_five_values(H, oracle, world):
    """The headline parameters: n = 5 is no multiple of the 4 waves per block, and the borrow's
    tile width steps up to 5 words per lane."""
    ea, eb = edge_pairs(np.uint32)
    pick = [0, 1, 3, 5]  # equal, off by one, top bit only, signed min against max
    av = np.concatenate([ea[pick], plain(1, np.uint32, 1)])
    bv = np.concatenate([eb[pick], plain(1, np.uint32, 2)])
    a, A = encrypt_both(H, oracle, world, U32, av, 21)
    b, B = encrypt_both(H, oracle, world, U32, bv, 22)
    check_all(H, world, U32, a, A, av, b, B, bv, "u32")


def test_u64_two_values(H, oracle, world):
    """(256,64,1,64): p_i is 11 words (two kQSmall chunks) and the borrow reaches 651 words (more
    than one 512-word tile)."""
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
    """Both operands the same batch: x_i = 0, so == is exactly the unit polynomial, degree 0."""
    av = plain(3, np.uint8, 5)
    a, A = encrypt_both(H, oracle, world, U8, av, 51)
    check_all(H, world, U8, a, A, av, a, A, av, "same")
    ctx, _ = world(U8)
    r = ctx.apply2(H.HomomorphicEqual, a, a)
    l, d = r.to_host()
    stride = H.batch_stride(r.bound)
    l = l.reshape(3, stride)
    assert not d.any() and np.all(l[:, 0] == 1) and not l[:, 1:].any()


@pytest.mark.parametrize("which", ["a", "b", "both"])
def test_trivial_ciphertexts(H, oracle, world, which):
    """All-zero masks: every bit is the null or the unit polynomial, so p_i and the borrow may be
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


def test_signedness_defaults_from_the_plaintext_dtype(H, world):
    """apply2 takes `signed` from the operand's plaintext dtype, as for multiplication, and a
    difference keeps that dtype."""
    ctx, _ = world(U8)
    av, bv = np.array([-1, 5, -128, 7], np.int8), np.array([0, -3, 127, 7], np.int8)
    for dt in (np.int8, np.uint8):
        x, y = av.view(dt), bv.view(dt)
        a, b = ctx.encrypt(x), ctx.encrypt(y)
        for op in bm.COMPARISONS:
            got = ctx.decrypt(ctx.apply2(op_class(H, op), a, b))
            assert np.array_equal(got, bm.NUMPY_OPS[op](x, y)), (op, dt)
        diff = ctx.decrypt(ctx.apply2(H.HomomorphicSubtraction, a, b))
        with np.errstate(over="ignore"):
            assert diff.dtype == dt and np.array_equal(diff, (x - y).astype(dt))
    ctx.synchronize()


def test_graph_replay_equals_direct_call(H, oracle, world):
    ctx, _ = world(U8)
    av, bv = plain(6, np.uint8, 81), plain(6, np.uint8, 82)
    a, _ = encrypt_both(H, oracle, world, U8, av, 83)
    b, _ = encrypt_both(H, oracle, world, U8, bv, 84)
    ds = ctx.apply2(H.HomomorphicSubtraction, a, b)
    dc = ctx.apply2(H.HomomorphicLessEqual, a, b, signed=True)
    gs = H.Ciphered.empty(6, ds.bound, ctx.device, np.dtype(np.uint8))
    gc = H.Ciphered.empty(6, dc.bound, ctx.device, np.dtype(np.bool_))

    def step():
        H.sub_into(ctx, a, b, gs)
        H.compare_into(ctx, H.HomomorphicLessEqual, a, b, gc, signed=True)
    g = ctx.graph(step)
    for t in (gs, gc):
        t.limbs.fill_(-1)
        t.degree.fill_(-1)
    import torch
    torch.cuda.synchronize()  # the fills ran on torch's stream, the replay runs on the engine's
    g.replay()
    ctx.synchronize()
    for got, want in ((gs, ds), (gc, dc)):
        gl, gd = got.to_host()
        wl, wd = want.to_host()
        assert_batches_equal(gl, gd, wl, wd, want.bound, 6, "graph replay")
    assert np.array_equal(ctx.decrypt(gc), av.view(np.int8) <= bv.view(np.int8))


def test_argument_errors(H, oracle, world):
    ctx, _ = world(U8)
    from homomorph import _lib
    av = plain(4, np.uint8, 91)
    a, _ = encrypt_both(H, oracle, world, U8, av, 92)
    b, _ = encrypt_both(H, oracle, world, U8, av, 93)
    short, _ = encrypt_both(H, oracle, world, U8, av[:3], 94)
    LT = H.HomomorphicLessThan
    need = H.compare_out_bounds(LT, a.bound, b.bound)

    def status(fn):
        with pytest.raises(H.EngineError) as ei:
            fn()
        return ei.value.status

    # a comparison's output has 8 bits, whatever the inputs' width
    wide = H.Ciphered.empty(4, np.concatenate([need, [0]]), ctx.device)
    assert status(lambda: H.compare_into(ctx, LT, a, b, wide)) == _lib.ERR_INVALID_ARGUMENT
    # short output bounds
    low = need.copy()
    low[0] -= 1
    out = H.Ciphered.empty(4, low, ctx.device)
    assert status(lambda: H.compare_into(ctx, LT, a, b, out)) == _lib.ERR_INVALID_ARGUMENT
    sb = H.sub_out_bounds(a.bound, b.bound)
    low = sb.copy()
    low[7] -= 1
    out = H.Ciphered.empty(4, low, ctx.device)
    assert status(lambda: H.sub_into(ctx, a, b, out)) == _lib.ERR_INVALID_ARGUMENT
    # mismatched n
    out = H.Ciphered.empty(4, need, ctx.device)
    assert status(lambda: H.compare_into(ctx, LT, a, short, out)) == _lib.ERR_INVALID_ARGUMENT
    out = H.Ciphered.empty(4, sb, ctx.device)
    assert status(lambda: H.sub_into(ctx, a, short, out)) == _lib.ERR_INVALID_ARGUMENT
    ctx.synchronize()


def test_requirement_depends_on_width(H):
    """u8 <: m = 9, so d >= 19 delta: (56,64,3,64) fails with required 19, (57,64,3,64) passes."""
    av = np.array([3, 200], np.uint8)
    bv = np.array([7, 100], np.uint8)
    for d, ok in ((56, False), (57, True)):
        ctx = H.Context(H.Parameters(d, 64, 3, 64))
        ctx.seed_rng(5)
        ctx.generate_secret_key()
        ctx.generate_public_key()
        a, b = ctx.encrypt(av), ctx.encrypt(bv)
        if ok:
            r = ctx.apply2(H.HomomorphicLessThan, a, b)
            assert np.array_equal(ctx.decrypt(r), av < bv)
            ctx.synchronize()
        else:
            with pytest.raises(H.OperationError) as ei:
                ctx.apply2(H.HomomorphicLessThan, a, b)
            assert ei.value.required_min_d_over_delta == 19
            assert (ei.value.actual_d, ei.value.actual_delta) == (56, 3)


def test_validate_entries_empty_batch_and_lds_limit(H):
    from homomorph import _lib
    import ctypes
    L = _lib.lib()
    ctx = H.Context(H.Parameters(300, 64, 1, 8))  # no keys: the operations need none
    req = ctypes.c_uint16()
    # hm_validate_operation has no width: the new codes are invalid arguments there ...
    for code in range(_lib.OP_SUB, _lib.OP_GE + 1):
        assert L.hm_validate_operation(ctx._h, code, ctypes.byref(req)) == _lib.ERR_INVALID_ARGUMENT
    # ... and hm_validate_operation_bits is hm_validate_operation for the old ones
    for code in range(_lib.OP_AND, _lib.OP_MUL_SIGNED + 1):
        r2 = ctypes.c_uint16()
        assert (L.hm_validate_operation_bits(ctx._h, code, 32, ctypes.byref(r2))
                == L.hm_validate_operation(ctx._h, code, ctypes.byref(req)))
        assert r2.value == req.value
    assert L.hm_validate_operation_bits(ctx._h, _lib.OP_LT, 32, ctypes.byref(req)) == _lib.OK
    assert req.value == 67
    assert L.hm_validate_operation_bits(ctx._h, _lib.OP_SUB, 32, ctypes.byref(req)) == _lib.OK
    assert req.value == 65
    for nbits in (0, 129):
        assert (L.hm_validate_operation_bits(ctx._h, _lib.OP_EQ, nbits, None)
                == _lib.ERR_INVALID_ARGUMENT)
    ctx.validate_operation(H.HomomorphicGreaterEqual, 64)
    with pytest.raises(ValueError):
        ctx.validate_operation(H.HomomorphicGreaterEqual)
    # n = 0 is fine and launches nothing
    b32 = np.full(32, 364, np.uint32)
    e = H.Ciphered.empty(0, b32, ctx.device, np.dtype(np.uint32))
    assert ctx.apply2(H.HomomorphicSubtraction, e, e).n == 0
    assert ctx.apply2(H.HomomorphicLessThan, e, e).n == 0
    # a chain that does not fit a wave's share of LDS is refused before any launch: u128 at
    # bound 2000 needs two borrow buffers of 129 * 2000 / 32 words each
    big = H.Ciphered.empty(1, np.full(128, 2000, np.uint32), ctx.device, None)
    for op in (H.HomomorphicSubtraction, H.HomomorphicLessThan, H.HomomorphicEqual):
        with pytest.raises(H.EngineError) as ei:
            ctx.apply2(op, big, big, signed=False)
        assert ei.value.status == _lib.ERR_UNSUPPORTED
    ctx.synchronize()


def test_corrupted_degree_word_is_flagged(H, oracle, world):
    from homomorph import _lib
    ctx, _ = world(U8)
    av = plain(4, np.uint8, 95)
    a, _ = encrypt_both(H, oracle, world, U8, av, 96)
    b, _ = encrypt_both(H, oracle, world, U8, av, 97)
    ctx.synchronize()
    a.degree[2, 5] += 1  # the limbs have no coefficient there (or it is past the bound)
    for fn in (lambda: ctx.apply2(H.HomomorphicSubtraction, a, b),
               lambda: ctx.apply2(H.HomomorphicGreaterEqual, b, a)):
        fn()
        with pytest.raises(H.EngineError) as ei:
            ctx.synchronize()
        assert ei.value.status == _lib.ERR_BAD_INPUT
    ctx.synchronize()  # the flag is cleared by the check
