"""GPU: oblivious array read and write by an encrypted index (hm_array_read_batch,
hm_array_write_batch) against the model circuits (tests/array_model.py over
oracle/gf2_model.py), bit-exact.

The pattern of tests/test_gpu_bitcount.py: both sides get identical seeded keys, masks and
plaintexts; every case checks the limbs and the degree words against the model, the bounds against
the model, the decrypted results against numpy indexing, and a clean ctx.synchronize().  u8
elements at (64,64,1,64) unless noted.  Shapes are the smallest that reach each path of the kernels
(DESIGN.md s4.4f): a batch that is no multiple of a block's four waves, counts that are no power
of two (a missing right sibling, a wholly missing subtree), the full stack depth at count 256,
null and unit index bits (every skipped product, the literal's flip both ways), operands that fill
their bounds, a shared table, and the existing select and lookup kernels as second references.
"""
import ctypes

import numpy as np
import pytest

import array_model as am
import lookup_model as lm
import synth
from circuit_gpu import encrypt_both, load_engine, make_world
from helpers import assert_batches_equal, bit_ints, plain

gpu = pytest.mark.gpu

U8 = (64, 64, 1, 64)
FRESH = U8[0] + U8[1]
SEED = 2028
B8 = np.full(8, FRESH, np.uint32)


@pytest.fixture(scope="module")
def H():
    return load_engine()


@pytest.fixture(scope="module")
def world(H, oracle):
    return make_world(H, SEED)


def synthetic(H, ctx, values, bound, dtype=None):
    """A device batch of the model polynomials `values` at the per-bit bounds."""
    bound = np.asarray(bound, dtype=np.uint32)
    return H.Ciphered.from_host(*am.pack(values, bound), bound, len(values), ctx.device, dtype)


def assert_equals_model(out, values, what):
    el, ed = am.pack(values, out.bound)
    gl, gd = out.to_host()
    assert_batches_equal(gl, gd, el, ed, out.bound, out.n, what)


def polys(c):
    """Every value of a device batch as model polynomials."""
    l, d = c.to_host()
    return [bit_ints(l, d, c.bound, e) for e in range(c.n)]


def arrays(A, count, shared=False):
    """The model's arrays per index value from the flat list of element values."""
    return (lambda e: A[:count]) if shared else (lambda e: A[e * count:(e + 1) * count])


def check_read(H, ctx, arr, A, idx, S, count, av=None, iv=None, what=""):
    """array_read of device batches (model polynomials A, S; av, iv: the plaintexts, or None when
    the operands do not decrypt to anything meaningful)."""
    n = idx.n
    shared = arr.n == count and n != 1
    out = ctx.array_read(arr, idx, count)
    assert (out.nbits, out.n, out.plain_dtype) == (arr.nbits, n, arr.plain_dtype)
    assert np.array_equal(out.bound, am.read_bounds(arr.bound, count, idx.bound)), what
    get = arrays(A, count, shared)
    assert_equals_model(out, [am.circuit_read(get(e), S[e]) for e in range(n)], what)
    if av is not None:
        got = ctx.decrypt(out)
        want = [am.int_read(av[:count] if shared else av[e * count:(e + 1) * count], int(iv[e]), count)
                for e in range(n)]
        assert got.tolist() == want, what
    ctx.synchronize()
    return out


def check_write(H, ctx, arr, A, idx, S, val, X, count, av=None, iv=None, xv=None, what=""):
    n = idx.n
    out = ctx.array_write(arr, idx, val, count)
    assert (out.nbits, out.n, out.plain_dtype) == (arr.nbits, arr.n, arr.plain_dtype)
    assert np.array_equal(out.bound, am.write_bounds(arr.bound, val.bound, count, idx.bound)), what
    want = []
    for e in range(n):
        want += am.circuit_write(A[e * count:(e + 1) * count], S[e], X[e])
    assert_equals_model(out, want, what)
    if av is not None:
        got = ctx.decrypt(out).reshape(n, count)
        for e in range(n):
            assert got[e].tolist() == am.int_write(av[e * count:(e + 1) * count], int(iv[e]),
                                                   int(xv[e]), count), (what, e)
    ctx.synchronize()
    return out


def fresh_case(H, oracle, world, count, n, seed, index=None):
    """Fresh u8 arrays, indices (every index of k bits in turn, high bits set in some: not read)
    and values written, on both sides."""
    k = am.index_bits(count)
    av = plain(n * count, np.uint8, seed)
    iv = (np.arange(n) % (1 << k)).astype(np.uint8) if index is None else np.asarray(index, np.uint8)
    iv = iv | np.where(np.arange(n) % 2 == 1, np.uint8(0xFF << k & 0xFF), np.uint8(0))
    xv = plain(n, np.uint8, seed + 1)
    arr, A = encrypt_both(H, oracle, world, U8, av, seed + 2)
    idx, S = encrypt_both(H, oracle, world, U8, iv, seed + 3)
    val, X = encrypt_both(H, oracle, world, U8, xv, seed + 4)
    return (arr, A, av), (idx, S, iv), (val, X, xv)


@pytest.fixture(scope="module")
def two(H, oracle, world):
    """Count 2, n = 5 (no multiple of a block's four waves): shared and left unchanged."""
    return fresh_case(H, oracle, world, 2, 5, 100, index=[0, 1, 1, 0, 1])


@pytest.fixture(scope="module")
def four(H, oracle, world):
    """Count 4, every index once: shared and left unchanged."""
    return fresh_case(H, oracle, world, 4, 4, 200)


def condition(H, ctx, S, t):
    """Bit t of every index value as a Ciphered<bool> (bits 1..7 null)."""
    bound = np.array([FRESH] + [0] * 7, np.uint32)
    return synthetic(H, ctx, [[s[t]] + [0] * 7 for s in S], bound, np.dtype(np.bool_))


def element(H, ctx, A, count, v, bound=B8):
    """Element v of every array as a batch of its own."""
    return synthetic(H, ctx, A[v::count], bound, np.dtype(np.uint8))


# ------------------------------------------------------------------ read
@gpu
def test_read_count_2(H, world, two):
    ctx, _ = world(U8)
    (arr, A, av), (idx, S, iv), _ = two
    out = check_read(H, ctx, arr, A, idx, S, 2, av, iv, "read x2")
    assert out.bound.tolist() == [2 * FRESH] * 8
    # limb for limb the select kernel, the u8 index itself as the condition (bit 0 is read)
    ref = ctx.select(idx, element(H, ctx, A, 2, 1), element(H, ctx, A, 2, 0))
    assert np.array_equal(ref.bound, out.bound)
    assert_batches_equal(*out.to_host(), *ref.to_host(), out.bound, 5, "read x2: against select")
    # apply_n routes the marker to ctx.array_read and infers the count
    via = ctx.apply_n(H.HomomorphicArrayRead, [arr, idx])
    assert_batches_equal(*via.to_host(), *out.to_host(), out.bound, 5, "apply_n read")
    ctx.synchronize()


@gpu
def test_read_count_4_equals_the_select_tree(H, world, four):
    ctx, _ = world(U8)
    (arr, A, av), (idx, S, iv), _ = four
    out = check_read(H, ctx, arr, A, idx, S, 4, av, iv, "read x4")
    c0, c1 = condition(H, ctx, S, 0), condition(H, ctx, S, 1)
    el = [element(H, ctx, A, 4, v) for v in range(4)]
    ref = ctx.select(c1, ctx.select(c0, el[3], el[2]), ctx.select(c0, el[1], el[0]))
    assert np.array_equal(ref.bound, out.bound) and out.bound.tolist() == [3 * FRESH] * 8
    assert_batches_equal(*out.to_host(), *ref.to_host(), out.bound, 4, "read x4: select tree")
    ctx.synchronize()


@gpu
@pytest.mark.parametrize("count", [3, 5])
def test_read_counts_that_are_no_power_of_two(H, oracle, world, count):
    """A missing right sibling (count 3: element 2's; count 5: element 4's at two levels, its
    whole right subtree 6..7 missing); indices 3 and 5..7 read 0."""
    ctx, _ = world(U8)
    n = 1 << am.index_bits(count)
    (arr, A, av), (idx, S, iv), _ = fresh_case(H, oracle, world, count, n, 300 + count)
    out = check_read(H, ctx, arr, A, idx, S, count, av, iv, f"read x{count}")
    got = ctx.decrypt(out)
    assert not got[count:].any() and got[:count].tolist() == [int(av[e * count + e]) for e in range(count)]


@gpu
def test_read_of_trivial_elements_equals_the_lookup(H, oracle, world):
    """Count 16, elements that are null / unit polynomials from a random byte table: the read and
    the plaintext-table lookup give the same polynomials; only their static bounds differ."""
    ctx, _ = world(U8)
    table = plain(16, np.uint8, 41)
    iv = np.array([0, 15, 6], np.uint8)
    idx, S = encrypt_both(H, oracle, world, U8, iv, 42)
    T = [[(int(t) >> j) & 1 for j in range(8)] for t in table]
    arr = synthetic(H, ctx, T * 3, np.zeros(8, np.uint32), np.dtype(np.uint8))
    out = check_read(H, ctx, arr, T * 3, idx, S, 16, np.tile(table, 3), iv, "read x16 trivial")
    ref = ctx.lookup(idx, table, in_bits=4)
    assert out.bound.tolist() == [4 * FRESH] * 8 and not np.array_equal(out.bound, ref.bound)
    assert polys(out) == polys(ref) == [lm.lookup_circuit(s, table) for s in S]
    _, od = out.to_host()
    _, rd = ref.to_host()
    assert np.array_equal(od, rd)
    assert np.array_equal(ctx.decrypt(out), ctx.decrypt(ref))
    ctx.synchronize()


@gpu
def test_read_count_256(H, oracle, world):
    """The full stack depth: 256 elements under a u8 index, n = 2."""
    ctx, _ = world(U8)
    (arr, A, av), (idx, S, iv), _ = fresh_case(H, oracle, world, 256, 2, 500, index=[0xA7, 0xFF])
    out = check_read(H, ctx, arr, A, idx, S, 256, av, iv, "read x256")
    assert out.bound.tolist() == [9 * FRESH] * 8


@gpu
def test_read_skewed_bounds_that_are_filled(H, world):
    """Synthetic operands of exact degree = bound: index bits at fresh + 37 t, element bits at
    fresh + 5 j with a zero-bound hole; count 5, so every kind of node occurs."""
    ctx, _ = world(U8)
    rng = np.random.default_rng(6)
    count, n = 5, 3
    sb = (FRESH + 37 * np.arange(8)).astype(np.uint32)
    ab = (FRESH + 5 * np.arange(8)).astype(np.uint32)
    ab[3] = 0
    S = [[synth.poly("FULL", b, rng) for b in sb] for _ in range(n)]
    A = [[synth.poly("FULL" if b else "UNIT", b, rng) for b in ab] for _ in range(n * count)]
    idx, arr = synthetic(H, ctx, S, sb), synthetic(H, ctx, A, ab)
    out = check_read(H, ctx, arr, A, idx, S, count, what="read skewed")
    assert out.bound.tolist() == [int(sb[:3].sum()) + int(b) for b in ab]
    _, od = out.to_host()
    assert (od.reshape(n, 8)[:, [0, 7]] == out.bound[[0, 7]]).all()  # the widest term is unique


@gpu
def test_read_u32_index_reads_two_bits(H, oracle, world, four):
    """A Ciphered<u32> index on count 4: its degree words above bit 1 are garbage, neither read
    nor validated."""
    ctx, _ = world(U8)
    (arr, A, av), (_, S, iv), _ = four
    rng = np.random.default_rng(9)
    b32 = np.full(32, FRESH, np.uint32)
    S32 = [s[:2] + [synth.poly("FULL", FRESH, rng) for _ in range(30)] for s in S]
    idx = synthetic(H, ctx, S32, b32, np.dtype(np.uint32))
    idx.degree[:, 2:] = 0x7FFFFFFF
    out = check_read(H, ctx, arr, A, idx, S32, 4, what="read u32 index")
    assert ctx.decrypt(out).tolist() == [am.int_read(av[4 * e:4 * e + 4], int(iv[e]), 4) for e in range(4)]
    ctx.synchronize()


@gpu
def test_read_null_and_unit_index_bits(H, oracle, world, four):
    """A null s_t takes the left child, a unit s_t the right: exact copies of the chosen element,
    a null one among them; mixed with real bits the products that remain."""
    ctx, _ = world(U8)
    (_, A, _), (_, S, _), _ = four
    x = S[1][0]
    combos = [[0, 0], [1, 0], [0, 1], [1, 1], [x, 0], [1, x], [0, x], [x, 1]]
    n = len(combos)
    els = [A[v] for v in range(4)]
    els[2] = [0] * 8          # a null element, chosen by [0, 1]
    els[3] = els[3][:4] + [1, 0, 1, 0]
    Sx = [c + [0] * 6 for c in combos]
    idx = synthetic(H, ctx, Sx, B8)
    arr = synthetic(H, ctx, els * n, B8, np.dtype(np.uint8))
    out = check_read(H, ctx, arr, els * n, idx, Sx, 4, what="read trivial index")
    got = polys(out)
    for e, v in enumerate([0, 1, 2, 3]):
        assert got[e] == els[v], e
    # a count that is no power of two: the missing sibling under trivial bits (index 2 and 3 of 3)
    Sy = [[0, 1], [1, 1], [x, 1], [0, 0]]
    idy = synthetic(H, ctx, [s + [0] * 6 for s in Sy], B8)
    arr3 = synthetic(H, ctx, els[:3] * 4, B8, np.dtype(np.uint8))
    out = check_read(H, ctx, arr3, els[:3] * 4, idy, [s + [0] * 6 for s in Sy], 3,
                     what="read x3 trivial index")
    got = polys(out)
    assert got[0] == els[2] and got[1] == [0] * 8 and got[3] == els[0]


@gpu
def test_read_shared_table(H, oracle, world, four):
    """arr.n == count: one table read by every index gives what the table tiled n times gives."""
    import torch
    ctx, _ = world(U8)
    (arr, A, av), _, _ = four
    n = 6
    iv = np.array([3, 0, 2, 1, 7, 2], np.uint8)  # (7: bits above k are not read: element 3)
    idx, S = encrypt_both(H, oracle, world, U8, iv, 77)
    table = H.value_slice(arr, 0, 4)
    out = check_read(H, ctx, table, A[:4], idx, S, 4, av[:4], iv, "read shared")
    tiled = H.Ciphered(table.limbs.repeat(n), table.degree.repeat(n, 1), B8, 8, 4 * n,
                       np.dtype(np.uint8))
    ref = ctx.array_read(tiled, idx, 4)
    assert_batches_equal(*out.to_host(), *ref.to_host(), out.bound, n, "shared against tiled")
    assert ctx.decrypt(out).tolist() == [int(av[i & 3]) for i in iv]
    torch.cuda.synchronize()
    ctx.synchronize()


# ------------------------------------------------------------------ write
@gpu
def test_write_count_2(H, world, two):
    ctx, _ = world(U8)
    (arr, A, av), (idx, S, iv), (val, X, xv) = two
    out = check_write(H, ctx, arr, A, idx, S, val, X, 2, av, iv, xv, "write x2")
    assert out.bound.tolist() == [2 * FRESH] * 8
    # limb for limb two selects: element 1 on the index, element 0 on its NOT (on a copy)
    neg = H.Ciphered(idx.limbs.clone(), idx.degree.clone(), idx.bound, 8, 5, idx.plain_dtype)
    ctx.apply1(H.HomomorphicNotGate, neg)
    r1 = ctx.select(idx, val, element(H, ctx, A, 2, 1))
    r0 = ctx.select(neg, val, element(H, ctx, A, 2, 0))
    ref = H.stack_values([r0, r1])
    assert ref.n == 10 and np.array_equal(ref.bound, out.bound)
    assert_batches_equal(*out.to_host(), *ref.to_host(), out.bound, 10, "write x2: two selects")
    via = ctx.apply_n(H.HomomorphicArrayWrite, [arr, idx, val])
    assert_batches_equal(*via.to_host(), *out.to_host(), out.bound, 10, "apply_n write")
    ctx.synchronize()


@gpu
@pytest.mark.parametrize("count", [3, 4, 5])
def test_write_small_counts(H, oracle, world, count):
    """Every index of k bits: those >= count leave every element's plaintext unchanged."""
    ctx, _ = world(U8)
    n = 1 << am.index_bits(count)
    (arr, A, av), (idx, S, iv), (val, X, xv) = fresh_case(H, oracle, world, count, n, 600 + count)
    out = check_write(H, ctx, arr, A, idx, S, val, X, count, av, iv, xv, f"write x{count}")
    got = ctx.decrypt(out).reshape(n, count)
    for e in range(count, n):
        assert got[e].tolist() == av[e * count:(e + 1) * count].tolist()
    for e in range(count):
        assert got[e, e] == xv[e]


@gpu
def test_write_count_256(H, oracle, world):
    ctx, _ = world(U8)
    (arr, A, av), (idx, S, iv), (val, X, xv) = fresh_case(H, oracle, world, 256, 1, 700, index=[0x5C])
    out = check_write(H, ctx, arr, A, idx, S, val, X, 256, av, iv, xv, "write x256")
    assert out.bound.tolist() == [9 * FRESH] * 8


@gpu
def test_write_null_and_unit_index_bits(H, oracle, world, four):
    """The literal's flip both ways (a unit s_t gives a null s_t + 1, a null s_t a unit one), a
    null indicator (an exact copy of the element) and a unit one (the value itself), with a
    unit-polynomial value and null / unit element bits."""
    ctx, _ = world(U8)
    (_, A, _), (_, S, _), (_, X, _) = four
    x = S[1][0]
    combos = [[0, 0], [1, 0], [0, 1], [1, 1], [x, 0], [1, x], [x, x ^ 1]]
    n = len(combos)
    els = [A[v] for v in range(4)]
    els[1] = els[1][:4] + [1, 0, 1, 0]
    Sx = [c + [0] * 6 for c in combos]
    Xs = [X[e % 4] for e in range(n)]
    Xs[0] = [1] * 8           # a value of unit polynomials
    Xs[4] = [1, 0] * 4
    idx, val = synthetic(H, ctx, Sx, B8), synthetic(H, ctx, Xs, B8)
    arr = synthetic(H, ctx, els * n, B8, np.dtype(np.uint8))
    out = check_write(H, ctx, arr, els * n, idx, Sx, val, Xs, 4, what="write trivial index")
    got = polys(out)
    for e in range(4):  # a plaintext index: the element replaced, the others exact copies
        for v in range(4):
            assert got[4 * e + v] == (Xs[e] if v == e else els[v]), (e, v)
    # count 3 under the same index bits: an index of 3 writes nowhere
    arr3 = synthetic(H, ctx, els[:3] * n, B8, np.dtype(np.uint8))
    out = check_write(H, ctx, arr3, els[:3] * n, idx, Sx, val, Xs, 3, what="write x3 trivial index")
    assert polys(out)[9:12] == els[:3]


@gpu
def test_write_skewed_bounds_that_are_filled(H, world):
    ctx, _ = world(U8)
    rng = np.random.default_rng(8)
    count, n = 5, 2
    sb = (FRESH + 37 * np.arange(8)).astype(np.uint32)
    ab = (FRESH + 5 * np.arange(8)).astype(np.uint32)
    ab[3] = 0
    xb = ab[::-1].copy()
    S = [[synth.poly("FULL", b, rng) for b in sb] for _ in range(n)]
    A = [[synth.poly("FULL" if b else "UNIT", b, rng) for b in ab] for _ in range(n * count)]
    X = [[synth.poly("FULL" if b else "NULL", b, rng) for b in xb] for _ in range(n)]
    idx, arr, val = synthetic(H, ctx, S, sb), synthetic(H, ctx, A, ab), synthetic(H, ctx, X, xb)
    out = check_write(H, ctx, arr, A, idx, S, val, X, count, what="write skewed")
    assert out.bound.tolist() == [int(sb[:3].sum()) + max(int(a), int(x)) for a, x in zip(ab, xb)]


@gpu
def test_read_after_write(H, world, four):
    """array_read(array_write(arr, i, x), i) decrypts to x, and at i ^ 1 to the old element."""
    ctx, _ = world(U8)
    (arr, A, av), (idx, S, iv), (val, X, xv) = four
    written = ctx.array_write(arr, idx, val, 4)
    assert ctx.decrypt(ctx.array_read(written, idx, 4)).tolist() == xv.tolist()
    flip = synthetic(H, ctx, [[s[0] ^ 1] + s[1:] for s in S], B8)
    old = ctx.decrypt(ctx.array_read(written, flip, 4))
    assert old.tolist() == [int(av[4 * e + (int(iv[e]) & 3 ^ 1)]) for e in range(4)]
    ctx.synchronize()


# ------------------------------------------------------------------ arguments, requirement, limits
@gpu
def test_argument_errors(H, world, four):
    """Each returns HM_ERR_INVALID_ARGUMENT, writes nothing and leaves the status word clean."""
    import torch
    from homomorph import _lib
    ctx, _ = world(U8)
    (arr, _, _), (idx, _, _), (val, _, _) = four
    INV = _lib.ERR_INVALID_ARGUMENT
    L = _lib.lib()

    def read(arr, count, idx, out):
        ca, ci, co = arr._c(), idx._c(), out._c()
        return L.hm_array_read_batch(ctx._h, ctypes.byref(ca), count, ctypes.byref(ci), ctypes.byref(co))

    def write(arr, count, idx, val, out):
        ca, ci, cv, co = arr._c(), idx._c(), val._c(), out._c()
        return L.hm_array_write_batch(ctx._h, ctypes.byref(ca), count, ctypes.byref(ci),
                                      ctypes.byref(cv), ctypes.byref(co))

    rneed = H.array_read_out_bounds(arr.bound, 4, idx.bound)
    wneed = H.array_write_out_bounds(arr.bound, val.bound, 4, idx.bound)
    rout, wout = H.Ciphered.empty(4, rneed, ctx.device), H.Ciphered.empty(16, wneed, ctx.device)
    for o in (rout, wout):
        o.limbs.fill_(-1)
        o.degree.fill_(-1)
    torch.cuda.synchronize()
    # out overlapping arr (its limbs, or its degree words alone), the index or the value
    assert read(arr, 4, idx, H.Ciphered(arr.limbs, rout.degree, rneed, 8, 4)) == INV
    assert read(arr, 4, idx, H.Ciphered(rout.limbs, arr.degree, rneed, 8, 4)) == INV
    assert read(arr, 4, idx, H.Ciphered(rout.limbs, idx.degree, rneed, 8, 4)) == INV
    assert write(arr, 4, idx, val, H.Ciphered(arr.limbs, wout.degree, wneed, 8, 16)) == INV
    assert write(arr, 4, idx, val, H.Ciphered(wout.limbs, val.degree, wneed, 8, 16)) == INV
    # arr.n neither count * n nor count
    assert read(H.value_slice(arr, 0, 12), 4, idx, rout) == INV
    assert read(arr, 2, idx, rout) == INV
    assert write(H.value_slice(arr, 0, 4), 4, idx, val, H.value_slice(wout, 0, 4)) == INV  # no shared form
    assert write(arr, 4, idx, H.value_slice(val, 0, 3), wout) == INV
    assert write(arr, 4, idx, val, H.value_slice(wout, 0, 12)) == INV
    assert read(arr, 4, idx, H.value_slice(rout, 0, 3)) == INV
    # a too-small output bound, a wrong output width
    for need, out, call in ((rneed, rout, lambda o: read(arr, 4, idx, o)),
                            (wneed, wout, lambda o: write(arr, 4, idx, val, o))):
        low = need.copy()
        low[5] -= 1
        assert call(H.Ciphered(out.limbs, out.degree, low, 8, out.n)) == INV
        assert call(H.Ciphered.empty(out.n, np.full(16, 2048, np.uint32), ctx.device)) == INV
    # index.nbits < k, count outside 2..256, null batches
    one_bit = H.Ciphered.empty(4, idx.bound[:1], ctx.device)
    assert read(arr, 4, one_bit, rout) == INV and write(arr, 4, one_bit, val, wout) == INV
    for count in (0, 1, 257):
        assert read(arr, count, idx, rout) == INV and write(arr, count, idx, val, wout) == INV
    ca, ci, co = arr._c(), idx._c(), rout._c()
    assert L.hm_array_read_batch(ctx._h, None, 4, ctypes.byref(ci), ctypes.byref(co)) == INV
    assert L.hm_array_read_batch(ctx._h, ctypes.byref(ca), 4, None, ctypes.byref(co)) == INV
    assert L.hm_array_write_batch(ctx._h, ctypes.byref(ca), 4, ctypes.byref(ci), None, ctypes.byref(co)) == INV
    ctx.synchronize()  # clean
    torch.cuda.synchronize()
    for o in (rout, wout):
        assert bool((o.limbs == -1).all()) and bool((o.degree == -1).all())  # nothing was written
    # larger out bounds are accepted; n == 0 is HM_OK
    assert read(arr, 4, idx, H.Ciphered.empty(4, rneed + 70, ctx.device)) == _lib.OK
    assert write(arr, 4, idx, val, H.Ciphered.empty(16, wneed + 70, ctx.device)) == _lib.OK
    e8 = lambda n: H.Ciphered.empty(n, B8, ctx.device)  # noqa: E731
    assert read(e8(0), 4, e8(0), H.Ciphered.empty(0, rneed, ctx.device)) == _lib.OK
    assert write(e8(0), 4, e8(0), e8(0), H.Ciphered.empty(0, wneed, ctx.device)) == _lib.OK
    ctx.synchronize()
    with pytest.raises(ValueError):
        ctx.array_read(arr, idx, 1)
    with pytest.raises(ValueError):
        ctx.apply_n(H.HomomorphicArrayRead, [H.value_slice(arr, 0, 15), idx])


@gpu
def test_corrupted_degree_word(H, oracle, world):
    """An element whose degree word disagrees with its limbs, or an index bit's, or the value's, is
    flagged at synchronise; afterwards the flag is clear."""
    from homomorph import _lib
    ctx, _ = world(U8)
    (arr, A, av), (idx, S, iv), (val, X, xv) = fresh_case(H, oracle, world, 3, 4, 800)
    ctx.synchronize()
    for batch, pos in ((arr, (11, 6)), (idx, (2, 1)), (val, (3, 7))):
        for op in ("read", "write"):
            if batch is val and op == "read":
                continue
            batch.degree[pos] += 1
            if op == "read":
                ctx.array_read(arr, idx, 3)
            else:
                ctx.array_write(arr, idx, val, 3)
            with pytest.raises(H.EngineError) as ei:
                ctx.synchronize()
            assert ei.value.status == _lib.ERR_BAD_INPUT
            batch.degree[pos] -= 1
    got = ctx.decrypt(ctx.array_read(arr, idx, 3))
    ctx.synchronize()  # clean: the flag was cleared by the check
    assert got.tolist() == [am.int_read(av[3 * e:3 * e + 3], int(iv[e]), 3) for e in range(4)]
    # an index bit above k is not validated
    idx.degree[0, 2] += 1
    ctx.array_read(arr, idx, 3)
    ctx.synchronize()
    idx.degree[0, 2] -= 1


@gpu
def test_requirement(H):
    """2k + 3 for k index bits, through the markers and the engine."""
    from homomorph import _lib
    L = _lib.lib()
    ctx = H.Context(H.Parameters(7, 8, 1, 8))  # d / delta = 7: count 4 passes, count 5 needs 9
    ctx.seed_rng(5)
    ctx.generate_secret_key()
    ctx.generate_public_key()
    av = np.arange(16, dtype=np.uint8) * 9
    iv = np.array([2, 0, 3, 1], np.uint8)
    xv = np.array([200, 201, 202, 203], np.uint8)
    arr, idx, val = ctx.encrypt(av), ctx.encrypt(iv), ctx.encrypt(xv)
    assert ctx.decrypt(ctx.array_read(arr, idx, 4)).tolist() == [int(av[4 * e + iv[e]]) for e in range(4)]
    got = ctx.decrypt(ctx.array_write(arr, idx, val, 4)).reshape(4, 4)
    assert [int(got[e, iv[e]]) for e in range(4)] == xv.tolist()
    ctx.synchronize()
    a5 = ctx.encrypt(np.arange(20, dtype=np.uint8))
    for call in (lambda: ctx.array_read(a5, idx, 5), lambda: ctx.array_write(a5, idx, val, 5)):
        with pytest.raises(H.OperationError) as ei:
            call()
        assert ei.value.required_min_d_over_delta == 9
        assert (ei.value.actual_d, ei.value.actual_delta) == (7, 1)
    out = H.Ciphered.empty(4, H.array_read_out_bounds(a5.bound, 5, idx.bound), ctx.device)
    with pytest.raises(H.EngineError) as ei:
        H.array_read_into(ctx, a5, idx, 5, out)
    assert ei.value.status == _lib.ERR_INVALID_PARAMETERS
    ctx.synchronize()
    wide = H.Context(H.Parameters(300, 64, 1, 8))  # no keys: validation needs none
    req = ctypes.c_uint16()
    for marker in (H.HomomorphicArrayRead, H.HomomorphicArrayWrite):
        assert L.hm_validate_operation(wide._h, marker.CODE, ctypes.byref(req)) == _lib.ERR_INVALID_ARGUMENT
        for count, want in ((2, 5), (4, 7), (16, 11), (256, 19)):
            k = marker.index_bits(count)
            assert L.hm_validate_operation_bits(wide._h, marker.CODE, k, ctypes.byref(req)) == _lib.OK
            assert req.value == want == marker.min_d_over_delta(k)
        for k in (0, 9, 128):
            assert L.hm_validate_operation_bits(wide._h, marker.CODE, k, None) == _lib.ERR_INVALID_ARGUMENT
        wide.validate_operation(marker, 8)
        with pytest.raises(ValueError):
            wide.validate_operation(marker)


@gpu
def test_lds_limit_is_refused_before_any_launch(H, world):
    """256 elements at bound 2048 on every bit: the eight waiting left children do not fit a
    wave's 2560 words; refused, the output left as it was."""
    import torch
    from homomorph import _lib
    ctx, _ = world(U8)
    big = np.full(8, 2048, np.uint32)
    arr, idx = H.Ciphered.empty(256, big, ctx.device), H.Ciphered.empty(1, big, ctx.device)
    for c in (arr, idx):
        c.limbs.zero_()
        c.degree.zero_()
    out = H.Ciphered.empty(1, H.array_read_out_bounds(big, 256, big), ctx.device)
    wout = H.Ciphered.empty(256, H.array_write_out_bounds(big, big, 256, big), ctx.device)
    for o in (out, wout):
        o.limbs.fill_(-1)
        o.degree.fill_(-1)
    torch.cuda.synchronize()
    with pytest.raises(H.EngineError) as ei:
        H.array_read_into(ctx, arr, idx, 256, out)
    assert ei.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(H.EngineError) as ei:
        H.array_write_into(ctx, arr, idx, idx, 256, wout)
    assert ei.value.status == _lib.ERR_UNSUPPORTED
    ctx.synchronize()
    torch.cuda.synchronize()
    for o in (out, wout):
        assert bool((o.limbs == -1).all()) and bool((o.degree == -1).all())


@gpu
def test_graph_replay_equals_direct_call(H, world, four):
    """Replays into buffers prefilled with -1: every limb and degree word is written."""
    import torch
    ctx, _ = world(U8)
    (arr, _, _), (idx, _, _), (val, _, _) = four
    direct_r, direct_w = ctx.array_read(arr, idx, 4), ctx.array_write(arr, idx, val, 4)
    got_r = H.Ciphered.empty(4, direct_r.bound, ctx.device, np.dtype(np.uint8))
    got_w = H.Ciphered.empty(16, direct_w.bound, ctx.device, np.dtype(np.uint8))

    def both():
        H.array_read_into(ctx, arr, idx, 4, got_r)
        H.array_write_into(ctx, arr, idx, val, 4, got_w)

    g = ctx.graph(both)
    for o in (got_r, got_w):
        o.limbs.fill_(-1)
        o.degree.fill_(-1)
    torch.cuda.synchronize()  # the fills ran on torch's stream, the replay on the engine's
    g.replay()
    ctx.synchronize()
    assert_batches_equal(*got_r.to_host(), *direct_r.to_host(), direct_r.bound, 4, "graph read")
    assert_batches_equal(*got_w.to_host(), *direct_w.to_host(), direct_w.bound, 16, "graph write")
