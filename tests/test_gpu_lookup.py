"""GPU: homomorphic table lookup (hm_lookup_batch) against the model circuit
(tests/lookup_model.py over oracle/gf2_model.py), bit-exact.

The pattern of tests/test_gpu_select.py: both sides get identical seeded keys, masks and
plaintexts; every case checks the limbs and the degree words against the model, the bounds against
the model, the decrypted results against table[v], and a clean ctx.synchronize().  Shapes are the
smallest that reach each path of the kernel: null and unit inner sums, the
t = 0-only path, one product and fifteen products per output bit, every split of the index bits.
The last test reads the kernel's code object and needs no GPU.
"""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import lookup_model as lm
import select_model as sm
from circuit_gpu import encrypt_both, load_engine, make_world
from helpers import assert_batches_equal, plain

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8, U16, U32 = (64, 64, 1, 64), (64, 32, 1, 32), (128, 128, 1, 128)
SEED = 2025


@pytest.fixture(scope="module")
def H():
    return load_engine()


@pytest.fixture(scope="module")
def world(H, oracle):
    return make_world(H, SEED)


def random_table(k, dtype, seed):
    info = np.iinfo(dtype)
    return np.random.default_rng(seed).integers(info.min, info.max, size=1 << k, dtype=dtype,
                                                endpoint=True)


def assert_equals_model(out, values, what):
    """The device batch against the model's bit polynomials per value, limbs and degree words."""
    el, ed = lm.pack(values, out.bound)
    gl, gd = out.to_host()
    assert_batches_equal(gl, gd, el, ed, out.bound, out.n, what)


def check_lookup(ctx, a, A, av, table, in_bits=None, what=""):
    """lookup(a, table) of a device batch (model polynomials A, plaintexts av as unsigned)."""
    out = ctx.lookup(a, table, in_bits)
    k = min(a.nbits, 8) if in_bits is None else in_bits
    t = np.asarray(table)
    assert out.nbits == 8 * t.dtype.itemsize and out.n == a.n and out.plain_dtype == t.dtype
    assert np.array_equal(out.bound, lm.lookup_bounds(a.bound[:k], t)), what
    assert_equals_model(out, [lm.lookup_circuit(A[e][:k], t) for e in range(a.n)], what)
    idx = (av.astype(np.uint64) & np.uint64((1 << k) - 1)).astype(np.int64)
    assert np.array_equal(ctx.decrypt(out), t[idx]), what
    ctx.synchronize()
    return out


FIVE = np.concatenate([np.array([0, 255, 128], np.uint8), plain(2, np.uint8, 3)])


@pytest.fixture(scope="module")
def five(H, oracle, world):
    """The first case's batch, shared and left unchanged: 0, 255, 128 and two random bytes at
    (64,64,1,64); five is no multiple of the four waves of a block."""
    return encrypt_both(H, oracle, world, U8, FIVE, 11)


@gpu
def test_u8_random_table(H, world, five):
    ctx, _ = world(U8)
    a, A = five
    check_lookup(ctx, a, A, FIVE, random_table(8, np.uint8, 1), what="u8 random")
    # a signed table, indexed by a signed value's bit pattern
    relu = np.maximum(np.arange(256).astype(np.uint8).view(np.int8), 0)
    signed = H.Ciphered(a.limbs, a.degree, a.bound, 8, a.n, np.dtype(np.int8))
    out = check_lookup(ctx, signed, A, FIVE, relu, what="relu")
    assert np.array_equal(ctx.decrypt(out), np.maximum(FIVE.view(np.int8), 0))


@gpu
@pytest.mark.parametrize("name", ["identity", "zero", "ones", "not", "parity", "is255", "popcount"])
def test_structured_tables(H, world, five, name):
    """Null inner sums (constants, identity), unit inner sums (identity's high bits, NOT), the
    t = 0-only path (identity's low bits, parity's low half), the single product (v == 255)."""
    ctx, _ = world(U8)
    a, A = five
    v = np.arange(256)
    pop = np.array([bin(x).count("1") for x in v])
    t = {"identity": v, "zero": 0 * v, "ones": 0 * v + 255, "not": 255 - v, "parity": pop & 1,
         "is255": v == 255, "popcount": pop}[name].astype(np.uint8)
    out = check_lookup(ctx, a, A, FIVE, t, what=name)
    if name == "identity":
        assert np.array_equal(out.bound, a.bound)
        assert_equals_model(out, A, "identity: the input, limb for limb")
    if name in ("zero", "ones"):
        assert not out.bound.any()
        assert_equals_model(out, [[int(name == "ones")] * 8] * 5, "constant: null / unit")
    if name == "parity":
        assert out.bound.tolist() == [128] + [0] * 7
    if name == "is255":
        assert out.bound.tolist() == [8 * 128] + [0] * 7


@gpu
def test_u8_to_u32_headline_parameters(H, oracle, world):
    """(128,128,1,128), n = 3: 32 output bits of up to 8 D = 2048 bits."""
    ctx, _ = world(U32)
    av = np.array([255, 0, plain(1, np.uint8, 5)[0]], np.uint8)
    a, A = encrypt_both(H, oracle, world, U32, av, 21)
    check_lookup(ctx, a, A, av, random_table(8, np.uint32, 2), what="u8->u32")


@gpu
def test_one_index_bit_on_a_comparison(H, oracle, world):
    """in_bits = 1 on a < b of u8 operands: a deep index (bound 9 D) and no product at all:
    out_j = t0_j + (t0_j ^ t1_j) c."""
    ctx, _ = world(U8)
    av, bv = plain(4, np.uint8, 31), plain(4, np.uint8, 32)
    bv[0] = av[0]
    a, A = encrypt_both(H, oracle, world, U8, av, 33)
    b, B = encrypt_both(H, oracle, world, U8, bv, 34)
    lt = ctx.apply2(H.HomomorphicLessThan, a, b, signed=False)
    assert lt.bound.tolist() == [9 * 128] + [0] * 7
    LT = [[sm.less_than(A[e], B[e])] + [0] * 7 for e in range(4)]
    t = np.array([0x5A, 0xC3], np.uint8)
    out = check_lookup(ctx, lt, LT, (av < bv).astype(np.uint8), t, in_bits=1, what="bool index")
    want = [[((0x5A >> j) & 1) ^ ((((0x5A ^ 0xC3) >> j) & 1) * LT[e][0]) for j in range(8)]
            for e in range(4)]
    assert_equals_model(out, want, "t0 + (t0 ^ t1) c")
    # a bool table: the negated comparison
    no = check_lookup(ctx, lt, LT, (av < bv).astype(np.uint8), np.array([True, False]), in_bits=1,
                      what="bool table")
    assert no.plain_dtype == np.bool_ and np.array_equal(ctx.decrypt(no), av >= bv)


@gpu
@pytest.mark.parametrize("in_bits,dtype", [(3, np.uint8), (5, np.uint16)])
def test_low_bits_of_a_u16_batch(H, oracle, world, in_bits, dtype):
    """The low bits of a wider batch read in place (degree stride 16), splits kl, kh = 2, 1 and
    3, 2, input bounds fresh + 37 i."""
    ctx, _ = world(U16)
    av = np.concatenate([np.array([0xFFFF, 0], np.uint16), plain(2, np.uint16, 41)])
    skew = (U16[0] + U16[1] + 37 * np.arange(16)).astype(np.uint32)
    a, A = encrypt_both(H, oracle, world, U16, av, 42, bound=skew)
    for seed in (3, 4):
        check_lookup(ctx, a, A, av, random_table(in_bits, dtype, seed), in_bits=in_bits,
                     what=f"u16 low {in_bits}")
    top = (np.arange(1 << in_bits) == (1 << in_bits) - 1).astype(dtype)
    out = check_lookup(ctx, a, A, av, top, in_bits=in_bits, what="u16 top monomial")
    assert out.bound[0] == skew[:in_bits].sum()


@gpu
def test_trivial_ciphertexts(H, oracle, world):
    """All-zero masks: every index bit is the null or the unit polynomial, so is every monomial."""
    ctx, _ = world(U8)
    av = np.array([0, 255, 0x5A, 128], np.uint8)
    a, A = encrypt_both(H, oracle, world, U8, av, 51, zero_masks=True)
    assert all(p in (0, 1) for v in A for p in v)
    t = random_table(8, np.uint16, 6)
    out = check_lookup(ctx, a, A, av, t, what="trivial")
    assert_equals_model(out, [[(int(t[x]) >> j) & 1 for j in range(16)] for x in av],
                        "trivial: the table's bits")


@gpu
def test_single_value_and_empty_batch(H, oracle, world):
    ctx, _ = world(U8)
    av = plain(1, np.uint8, 61)
    a, A = encrypt_both(H, oracle, world, U8, av, 62)
    t = random_table(8, np.uint8, 7)
    check_lookup(ctx, a, A, av, t, what="n=1")
    e = H.Ciphered.empty(0, a.bound, ctx.device, np.dtype(np.uint8))
    out = ctx.lookup(e, t)
    assert out.n == 0 and out.nbits == 8
    ctx.synchronize()


@gpu
def test_graph_replay_equals_direct_call(H, world, five):
    """Replays into buffers prefilled with -1: every limb and degree word is written."""
    import torch
    ctx, _ = world(U8)
    a, _ = five
    t = random_table(8, np.uint16, 8)
    direct = ctx.lookup(a, t)
    got = H.Ciphered.empty(5, direct.bound, ctx.device, np.dtype(np.uint16))
    g = ctx.graph(lambda: H.lookup_into(ctx, a, t, got))
    got.limbs.fill_(-1)
    got.degree.fill_(-1)
    torch.cuda.synchronize()  # the fills ran on torch's stream, the replay runs on the engine's
    g.replay()
    ctx.synchronize()
    gl, gd = got.to_host()
    wl, wd = direct.to_host()
    assert_batches_equal(gl, gd, wl, wd, direct.bound, 5, "graph replay")
    assert np.array_equal(ctx.decrypt(got), t[FIVE])


@gpu
def test_argument_errors(H, world, five):
    from homomorph import _lib
    ctx, _ = world(U8)
    a, _ = five
    t = random_table(8, np.uint32, 9)
    raw = np.ascontiguousarray(t.astype("<u4")).view(np.uint8)
    tp = raw.ctypes.data_as(_lib.u8p)
    ident = np.arange(256, dtype=np.uint8)

    def call(a, in_bits, table, nbytes, out):
        ca, co = a._c(), out._c()
        return _lib.lib().hm_lookup_batch(ctx._h, ctypes.byref(ca), in_bits, table, nbytes,
                                          ctypes.byref(co))

    need8 = H.lookup_out_bounds(a.bound, raw[:256])
    out8 = H.Ciphered.empty(5, need8, ctx.device)
    assert call(a, 8, tp, 1, out8) == _lib.OK
    nibble = H.Ciphered.empty(5, a.bound[:4], ctx.device)
    for bad_bits, src in ((0, a), (9, a), (5, nibble)):
        assert call(src, bad_bits, tp, 1, out8) == _lib.ERR_INVALID_ARGUMENT
    # the output has 8 out_nbytes bits, out_nbytes is 1, 2 or 4
    assert call(a, 8, tp, 2, out8) == _lib.ERR_INVALID_ARGUMENT
    for nbytes in (3, 8):
        wide = H.Ciphered.empty(5, np.full(8 * nbytes, 1024, np.uint32), ctx.device)
        assert call(a, 8, tp, nbytes, wide) == _lib.ERR_INVALID_ARGUMENT
    # short output bounds, in bit 0 and in the top bit
    need32 = H.lookup_out_bounds(a.bound, t)
    assert need32[0] > 0 and need32[31] > 0
    assert call(a, 8, tp, 4, H.Ciphered.empty(5, need32, ctx.device)) == _lib.OK
    for k in (0, 31):
        low = need32.copy()
        low[k] -= 1
        assert call(a, 8, tp, 4, H.Ciphered.empty(5, low, ctx.device)) == _lib.ERR_INVALID_ARGUMENT
    # mismatched n
    assert call(a, 8, tp, 1, H.Ciphered.empty(4, need8, ctx.device)) == _lib.ERR_INVALID_ARGUMENT
    # the output may not overlap the input: its limbs, or its degree words alone
    ip = ident.ctypes.data_as(_lib.u8p)
    same = H.Ciphered(a.limbs, a.degree, a.bound, 8, 5)
    assert call(a, 8, ip, 1, same) == _lib.ERR_INVALID_ARGUMENT
    other = H.Ciphered.empty(5, a.bound, ctx.device)
    assert call(a, 8, ip, 1, H.Ciphered(other.limbs, a.degree, a.bound, 8, 5)) \
        == _lib.ERR_INVALID_ARGUMENT
    assert call(a, 8, ip, 1, other) == _lib.OK
    # a null table
    assert call(a, 8, None, 1, out8) == _lib.ERR_INVALID_ARGUMENT
    # the Python layer refuses a table of the wrong size or type before the engine sees it
    with pytest.raises(ValueError):
        ctx.lookup(a, ident[:100])
    with pytest.raises(H.EngineError) as ei:
        ctx.lookup(nibble, ident[:32], in_bits=5)
    assert ei.value.status == _lib.ERR_INVALID_ARGUMENT
    ctx.synchronize()


@gpu
def test_requirement_is_2n_plus_1(H):
    """A byte index needs d >= 17 delta: (16,8,1,8) fails with required 17, (17,8,1,8) passes and
    decrypts (its model is checked in test_lookup_host.py)."""
    from homomorph import _lib
    av = np.array([0, 255, 0x5A, 77], np.uint8)
    t = random_table(8, np.uint16, 10)
    for d, ok in ((16, False), (17, True)):
        ctx = H.Context(H.Parameters(d, 8, 1, 8))
        ctx.seed_rng(5)
        ctx.generate_secret_key()
        ctx.generate_public_key()
        a = ctx.encrypt(av)
        if ok:
            assert np.array_equal(ctx.decrypt(ctx.lookup(a, t)), t[av])
            ctx.synchronize()
            continue
        with pytest.raises(H.OperationError) as ei:
            ctx.lookup(a, t)
        assert ei.value.required_min_d_over_delta == 17
        assert (ei.value.actual_d, ei.value.actual_delta) == (16, 1)
        out = H.Ciphered.empty(4, H.lookup_out_bounds(a.bound, t), ctx.device)
        with pytest.raises(H.EngineError) as ei:
            H.lookup_into(ctx, a, t, out)
        assert ei.value.status == _lib.ERR_INVALID_PARAMETERS
        # fewer index bits need less: a nibble 9, a bool 3
        assert np.array_equal(ctx.decrypt(ctx.lookup(a, t[:16], in_bits=4)), t[av & 15])
        ctx.synchronize()


@gpu
def test_validate_entries(H):
    from homomorph import _lib
    L = _lib.lib()
    ctx = H.Context(H.Parameters(300, 64, 1, 8))  # no keys: validation needs none
    req = ctypes.c_uint16()
    assert L.hm_validate_operation(ctx._h, _lib.OP_LOOKUP, ctypes.byref(req)) == _lib.ERR_INVALID_ARGUMENT
    for nbits in (1, 4, 8, 128):
        assert L.hm_validate_operation_bits(ctx._h, _lib.OP_LOOKUP, nbits, ctypes.byref(req)) == _lib.OK
        assert req.value == 2 * nbits + 1
    for nbits in (0, 129):
        assert (L.hm_validate_operation_bits(ctx._h, _lib.OP_LOOKUP, nbits, None)
                == _lib.ERR_INVALID_ARGUMENT)
    ctx.validate_operation(H.HomomorphicLookup, 8)
    with pytest.raises(ValueError):
        ctx.validate_operation(H.HomomorphicLookup)
    tight = H.Context(H.Parameters(16, 8, 1, 8))
    with pytest.raises(H.OperationError) as ei:
        tight.validate_operation(H.HomomorphicLookup, 8)
    assert ei.value.required_min_d_over_delta == 17
    tight.validate_operation(H.HomomorphicLookup, 7)


@gpu
def test_corrupted_degree_words(H, oracle, world):
    """A corrupted degree word in a bit the lookup reads is flagged whether or not the table uses
    the bit; the same corruption above in_bits is not looked at."""
    from homomorph import _lib
    ctx, _ = world(U16)
    av = plain(4, np.uint16, 71)
    a, _ = encrypt_both(H, oracle, world, U16, av, 72)
    ctx.synchronize()
    t = random_table(8, np.uint8, 11)
    bit0 = (np.arange(256) & 1).astype(np.uint8)  # uses index bit 0 only
    a.degree[2, 9] += 1  # not read: in_bits = 8
    assert np.array_equal(ctx.decrypt(ctx.lookup(a, t, in_bits=8)), t[av & 255])
    ctx.synchronize()
    a.degree[2, 5] += 1  # the limbs have no coefficient there (or it is past the bound)
    for table in (t, bit0):
        ctx.lookup(a, table, in_bits=8)
        with pytest.raises(H.EngineError) as ei:
            ctx.synchronize()
        assert ei.value.status == _lib.ERR_BAD_INPUT
    ctx.lookup(a, t[:32], in_bits=5)  # bits 0..4 are sound
    ctx.synchronize()  # clean: the flag was cleared by the checks


@gpu
def test_lds_limit_is_refused_before_any_launch(H, world):
    """A byte index at bound 20 000 per bit: two product-width buffers alone are 2 x 5 000 words
    per wave, 160 KB per block."""
    from homomorph import _lib
    ctx, _ = world(U8)
    big = H.Ciphered.empty(1, np.full(8, 20000, np.uint32), ctx.device, np.dtype(np.uint8))
    with pytest.raises(H.EngineError) as ei:
        ctx.lookup(big, random_table(8, np.uint8, 12))
    assert ei.value.status == _lib.ERR_UNSUPPORTED
    ctx.synchronize()


def test_kernel_has_no_private_segment_and_uniform_argument_reads():
    """lookup_kernel's code object (tools/kernarg_audit.py, as tests/test_kernarg_audit.py uses
    it): no private segment, and the by-value coefficient masks, offsets and bounds are read with
    scalar loads only.  No GPU needed."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernarg_audit
    pkg = os.path.join(ROOT, "homomorph-rust_amd")
    subprocess.run(["make", "-C", pkg, "-j8", "-s"], check=True, capture_output=True)
    res = {}
    for obj in sorted(glob.glob(os.path.join(pkg, "build", "kernels.o"))):
        res.update(kernarg_audit.parse(obj))
    k = res["_ZN2hm13lookup_kernelENS_10LookupArgsE"]
    assert k["private"] == 0
    assert not k["findings"], k["findings"][:2]
