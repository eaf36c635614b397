"""CPU checks of the ripple-borrow operations (subtraction and comparisons):
the host-only bounds entry points against the circuit's recurrences, the bounds against the model
circuits' actual degrees, and the model circuits themselves against numpy after decryption.
No GPU, no launch.
"""
import numpy as np
import pytest

import borrow_model as bm
from helpers import as_bytes, bit_ints, keys, masks, plain

OPS = {"eq": "HomomorphicEqual", "ne": "HomomorphicNotEqual", "lt": "HomomorphicLessThan",
       "le": "HomomorphicLessEqual", "gt": "HomomorphicGreaterThan",
       "ge": "HomomorphicGreaterEqual"}

# (d, dp, delta, tau), unsigned dtype, signed dtype
SETS = [((64, 64, 1, 64), np.uint8, np.int8),
        ((64, 32, 1, 32), np.uint16, np.int16),
        ((128, 128, 1, 128), np.uint32, np.int32),
        ((256, 64, 1, 64), np.uint64, np.int64),
        ((64, 64, 3, 64), np.uint8, np.int8)]


@pytest.fixture(scope="module")
def H():
    import homomorph
    homomorph.lib()
    return homomorph


def test_bounds_at_u32_d256(H):
    D = np.full(32, 256, np.uint32)
    sb = H.sub_out_bounds(D, D)
    assert sb[0] == 256 and all(sb[i] == (i + 1) * 256 for i in range(1, 32))
    assert H.batch_stride(sb) == 2144  # 17 152 B per value
    for op in ("lt", "le", "gt", "ge"):
        assert H.compare_out_bounds(getattr(H, OPS[op]), D, D).tolist() == [8448] + [0] * 7
    for op in ("eq", "ne"):
        assert H.compare_out_bounds(getattr(H, OPS[op]), D, D).tolist() == [8192] + [0] * 7


@pytest.mark.parametrize("nbits", [1, 8, 16, 64, 128])
def test_bounds_equal_the_recurrences(H, nbits):
    rng = np.random.default_rng(nbits)
    uniform = np.full(nbits, 192, np.uint32)
    skew_a = (192 + 37 * np.arange(nbits)).astype(np.uint32)
    skew_b = rng.integers(0, 700, size=nbits).astype(np.uint32)
    for ba, bb in ((uniform, uniform), (skew_a, uniform), (skew_a, skew_b), (skew_b, skew_a)):
        assert np.array_equal(H.sub_out_bounds(ba, bb), bm.sub_bounds(ba, bb))
        for op in bm.COMPARISONS:
            got = H.compare_out_bounds(getattr(H, OPS[op]), ba, bb)
            assert np.array_equal(got, bm.compare_bounds(op, ba, bb)), op


def test_bounds_reject_bad_arguments(H):
    from homomorph import _lib
    L = _lib.lib()
    a = np.full(4, 10, np.uint32)
    out = np.zeros(8, np.uint32)
    p = lambda x: x.ctypes.data_as(_lib.u32p)  # noqa: E731
    assert L.hm_sub_out_bounds(0, p(a), p(a), p(out)) == _lib.ERR_INVALID_ARGUMENT
    assert L.hm_compare_out_bounds(_lib.OP_LT, 0, p(a), p(a), p(out)) == _lib.ERR_INVALID_ARGUMENT
    for code in (_lib.OP_AND, _lib.OP_ADD, _lib.OP_MUL_SIGNED, _lib.OP_SUB, 14, 99):
        assert L.hm_compare_out_bounds(code, 4, p(a), p(a), p(out)) == _lib.ERR_INVALID_ARGUMENT
    for code in range(_lib.OP_EQ, _lib.OP_GE + 1):
        assert L.hm_compare_out_bounds(code, 4, p(a), p(a), p(out)) == _lib.OK
    assert L.hm_sub_out_bounds(4, p(a), p(a), p(out)) == _lib.OK


def test_requirement_by_width(H):
    assert H.HomomorphicSubtraction.min_d_over_delta(32) == 65
    assert H.HomomorphicEqual.min_d_over_delta(32) == 65
    assert H.HomomorphicNotEqual.min_d_over_delta(32) == 65
    for op in ("lt", "le", "gt", "ge"):
        assert getattr(H, OPS[op]).min_d_over_delta(32) == 67
    assert H.HomomorphicLessThan.min_d_over_delta(8) == 19


def _pairs(n, udt, seed):
    """Random, equal and off-by-one value pairs (bit patterns, as the unsigned dtype)."""
    a, b = plain(n, udt, seed), plain(n, udt, seed + 1)
    b[1] = a[1]
    b[2] = a[2] + udt(1)  # wraps at the maximum
    a[3], b[3] = np.iinfo(udt).max, 0
    return a, b


@pytest.mark.parametrize("params,udt,sdt", SETS)
def test_model_circuits_decrypt_to_numpy(oracle, model, params, udt, sdt):
    """The circuits on fresh ciphertexts decrypt to numpy's -, ==, <, ... (signed and unsigned),
    and their actual degrees stay within the static bounds."""
    d, dp, delta, tau = params
    nbits = 8 * np.dtype(udt).itemsize
    n = 5
    sk, pk, _ = keys(d, dp, delta, tau, 31)
    s = model.limbs_to_int(sk)
    bound = np.full(nbits, d + dp, np.uint32)
    a, b = _pairs(n, udt, 7)
    la, da = oracle.encrypt_batch(pk, as_bytes(a), masks(n, nbits, tau, 3), bound)
    lb, db = oracle.encrypt_batch(pk, as_bytes(b), masks(n, nbits, tau, 4), bound)
    sb = bm.sub_bounds(bound, bound)
    cb = {op: bm.compare_bounds(op, bound, bound)[0] for op in bm.COMPARISONS}
    with np.errstate(over="ignore"):
        diff = (a - b).astype(udt)
    for e in range(n):
        A, B = bit_ints(la, da, bound, e), bit_ints(lb, db, bound, e)
        out = bm.sub_circuit(A, B)
        assert all(model.degree(p) <= int(sb[i]) for i, p in enumerate(out))
        assert bm.decrypt_value(out, s) == int(diff[e]), (e, a[e], b[e])
        for signed, dt in ((False, udt), (True, sdt)):
            x, y = a.view(dt)[e], b.view(dt)[e]
            for op in bm.COMPARISONS:
                r = bm.compare_circuit(op, A, B, signed)
                assert model.degree(r) <= int(cb[op]), op
                assert model.decipher_bit(r, s) == int(bm.NUMPY_OPS[op](x, y)), (op, signed, x, y)
        # a value compared with itself: x_i = 0, so == is exactly the unit polynomial
        # (< is not the null polynomial there, a_i a_i + a_i is only noise: it decrypts to 0)
        assert bm.compare_circuit("eq", A, A) == 1
        assert model.decipher_bit(bm.compare_circuit("lt", A, A), s) == 0
