"""CPU checks of select, min and max: the host-only bounds entry points against
the recurrences of tests/select_model.py, the model circuits against numpy after decryption (with
their degrees against the bounds, and min against select(a < b, a, b)), and the requirement
numbers.  No GPU, no launch.
"""
import ctypes

import numpy as np
import pytest

import borrow_model as bm
import select_model as sm
from helpers import as_bytes, bit_ints, keys, masks, plain
from test_compare_host import SETS, _pairs


@pytest.fixture(scope="module")
def H():
    import homomorph
    homomorph.lib()
    return homomorph


def test_bounds_at_u32_d256(H):
    D = np.full(32, 256, np.uint32)
    mb = H.minmax_out_bounds(D, D)
    assert mb.tolist() == [8704] * 32
    assert H.caps(mb).tolist() == [137] * 32
    assert H.batch_stride(mb) == 4384  # 35 072 B per value
    # a condition out of `<` gives the same bounds through the select entry
    lt = H.compare_out_bounds(H.HomomorphicLessThan, D, D)
    assert np.array_equal(H.select_out_bounds(lt[0], D, D), mb)
    assert H.select_out_bounds(256, D, D).tolist() == [512] * 32  # a fresh condition


@pytest.mark.parametrize("nbits", [1, 8, 16, 64, 128])
def test_bounds_equal_the_recurrences(H, nbits):
    rng = np.random.default_rng(nbits)
    uniform = np.full(nbits, 192, np.uint32)
    skew_a = (192 + 37 * np.arange(nbits)).astype(np.uint32)
    skew_b = rng.integers(0, 700, size=nbits).astype(np.uint32)
    for ba, bb in ((uniform, uniform), (skew_a, uniform), (skew_a, skew_b), (skew_b, skew_a)):
        assert np.array_equal(H.minmax_out_bounds(ba, bb), sm.minmax_bounds(ba, bb))
        for cb in (0, 192, int(bm.compare_bounds("lt", ba, bb)[0])):
            assert np.array_equal(H.select_out_bounds(cb, ba, bb), sm.select_bounds(cb, ba, bb))


def test_bounds_reject_bad_arguments(H):
    from homomorph import _lib
    L = _lib.lib()
    a = np.full(128, 10, np.uint32)
    out = np.zeros(128, np.uint32)
    p = lambda x: x.ctypes.data_as(_lib.u32p)  # noqa: E731
    for nbits in (0, 129):
        assert L.hm_select_out_bounds(nbits, 10, p(a), p(a), p(out)) == _lib.ERR_INVALID_ARGUMENT
        assert L.hm_minmax_out_bounds(nbits, p(a), p(a), p(out)) == _lib.ERR_INVALID_ARGUMENT
    assert L.hm_select_out_bounds(128, 10, p(a), p(a), p(out)) == _lib.OK
    assert L.hm_minmax_out_bounds(128, p(a), p(a), p(out)) == _lib.OK
    # beyond the engine's degree range, as hm_sub_out_bounds reports it
    big = np.full(128, 1 << 29, np.uint32)
    assert L.hm_minmax_out_bounds(128, p(big), p(big), p(out)) == _lib.ERR_UNSUPPORTED
    assert L.hm_select_out_bounds(128, 1 << 29, p(big), p(big), p(out)) == _lib.ERR_UNSUPPORTED
    # the comparison entry does not know the new codes
    for code in (_lib.OP_SELECT, _lib.OP_MIN, _lib.OP_MAX):
        assert L.hm_compare_out_bounds(code, 4, p(a), p(a), p(out)) == _lib.ERR_INVALID_ARGUMENT


def test_requirement_numbers(H):
    from homomorph import _lib
    assert (_lib.OP_SELECT, _lib.OP_MIN, _lib.OP_MAX) == (14, 15, 16)
    assert H.HomomorphicSelect.MIN_D_OVER_DELTA == 5
    for op in (H.HomomorphicMin, H.HomomorphicMax):
        assert [op.min_d_over_delta(n) for n in (8, 16, 32, 64)] == [21, 37, 69, 133]
    # hm_validate_operation has no width.  (A context needs a device: without one only the
    # refusal can be seen here; tests/test_gpu_select.py reads the engine's numbers.)
    L = _lib.lib()
    req = ctypes.c_uint16()
    for code in (_lib.OP_MIN, _lib.OP_MAX):
        assert L.hm_validate_operation(None, code, ctypes.byref(req)) == _lib.ERR_INVALID_ARGUMENT


def check_model(oracle, model, params, udt, sdt, n=5, key_seed=31):
    """select, min and max of the model on fresh ciphertexts of _pairs (random, equal, off by
    one, max against 0): decryption against numpy, degrees against the bounds, and min / max
    against the select of the `<` polynomial."""
    d, dp, delta, tau = params
    nbits = 8 * np.dtype(udt).itemsize
    sk, pk, _ = keys(d, dp, delta, tau, key_seed)
    s = model.limbs_to_int(sk)
    bound = np.full(nbits, d + dp, np.uint32)
    a, b = _pairs(n, udt, 7)
    cv = np.array([1, 0, 1, 0, 1][:n], np.uint8)
    cbound = np.full(8, d + dp, np.uint32)
    la, da = oracle.encrypt_batch(pk, as_bytes(a), masks(n, nbits, tau, 3), bound)
    lb, db = oracle.encrypt_batch(pk, as_bytes(b), masks(n, nbits, tau, 4), bound)
    lc, dc = oracle.encrypt_batch(pk, as_bytes(cv), masks(n, 8, tau, 5), cbound)
    mb = sm.minmax_bounds(bound, bound)
    sb = sm.select_bounds(d + dp, bound, bound)
    for e in range(n):
        A, B = bit_ints(la, da, bound, e), bit_ints(lb, db, bound, e)
        c = bit_ints(lc, dc, cbound, e)[0]
        out = sm.select_circuit(c, A, B)
        assert all(model.degree(p) <= int(sb[i]) for i, p in enumerate(out))
        assert bm.decrypt_value(out, s) == int(np.where(cv[e], a[e], b[e])), (e, a[e], b[e])
        # the unit and the null condition return the operands themselves
        assert sm.select_circuit(1, A, B) == A and sm.select_circuit(0, A, B) == B
        for signed, dt in ((False, udt), (True, sdt)):
            x, y = a.view(dt)[e], b.view(dt)[e]
            lt = sm.less_than(A, B, signed)
            assert lt == bm.compare_circuit("lt", A, B, signed)
            lo, hi = sm.min_circuit(A, B, signed), sm.max_circuit(A, B, signed)
            assert lo == sm.select_circuit(lt, A, B)
            assert hi == sm.select_circuit(lt, B, A)
            for got, want in ((lo, np.minimum(x, y)), (hi, np.maximum(x, y))):
                assert all(model.degree(p) <= int(mb[i]) for i, p in enumerate(got))
                assert bm.decrypt_value(got, s) == int(np.array(want, dt).view(udt)), (signed, x, y)
        # a value against itself: x_i = 0, every output bit is the input bit
        assert sm.min_circuit(A, A) == A and sm.max_circuit(A, A, True) == A


@pytest.mark.parametrize("params,udt,sdt", SETS)
def test_model_circuits_decrypt_to_numpy(oracle, model, params, udt, sdt):
    check_model(oracle, model, params, udt, sdt)


def test_model_at_the_u8_requirement_edge(oracle, model):
    """u8 min needs d >= 21 delta: (63,64,3,64) is the smallest d that qualifies at delta = 3
    (m (delta + 1) = 40 < 63); the GPU test of the requirement relies on it."""
    check_model(oracle, model, (63, 64, 3, 64), np.uint8, np.int8)
