"""CPU checks of the table lookup: the host-only bounds entry point against the
model's rule (tests/lookup_model.py), the model circuit against table[v] after decryption (with its
degrees against the bounds), the requirement numbers, and the planner header compiled alone into
an ASan + UBSan driver (tests/sanitize/lookup_plan.cpp) whose masks and bounds are compared with
the model.  No GPU, no launch.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import borrow_model as bm
import lookup_model as lm
from helpers import as_bytes, bit_ints, keys, masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRESH = 192


@pytest.fixture(scope="module")
def H():
    import homomorph
    homomorph.lib()
    return homomorph


def tables(k, dtype, seed=0):
    """The structured tables of the issue over k index bits, as (name, table)."""
    n = 1 << k
    v = np.arange(n)
    info = np.iinfo(dtype)
    rng = np.random.default_rng(1000 * k + seed)
    pop = np.array([bin(x).count("1") for x in v])
    return [
        ("random", rng.integers(info.min, info.max, size=n, dtype=dtype, endpoint=True)),
        ("identity", v.astype(dtype)),
        ("constant", np.full(n, 0xA5 & info.max, dtype)),
        ("parity", (pop & 1).astype(dtype)),
        ("all ones", (v == n - 1).astype(dtype)),
    ]


def input_bounds(k):
    return [np.full(k, FRESH, np.uint32), (FRESH + 37 * np.arange(k)).astype(np.uint32)]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32])
@pytest.mark.parametrize("k", [1, 3, 5, 8])
def test_bounds_equal_the_model(H, k, dtype):
    for ab in input_bounds(k):
        for name, t in tables(k, dtype):
            got = H.lookup_out_bounds(ab, t)
            assert got.size == 8 * np.dtype(dtype).itemsize
            assert np.array_equal(got, lm.lookup_bounds(ab, t)), (name, ab)
            if name == "identity":
                assert np.array_equal(got[:k], ab) and not got[k:].any()
            if name == "constant":
                assert not got.any()
            if name == "parity":
                assert got[0] == ab.max() and not got[1:].any()
            if name == "all ones":
                assert got[0] == ab.sum() and not got[1:].any()


def test_a_random_byte_table_has_bounds_7d_or_8d(H):
    D = np.full(8, 256, np.uint32)
    t = tables(8, np.uint8)[0][1]
    c = lm.coefficient_masks(t)
    want = [2048 if (m >> 255) & 1 else 1792 for m in c]
    assert H.lookup_out_bounds(D, t).tolist() == want
    # in_bits reads the low bounds of a wider value
    wide = np.concatenate([D, np.full(24, 999, np.uint32)])
    assert H.lookup_out_bounds(wide, t, in_bits=8).tolist() == want


def test_bounds_reject_bad_arguments(H):
    from homomorph import _lib
    L = _lib.lib()
    a = np.full(8, 10, np.uint32)
    t = np.zeros(4 * 256, np.uint8)
    out = np.zeros(32, np.uint32)
    p32 = lambda x: x.ctypes.data_as(_lib.u32p)  # noqa: E731
    p8 = t.ctypes.data_as(_lib.u8p)
    assert L.hm_lookup_out_bounds(8, p32(a), p8, 4, p32(out)) == _lib.OK
    for k in (0, 9):
        assert L.hm_lookup_out_bounds(k, p32(a), p8, 1, p32(out)) == _lib.ERR_INVALID_ARGUMENT
    for nbytes in (0, 3, 8):
        assert L.hm_lookup_out_bounds(8, p32(a), p8, nbytes, p32(out)) == _lib.ERR_INVALID_ARGUMENT
    assert L.hm_lookup_out_bounds(8, None, p8, 1, p32(out)) == _lib.ERR_INVALID_ARGUMENT
    assert L.hm_lookup_out_bounds(8, p32(a), None, 1, p32(out)) == _lib.ERR_INVALID_ARGUMENT
    assert L.hm_lookup_out_bounds(8, p32(a), p8, 1, None) == _lib.ERR_INVALID_ARGUMENT
    # beyond the engine's degree range, as hm_sub_out_bounds reports it
    big = np.full(8, 1 << 28, np.uint32)
    ones = (np.arange(256) == 255).astype(np.uint8)
    assert (L.hm_lookup_out_bounds(8, p32(big), ones.ctypes.data_as(_lib.u8p), 1, p32(out))
            == _lib.ERR_UNSUPPORTED)
    # ... which a table that never multiplies does not reach
    ident = np.arange(256, dtype=np.uint8)
    assert (L.hm_lookup_out_bounds(8, p32(big), ident.ctypes.data_as(_lib.u8p), 1, p32(out))
            == _lib.OK)
    with pytest.raises(ValueError):
        H.lookup_out_bounds(a, np.zeros(100, np.uint8))
    with pytest.raises(ValueError):
        H.lookup_out_bounds(a, np.zeros(256, np.uint64))


def test_requirement_numbers(H):
    from homomorph import _lib
    L = _lib.lib()
    assert _lib.OP_LOOKUP == 17
    assert L.hm_abi_version() >= 8
    assert H.HomomorphicLookup.min_d_over_delta(8) == 17
    assert [H.HomomorphicLookup.min_d_over_delta(n) for n in (1, 4)] == [3, 9]
    # hm_validate_operation has no width.  (A context needs a device: without one only the
    # refusal can be seen here; tests/test_gpu_lookup.py reads the engine's numbers.)
    req = ctypes.c_uint16()
    assert L.hm_validate_operation(None, _lib.OP_LOOKUP, ctypes.byref(req)) == _lib.ERR_INVALID_ARGUMENT


def test_moebius_is_an_involution_and_evaluates_to_the_table():
    """The model's own footing: evaluating the algebraic normal form at plaintext bits gives the
    table back."""
    t = tables(5, np.uint16)[0][1]
    c = lm.moebius(t)
    for v in range(32):
        got = 0
        for j, f in enumerate(c):
            bit = 0
            for S, cs in enumerate(f):
                if cs and (S & v) == S:
                    bit ^= 1
            got |= bit << j
        assert got == int(t[v])


VALUES = np.array([0, 1, 255, 128, 0x5A, 77], np.uint8)


@pytest.mark.parametrize("params", [(64, 64, 1, 64), (128, 128, 1, 128), (17, 8, 1, 8),
                                    (51, 16, 3, 16)])
def test_model_decrypts_to_the_table(oracle, model, params):
    """A random 256-entry u16 table on fresh ciphertexts: decryption gives table[v], degrees stay
    within the bounds.  (17,8,1,8) is the requirement's edge: d = 17 delta."""
    d, dp, delta, tau = params
    assert d >= 17 * delta
    sk, pk, _ = keys(d, dp, delta, tau, 31)
    s = model.limbs_to_int(sk)
    bound = np.full(8, d + dp, np.uint32)
    t = tables(8, np.uint16, seed=7)[0][1]
    n = len(VALUES)
    la, da = oracle.encrypt_batch(pk, as_bytes(VALUES), masks(n, 8, tau, 3), bound)
    ob = lm.lookup_bounds(bound, t)
    for e in range(n):
        out = lm.lookup_circuit(bit_ints(la, da, bound, e), t)
        assert len(out) == 16
        assert all(model.degree(p) <= int(ob[j]) for j, p in enumerate(out))
        assert bm.decrypt_value(out, s) == int(t[VALUES[e]]), (e, VALUES[e])


# ------------------------------------------------------------------ the planner, stand-alone
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lookup_plan") / "lookup_plan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "sanitize", "lookup_plan.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    return exe


def case_line(ab, t):
    raw = as_bytes(np.asarray(t)) if np.asarray(t).dtype != np.bool_ else np.asarray(t, np.uint8)
    return " ".join([str(len(ab)), str(np.asarray(t).dtype.itemsize)] + [str(int(x)) for x in ab]
                    + [raw.tobytes().hex()])


def test_planner_under_asan_ubsan(driver):
    """Masks and bounds of the stand-alone planner against the model, over stdin and over
    arguments; the layout is ordered and within the LDS rule; the driver's own last case, a byte
    index at bound 20 000, does not fit."""
    cases = []
    for k, dtype in ((1, np.uint8), (3, np.uint16), (5, np.uint32), (8, np.uint8), (8, np.uint32)):
        for ab in input_bounds(k):
            for name, t in tables(k, dtype):
                cases.append((ab, t))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver], input="\n".join(case_line(ab, t) for ab, t in cases) + "\n",
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines()]
    assert len(lines) == len(cases) + 1
    for (ab, t), got in zip(cases, lines):
        k = len(ab)
        assert got["status"] == 0 and got["in_bits"] == k
        assert [int(m, 16) for m in got["masks"]] == lm.coefficient_masks(t)
        assert got["bounds"] == lm.lookup_bounds(ab, t).tolist()
        assert (got["kl"], got["kh"]) == ((k + 1) // 2, k // 2)
        # the slice: word counts | unit | monomials | inner sum | two accumulators
        offs = [got["off"][s] for s in range(1, 1 << got["kl"])]
        offs += [got["off"][16 + s] for s in range(1, 1 << got["kh"])]
        assert got["oN"] == 0 and got["off"][0] == got["off"][16] == 32
        assert offs == sorted(offs) and offs[0] >= 34 and offs[-1] < got["oI"]
        assert got["oI"] + got["cI"] <= got["oP"]
        assert got["oP"] + 2 * got["cP"] == got["lds_per_wave"]
        assert got["lds_per_wave"] * 16 <= 160 * 1024
        # an accumulator holds the widest output, an inner sum the widest low monomial
        assert 32 * got["cP"] > max(got["bounds"])
        assert 32 * got["cI"] > sum(int(x) for x in ab[:got["kl"]])
    # the headline shape: a byte at D = 256 is about 800 words per wave
    D = np.full(8, 256, np.uint32)
    r = subprocess.run([driver] + case_line(D, tables(8, np.uint8)[0][1]).split(),
                       capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    one, big = [json.loads(x) for x in r.stdout.splitlines()]
    assert one["status"] == 0 and 600 <= one["lds_per_wave"] <= 900
    assert one["need"] == 0xFFFFFFFF  # every monomial of both halves
    from homomorph import _lib
    assert big["status"] == _lib.ERR_UNSUPPORTED and big["bounds"] == [160000] + [0] * 7
    # a malformed case is refused
    r = subprocess.run([driver, "8", "1", "1", "2"], capture_output=True, text=True, env=env)
    assert r.returncode == 2
