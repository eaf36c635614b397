"""CPU checks of the shifts and rotates by an encrypted amount: the model circuit
(tests/shift_model.py) against numpy's <<, >> and rotates after decryption, with its degrees
against the bounds and both stage orders against each other; the host-only bounds entry point
against the model's rule; the requirement numbers; and the planner header compiled alone into an
ASan + UBSan driver (tests/sanitize/shift_plan.cpp) whose bounds, source map and layout are
compared with the model.  No GPU, no launch.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import borrow_model as bm
import shift_model as sm
from helpers import as_bytes, bit_ints, keys, masks, plain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRESH = 192


@pytest.fixture(scope="module")
def H():
    import homomorph
    homomorph.lib()
    return homomorph


def markers(H):
    return {"shl": H.HomomorphicShiftLeft, "shr": H.HomomorphicShiftRight,
            "rotl": H.HomomorphicRotateLeft, "rotr": H.HomomorphicRotateRight}


def input_bounds(n):
    """(a's bounds, the amount's bounds): uniform, and skewed (fresh + 37 i, fresh + 11 t)."""
    L = sm.stages(n)
    return [(np.full(n, FRESH, np.uint32), np.full(L, FRESH, np.uint32)),
            ((FRESH + 37 * np.arange(n)).astype(np.uint32),
             (FRESH + 11 * np.arange(L)).astype(np.uint32))]


# ------------------------------------------------------------------ the model circuit
@pytest.mark.parametrize("params,dtype", [((9, 8, 1, 8), np.uint8), ((13, 8, 1, 8), np.uint32),
                                          ((27, 16, 3, 16), np.uint8),
                                          ((128, 128, 1, 128), np.uint32)])
def test_model_decrypts_to_numpy(H, oracle, model, params, dtype):
    """Fresh ciphertexts at the edge of the requirement the marker classes state,
    d = (2L + 3) delta (and the headline parameters): every mode decrypts to numpy's result,
    degrees stay within shift_bounds, and ascending and descending stage order give equal
    polynomials.  On plaintext amounts (unit and null amount bits) the circuit renumbers a's
    polynomials."""
    d, dp, delta, tau = params
    n = 8 * np.dtype(dtype).itemsize
    L = sm.stages(n)
    for marker in markers(H).values():
        assert marker.min_d_over_delta(n) == 2 * L + 3 and d >= (2 * L + 3) * delta
    moves_the_bits_on_trivial_amounts()
    sk, pk, _ = keys(d, dp, delta, tau, 41)
    s = model.limbs_to_int(sk)
    top = np.iinfo(dtype).max
    av = np.concatenate([np.array([top, 1 << (n - 1), 1], dtype), plain(2, dtype, 5)])
    sv = np.array([0, n - 1, n, 255, int(plain(1, np.uint8, 6)[0])], np.uint8)
    nv = len(av)
    ab, sb = np.full(n, d + dp, np.uint32), np.full(8, d + dp, np.uint32)
    la, da = oracle.encrypt_batch(pk, as_bytes(av), masks(nv, n, tau, 7), ab)
    ls, ds = oracle.encrypt_batch(pk, as_bytes(sv), masks(nv, 8, tau, 8), sb)
    for op, signed in sm.MODES:
        ob = sm.shift_bounds(op, ab, sb)
        want = sm.numpy_shift(op, av, sv, signed)
        for e in range(nv):
            A, S = bit_ints(la, da, ab, e), bit_ints(ls, ds, sb, e)
            out = sm.shift_circuit(op, A, S, signed)
            assert len(out) == n
            assert all(model.degree(p) <= int(ob[j]) for j, p in enumerate(out)), (op, signed, e)
            assert bm.decrypt_value(out, s) == int(want[e]), (op, signed, e, av[e], sv[e])
            assert out == sm.shift_circuit(op, A, S, signed, order=range(L - 1, -1, -1))
            assert sm.int_shift(op, int(av[e]), int(sv[e]), n, signed) == int(want[e])


def moves_the_bits_on_trivial_amounts():
    """Unit and null amount bits (plaintext amounts): the output is a's polynomials renumbered."""
    a = [3 + 2 * i for i in range(8)]  # any distinct polynomials
    for k in range(8):
        s = [(k >> t) & 1 for t in range(3)]
        assert sm.shift_circuit("shl", a, s) == [0] * k + a[:8 - k]
        assert sm.shift_circuit("shr", a, s) == a[k:] + [0] * k
        assert sm.shift_circuit("shr", a, s, signed=True) == a[k:] + [a[7]] * k
        assert sm.shift_circuit("rotl", a, s) == a[8 - k:] + a[:8 - k]
        assert sm.shift_circuit("rotr", a, s) == a[k:] + a[:k]


# ------------------------------------------------------------------ the bounds entry point
@pytest.mark.parametrize("n", [8, 16, 32, 64, 128])
def test_bounds_equal_the_model(H, n):
    L = sm.stages(n)
    for ab, sb in input_bounds(n):
        for op, marker in markers(H).items():
            got = H.shift_out_bounds(marker, ab, sb)
            assert got.dtype == np.uint32 and got.size == n
            assert np.array_equal(got, sm.shift_bounds(op, ab, sb)), (op, ab)
            # a wider amount: only its low L bounds are read
            wide = np.concatenate([sb, np.full(8, 99999, np.uint32)])
            assert np.array_equal(H.shift_out_bounds(marker, ab, wide), got)
        S = int(sb.sum())
        shl = H.shift_out_bounds(H.HomomorphicShiftLeft, ab, sb)
        shr = H.shift_out_bounds(H.HomomorphicShiftRight, ab, sb)
        rot = H.shift_out_bounds(H.HomomorphicRotateLeft, ab, sb)
        assert shl[0] == S + ab[0] and shl[n - 1] == S + ab.max()
        assert shr[n - 1] == S + ab[n - 1] and shr[0] == S + ab.max()
        assert (rot == S + ab.max()).all()
        if ab[0] != ab[n - 1]:
            assert not np.array_equal(shl, shr)
    # the headline shape: a u32 at D = 256 has every bit at 6 D, 25 limbs, 800 limbs per value
    D = np.full(32, 256, np.uint32)
    b = H.shift_out_bounds(H.HomomorphicShiftLeft, D, D[:5])
    assert (b == 1536).all() and H.batch_stride(b) == 800


def test_bounds_reject_bad_arguments(H):
    from homomorph import _lib
    L = _lib.lib()
    a = np.full(256, 10, np.uint32)
    s = np.full(8, 10, np.uint32)
    out = np.zeros(256, np.uint32)
    p32 = lambda x: x.ctypes.data_as(_lib.u32p)  # noqa: E731
    for which in (_lib.OP_SHL, _lib.OP_SHR, _lib.OP_ROTL, _lib.OP_ROTR):
        for nbits in (2, 8, 32, 128):
            assert L.hm_shift_out_bounds(which, nbits, p32(a), p32(s), p32(out)) == _lib.OK
        for nbits in (0, 1, 24, 256):
            assert (L.hm_shift_out_bounds(which, nbits, p32(a), p32(s), p32(out))
                    == _lib.ERR_INVALID_ARGUMENT)
    for which in (_lib.OP_LOOKUP, _lib.OP_SELECT, _lib.OP_ADD, 22):
        assert L.hm_shift_out_bounds(which, 8, p32(a), p32(s), p32(out)) == _lib.ERR_INVALID_ARGUMENT
    assert L.hm_shift_out_bounds(_lib.OP_SHL, 8, None, p32(s), p32(out)) == _lib.ERR_INVALID_ARGUMENT
    assert L.hm_shift_out_bounds(_lib.OP_SHL, 8, p32(a), None, p32(out)) == _lib.ERR_INVALID_ARGUMENT
    assert L.hm_shift_out_bounds(_lib.OP_SHL, 8, p32(a), p32(s), None) == _lib.ERR_INVALID_ARGUMENT
    # beyond the engine's degree range, as hm_sub_out_bounds reports it
    big = np.full(8, 1 << 29, np.uint32)
    assert L.hm_shift_out_bounds(_lib.OP_ROTL, 8, p32(big), p32(big), p32(out)) == _lib.ERR_UNSUPPORTED
    assert L.hm_sub_out_bounds(8, p32(big), p32(big), p32(out)) == _lib.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        H.shift_out_bounds(H.HomomorphicShiftLeft, a[:32], s[:4])  # five amount bits are read
    with pytest.raises(H.EngineError) as ei:
        H.shift_out_bounds(H.HomomorphicShiftLeft, a[:24], s)
    assert ei.value.status == _lib.ERR_INVALID_ARGUMENT


def test_requirement_numbers(H):
    from homomorph import _lib
    L = _lib.lib()
    assert (_lib.OP_SHL, _lib.OP_SHR, _lib.OP_ROTL, _lib.OP_ROTR) == (18, 19, 20, 21)
    assert L.hm_abi_version() >= 9
    for marker in markers(H).values():
        assert [marker.min_d_over_delta(n) for n in (8, 16, 32, 64, 128)] == [9, 11, 13, 15, 17]
        assert marker.min_d_over_delta(2) == 5
        for bad in (0, 1, 24, 256):
            with pytest.raises(ValueError):
                marker.min_d_over_delta(bad)
    assert [m.CODE for m in markers(H).values()] == [18, 19, 20, 21]
    # hm_validate_operation has no width.  (A context needs a device: without one only the
    # refusal can be seen here; tests/test_gpu_shift.py reads the engine's numbers.)
    req = ctypes.c_uint16()
    assert L.hm_validate_operation(None, _lib.OP_SHL, ctypes.byref(req)) == _lib.ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------ the planner, stand-alone
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shift_plan") / "shift_plan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "sanitize", "shift_plan.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    return exe


CODES = {"shl": 18, "shr": 19, "rotl": 20, "rotr": 21}


def case_line(op, signed, ab, sb):
    return " ".join(str(int(x)) for x in [CODES[op], int(signed), len(ab), *ab, *sb])


def test_planner_under_asan_ubsan(driver):
    """Bounds and source map of the stand-alone planner against the model, over stdin and over
    arguments; the layout is ordered, every slot holds its bound and the slice is within the LDS
    rule; the driver's own last case, a u32 at bound 20 000, does not fit."""
    from homomorph import _lib
    cases = []
    for n in (2, 8, 16, 32, 64, 128):
        # (skewed bounds up to u32: fresh + 37 * 63 on a u64 is beyond a wave's share of LDS)
        for ab, sb in (input_bounds(n) if 2 < n <= 32 else input_bounds(n)[:1]):
            if n == 128:  # (the GPU test's u128: a fresh bound of 32)
                ab, sb = ab - (FRESH - 32), sb - (FRESH - 32)
            for op, signed in sm.MODES:
                cases.append((op, signed, ab, sb))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver], input="\n".join(case_line(*c) for c in cases) + "\n",
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines()]
    assert len(lines) == len(cases) + 1
    for (op, signed, ab, sb), got in zip(cases, lines):
        n, L = len(ab), len(sb)
        assert got["status"] == 0 and got["nbits"] == n and got["L"] == L, (op, n, got["status"])
        assert got["which"] == CODES[op]
        assert got["bounds"] == sm.shift_bounds(op, ab, sb).tolist()
        want_src = [[sm.source(op, n, 1 << t, i, signed) for i in range(n)] for t in range(L)]
        assert got["src"] == [[-1 if j is None else j for j in row] for row in want_src]
        # the slice: word counts | amount bits | x_i + x_src | one-bit buffer | saved bits | value
        assert got["oN"] == 0 and got["soff"][0] >= n + 8 + n // 2
        ends = [got["soff"][t] + 2 * (int(sb[t]) // 64 + 1) for t in range(L)]
        assert got["soff"] == sorted(got["soff"]) and got["soff"][1:] == ends[:-1]
        assert ends[-1] <= got["oX"] < got["oT"] < got["oS"] <= got["oV"]
        assert got["oV"] + got["cV"] == got["lds_per_wave"]
        assert got["lds_per_wave"] * 16 <= 160 * 1024
        # every slot holds a product at its bound (two factors' words) and its input bit's limbs
        off = got["off"] + [got["cV"]]
        assert off[0] == 0 and off == sorted(off)
        widest = 0
        for i in range(n):
            slot = off[i + 1] - off[i]
            assert slot >= got["bounds"][i] // 32 + 2 and slot >= 2 * (int(ab[i]) // 64 + 1)
            widest = max(widest, slot)
        assert got["oT"] - got["oX"] >= widest and got["oS"] - got["oT"] >= widest
        # a rotate's stage t saves 2^t bits at its input's bound: the stages above t have run
        if op in ("rotl", "rotr"):
            for t in range(L):
                inb = int(sb[t + 1:].sum()) + int(ab.max())
                assert got["sv"][t] >= inb // 32 + 1
                assert got["oV"] - got["oS"] >= (1 << t) * got["sv"][t]
        else:
            assert got["oS"] == got["oV"] and not any(got["sv"])
    # the shapes that must run: every width 8..64 at D = 256, u32 at D = 512; in place u128 at
    # D = 256 fits too (one block a CU), and the headline u32 is about 2 000 words a wave
    for n, D, lo, hi in ((8, 256, 0, 600), (16, 256, 0, 1200), (32, 256, 1800, 2100),
                         (64, 256, 0, 5000), (32, 512, 0, 4000), (128, 256, 0, 160 * 1024 // 16)):
        b = np.full(n, D, np.uint32)
        r = subprocess.run([driver] + case_line("rotl", False, b, b[:sm.stages(n)]).split(),
                           capture_output=True, text=True, timeout=60, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        one, big = [json.loads(x) for x in r.stdout.splitlines()]
        assert one["status"] == 0 and lo <= one["lds_per_wave"] <= hi, (n, D, one["lds_per_wave"])
    assert big["status"] == _lib.ERR_UNSUPPORTED and big["bounds"] == [120000] * 32
    # a u128 at D = 512 does not fit
    b = np.full(128, 512, np.uint32)
    r = subprocess.run([driver], input=case_line("shl", False, b, b[:7]) + "\n",
                       capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and json.loads(r.stdout.splitlines()[0])["status"] == _lib.ERR_UNSUPPORTED
    # a malformed case is refused: a width that is no power of two, a missing amount bound
    for bad in (["18", "0", "24"] + ["10"] * 28, ["18", "0", "8"] + ["10"] * 10,
                ["17", "0", "8"] + ["10"] * 11):
        r = subprocess.run([driver] + bad, capture_output=True, text=True, env=env)
        assert r.returncode == 2
