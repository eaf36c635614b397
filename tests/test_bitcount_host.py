"""CPU checks of the bit counts: the model circuits (tests/bitcount_model.py)
against int.bit_count and bit scans, on 0 / 1 values and after decryption, against the lookup
model for a byte, and their degrees against the bounds; the host-only bounds entry point against
the model's rule; the requirement numbers; and the planner header compiled alone into an
ASan + UBSan driver (tests/sanitize/bitcount_plan.cpp) whose bounds, needed set and layout are
compared with the model and with a brute-force reachability computation.  No GPU, no launch.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import bitcount_model as bcm
import borrow_model as bm
import lookup_model as lm
from helpers import as_bytes, bit_ints, keys, masks, plain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRESH = 192
WIDTHS = (1, 3, 8, 24, 32, 64, 128)


@pytest.fixture(scope="module")
def H():
    import homomorph
    homomorph.lib()
    return homomorph


def markers(H):
    return {"count_ones": H.HomomorphicCountOnes, "count_zeros": H.HomomorphicCountZeros,
            "leading_zeros": H.HomomorphicLeadingZeros, "leading_ones": H.HomomorphicLeadingOnes,
            "trailing_zeros": H.HomomorphicTrailingZeros,
            "trailing_ones": H.HomomorphicTrailingOnes}


def input_bounds(n):
    """Uniform; skewed (fresh + 37 i); skewed the other way; with zeros (null bit positions)."""
    i = np.arange(n)
    holes = np.where(i % 3 == 1, 0, FRESH + 5 * i)
    return [np.full(n, FRESH, np.uint32), (FRESH + 37 * i).astype(np.uint32),
            (FRESH + 37 * i[::-1]).astype(np.uint32), holes.astype(np.uint32)]


# ------------------------------------------------------------------ the model circuits
@pytest.mark.parametrize("n", [1, 3, 8, 24, 32, 64])
def test_model_on_plain_bits_is_the_integer_count(n):
    """On 0 / 1 polynomials the 8 output polynomials are the bits of the integer result."""
    rng = np.random.default_rng(n)
    full = (1 << n) - 1
    values = [0, full, 1, 1 << (n - 1), full ^ 1, full >> 1]
    values += [int.from_bytes(rng.bytes(16), "little") & full for _ in range(6)]
    for x in values:
        bits = [(x >> i) & 1 for i in range(n)]
        for op in bcm.OPS:
            out = bcm.circuit(op, bits)
            assert len(out) == 8 and all(p in (0, 1) for p in out)
            assert sum(p << k for k, p in enumerate(out)) == bcm.int_count(op, x, n), (op, n, x)
    assert bcm.int_count("count_ones", full, n) == n == bcm.int_count("leading_ones", full, n)
    assert bcm.int_count("trailing_zeros", 0, n) == n == bcm.int_count("count_zeros", 0, n)


@pytest.mark.parametrize("params,dtype", [((17, 8, 1, 8), np.uint8), ((33, 8, 1, 8), np.uint16)])
def test_model_decrypts_to_the_integer_count(H, oracle, model, params, dtype):
    """Fresh ciphertexts at the edge of the requirement the marker classes state, d = (2n + 1)
    delta: every op decrypts to the integer result and its degrees stay within the bounds."""
    d, dp, delta, tau = params
    n = 8 * np.dtype(dtype).itemsize
    for marker in markers(H).values():
        assert marker.min_d_over_delta(n) == 2 * n + 1 and d >= (2 * n + 1) * delta
    sk, pk, _ = keys(d, dp, delta, tau, 43)
    s = model.limbs_to_int(sk)
    top = np.iinfo(dtype).max
    av = np.concatenate([np.array([0, top, 1 << (n - 1), 1], dtype), plain(2, dtype, 6)])
    ab = np.full(n, d + dp, np.uint32)
    la, da = oracle.encrypt_batch(pk, as_bytes(av), masks(len(av), n, tau, 9), ab)
    for op in bcm.OPS:
        ob = bcm.bitcount_bounds(op, ab)
        for e in range(len(av)):
            out = bcm.circuit(op, bit_ints(la, da, ab, e))
            assert all(model.degree(p) <= int(ob[k]) for k, p in enumerate(out)), (op, e)
            assert bm.decrypt_value(out, s) == bcm.int_count(op, int(av[e]), n), (op, e, av[e])


def test_model_of_a_byte_is_the_lookup_model():
    """The multilinear form of a function of 8 bits is unique: the count circuits and the table
    lookup's algebraic normal form are the same polynomials."""
    rng = np.random.default_rng(7)
    a = [int.from_bytes(rng.bytes(3), "little") | 1 for _ in range(8)]
    a[5] = 1  # a unit polynomial among them
    for op in bcm.OPS:
        assert bcm.circuit(op, a) == lm.lookup_circuit(a, bcm.table(op)), op


# ------------------------------------------------------------------ the bounds entry point
@pytest.mark.parametrize("n", WIDTHS)
def test_bounds_equal_the_model(H, n):
    for ab in input_bounds(n):
        got = {}
        for op, marker in markers(H).items():
            got[op] = H.bitcount_out_bounds(marker, ab)
            assert got[op].dtype == np.uint32 and got[op].size == 8
            assert np.array_equal(got[op], bcm.bitcount_bounds(op, ab)), (op, n, ab)
            assert not got[op][int(n).bit_length():].any()  # 2^k > n: null
        assert np.array_equal(got["count_ones"], got["count_zeros"])
        assert np.array_equal(got["leading_ones"], got["leading_zeros"])
        assert got["count_ones"][0] == ab.max()
        assert got["leading_ones"][0] == got["trailing_ones"][0] == ab.sum()
    # skewed: a count takes the 2^k LARGEST, and the two ends of a run differ
    if n >= 3:
        skew = input_bounds(n)[1]
        k = int(n).bit_length() - 2
        c = H.bitcount_out_bounds(H.HomomorphicCountOnes, skew)
        assert c[k] == np.sort(skew)[::-1][:1 << k].sum() != skew[:1 << k].sum()
        lead = H.bitcount_out_bounds(H.HomomorphicLeadingZeros, skew)
        trail = H.bitcount_out_bounds(H.HomomorphicTrailingZeros, skew)
        # (at a power of two every M is n itself: both ends sum all the bounds)
        assert np.array_equal(lead, trail) == (n & (n - 1) == 0)
    # the headline shape: a u32 at D = 256
    D = np.full(32, 256, np.uint32)
    c = H.bitcount_out_bounds(H.HomomorphicCountOnes, D)
    r = H.bitcount_out_bounds(H.HomomorphicLeadingZeros, D)
    assert c.tolist() == [256, 512, 1024, 2048, 4096, 8192, 0, 0] and H.batch_stride(c) == 260
    assert r.tolist() == [8192] * 6 + [0, 0] and H.batch_stride(r) == 776


def test_bounds_reject_bad_arguments(H):
    from homomorph import _lib
    L = _lib.lib()
    a = np.full(256, 10, np.uint32)
    out = np.zeros(8, np.uint32)
    p32 = lambda x: x.ctypes.data_as(_lib.u32p)  # noqa: E731
    codes = list(range(22, 28))
    assert [_lib.OP_COUNT_ONES, _lib.OP_COUNT_ZEROS, _lib.OP_LEADING_ZEROS, _lib.OP_LEADING_ONES,
            _lib.OP_TRAILING_ZEROS, _lib.OP_TRAILING_ONES] == codes
    for which in codes:
        for nbits in (1, 3, 8, 24, 128):
            assert L.hm_bitcount_out_bounds(which, nbits, p32(a), p32(out)) == _lib.OK
        for nbits in (0, 129, 256):
            assert L.hm_bitcount_out_bounds(which, nbits, p32(a), p32(out)) == _lib.ERR_INVALID_ARGUMENT
        assert L.hm_bitcount_out_bounds(which, 8, None, p32(out)) == _lib.ERR_INVALID_ARGUMENT
        assert L.hm_bitcount_out_bounds(which, 8, p32(a), None) == _lib.ERR_INVALID_ARGUMENT
    for which in (_lib.OP_ROTR, _lib.OP_LOOKUP, _lib.OP_ADD, 28, -1):
        assert L.hm_bitcount_out_bounds(which, 8, p32(a), p32(out)) == _lib.ERR_INVALID_ARGUMENT
    # beyond the engine's degree range: one bound of 2^30, or a sum that reaches it
    big = a.copy()
    big[3] = 1 << 30
    half = np.full(8, 1 << 27, np.uint32)
    for which in codes:
        assert L.hm_bitcount_out_bounds(which, 8, p32(big), p32(out)) == _lib.ERR_UNSUPPORTED
        assert L.hm_bitcount_out_bounds(which, 8, p32(half), p32(out)) == _lib.ERR_UNSUPPORTED
    assert L.hm_bitcount_out_bounds(_lib.OP_COUNT_ONES, 7, p32(half), p32(out)) == _lib.OK
    with pytest.raises(H.EngineError) as ei:
        H.bitcount_out_bounds(H.HomomorphicShiftLeft, a[:8])
    assert ei.value.status == _lib.ERR_INVALID_ARGUMENT
    # the batch entry refuses null pointers and a which outside the six before it needs a device
    assert L.hm_bitcount_batch(None, _lib.OP_COUNT_ONES, None, None) == _lib.ERR_INVALID_ARGUMENT


def test_requirement_numbers(H):
    from homomorph import _lib
    L = _lib.lib()
    assert L.hm_abi_version() >= 10
    for op, marker in markers(H).items():
        assert marker.CODE == bcm.CODES[op]
        assert [marker.min_d_over_delta(n) for n in (8, 16, 32, 64)] == [17, 33, 65, 129]
        assert marker.min_d_over_delta(24) == (49 if bcm.OPS[op][0] else 33)
        assert marker.min_d_over_delta(1) == 3
        for n in WIDTHS:
            assert marker.min_d_over_delta(n) == 2 * bcm.degree_of(op, n) + 1
        for bad in (0, 129):
            with pytest.raises(ValueError):
                marker.min_d_over_delta(bad)
    # hm_validate_operation has no width.  (A context needs a device: without one only the
    # refusal can be seen here; tests/test_gpu_bitcount.py reads the engine's numbers.)
    req = ctypes.c_uint16()
    assert (L.hm_validate_operation(None, _lib.OP_COUNT_ONES, ctypes.byref(req))
            == _lib.ERR_INVALID_ARGUMENT)


# ------------------------------------------------------------------ the planner, stand-alone
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bitcount_plan") / "bitcount_plan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "sanitize", "bitcount_plan.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    return exe


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
           UBSAN_OPTIONS="print_stacktrace=1")


def case_line(op, ab):
    return " ".join(str(int(x)) for x in [bcm.CODES[op], len(ab), *ab])


def run_cases(driver, cases):
    r = subprocess.run([driver], input="\n".join(case_line(*c) for c in cases) + "\n",
                       capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines()]
    assert len(lines) == len(cases) + 1
    return lines


def reachable(n):
    """Brute force: the (i, j) from which the recurrence's dependency edges E_j^(i) -> E_j^(i+1)
    and E_j^(i) -> E_{j+1}^(i+1) reach a target (n, 2^k); only 1 <= j <= i can be non-null."""
    live = {(n, 1 << k) for k in range(8) if 1 << k <= n}
    for i in range(n - 1, 0, -1):
        live |= {(i, j) for j in range(1, i + 1) if (i + 1, j) in live or (i + 1, j + 1) in live}
    return live


def check_layout(got, op, ab):
    """Every buffer covers the words its polynomial can have at the bounds (a product buffer the
    nu + nv <= bound / 32 + 2 words wave_mul writes), in order and without overlap."""
    run = bcm.OPS[op][0]
    n = len(ab)
    ab = [int(b) for b in ab]
    total = sum(ab)
    K = n.bit_length()
    assert got["K"] == K and got["a_limbs"] == sum(b // 64 + 1 for b in ab)
    assert (got["zeros"], got["leading"]) == (int(bcm.OPS[op][1]), int(bcm.OPS[op][2]))
    # regions in order: word counts | literal | product buffer | two ping-pong buffers | slots
    assert got["oN"] == 0
    assert got["oU"] >= (8 if run else got["J"] + 1)
    assert got["oT"] - got["oU"] >= 2 * (max(ab) // 64 + 1)       # whole limbs of the widest bit
    assert got["oE"] == got["oD"] + 2 * got["cD"] and got["oD"] >= got["oT"]
    cT = got["oD"] - got["oT"]
    off = got["off"]
    if run:
        assert got["J"] == 0 and not got["diag"] and cT == 0
        assert got["cD"] >= total // 32 + 2                        # t_j = t_{j-1} v_j, any j
        ends = off[:K] + [got["lds_per_wave"] - got["oE"]]
        for k in range(K):
            assert ends[k + 1] - ends[k] >= got["bounds"][k] // 32 + 1, (op, n, k)
    else:
        top = 1 << (K - 1)
        J = n // 2 if top == n and n >= 2 else top
        assert got["J"] == J and got["diag"] == int(J < top)
        srt = sorted(ab, reverse=True)
        assert cT >= sum(srt[:J]) // 32 + 2                        # the widest slot's product
        assert got["cD"] >= (total // 32 + 2 if got["diag"] else 0)
        ends = off[1:J + 1] + [got["lds_per_wave"] - got["oE"]]
        assert off[1] == 0
        for j in range(1, J + 1):
            assert ends[j] - ends[j - 1] >= sum(srt[:j]) // 32 + 2, (op, n, j)
    assert ends == sorted(ends) and ends[0] == 0
    assert got["lds_per_wave"] <= 2560  # a quarter of the circuits' general rule: 4 blocks a CU


def test_planner_under_asan_ubsan(driver):
    """Bounds, needed set and layout of the stand-alone planner against the model, over stdin and
    over arguments; the driver's own last case, a u64 count at bound 256, does not fit."""
    from homomorph import _lib
    cases = []
    for n in WIDTHS:
        for ab in input_bounds(n):
            if n >= 24:  # (bounds that fit a wave's share of LDS at these widths)
                ab = ab // (4 if n < 64 else 2 * n)
            for op in bcm.OPS:
                cases.append((op, ab))
    lines = run_cases(driver, cases)
    for (op, ab), got in zip(cases, lines):
        n = len(ab)
        run = bcm.OPS[op][0]
        assert got["which"] == bcm.CODES[op] and got["nbits"] == n and got["run"] == int(run)
        assert got["bounds"] == bcm.bitcount_bounds(op, ab).tolist()
        assert got["m"] == bcm.degree_of(op, n)
        live = reachable(n)
        want = ["".join("1" if (i, j) in live else "0" for j in range(1, i + 1))
                for i in range(1, n + 1)]
        assert got["needed"] == want, (op, n)
        assert want == ["".join("01"[bcm.needed(n, i, j)] for j in range(1, i + 1))
                        for i in range(1, n + 1)]
        if run:
            assert (got["updates"], got["products"]) == (n, n - 1)
        else:
            assert got["updates"] == len(live) and got["products"] == sum(j >= 2 for _, j in live)
        assert got["status"] == 0, (op, n, ab.tolist(), got["status"])
        check_layout(got, op, ab)
    big = lines[-1]
    assert big["status"] == _lib.ERR_UNSUPPORTED and big["nbits"] == 64 and big["which"] == 22
    assert big["bounds"] == [256 << k for k in range(7)] + [0]
    # the updates the rule leaves: 29, 101 and 373 (21, 85, 341 of them products)
    counts = {n: next(g for (op, ab), g in zip(cases, lines) if op == "count_ones" and len(ab) == n)
              for n in (8, 32)}
    assert (counts[8]["updates"], counts[8]["products"]) == (29, 21)
    assert (counts[32]["updates"], counts[32]["products"]) == (373, 341)


def test_what_fits(driver):
    """u8, u16 and u32 at a uniform bound of 256 plan within the LDS rule for all six ops, over
    arguments; a u64 count at 256 and a u32 at 512 are refused."""
    from homomorph import _lib
    for n in (8, 16, 32):
        for op in bcm.OPS:
            ab = np.full(n, 256, np.uint32)
            r = subprocess.run([driver] + case_line(op, ab).split(), capture_output=True,
                               text=True, timeout=60, env=ENV)
            assert r.returncode == 0, r.stderr[-2000:]
            one, big = [json.loads(x) for x in r.stdout.splitlines()]
            assert one["status"] == 0 and one["lds_per_wave"] <= 2560, (op, n, one["lds_per_wave"])
            check_layout(one, op, ab)
            if n == 16 and op == "count_ones":
                assert (one["updates"], one["products"]) == (101, 85)
            if n == 32:  # about 1 800 words for a count, 2 100 for a run
                lo, hi = (2000, 2200) if bcm.OPS[op][0] else (1700, 1900)
                assert lo <= one["lds_per_wave"] <= hi, (op, one["lds_per_wave"])
    assert big["status"] == _lib.ERR_UNSUPPORTED
    refused = [("count_ones", np.full(64, 256, np.uint32)), ("count_zeros", np.full(64, 256, np.uint32)),
               ("leading_zeros", np.full(64, 256, np.uint32)), ("count_ones", np.full(32, 512, np.uint32)),
               ("trailing_ones", np.full(32, 512, np.uint32))]
    for got in run_cases(driver, refused)[:-1]:
        assert got["status"] == _lib.ERR_UNSUPPORTED
    # a malformed case is refused: a missing bound, a width of 0 or 129, a which outside the six
    for bad in (["22", "8"] + ["10"] * 7, ["22", "0"], ["22", "129"] + ["1"] * 129,
                ["21", "8"] + ["10"] * 8, ["28", "8"] + ["10"] * 8):
        r = subprocess.run([driver] + bad, capture_output=True, text=True, env=ENV)
        assert r.returncode == 2
