"""CPU checks of the oblivious array read and write: the model circuits
(tests/array_model.py) on 0 / 1 values and after decryption at the edge of the requirement, the
tree against the indicator sum, a read of trivial elements against the lookup model, and the
degrees against the bounds; the host-only bounds entry points against the model's rule; the
requirement numbers; and the planner header compiled alone into an ASan + UBSan driver
(tests/sanitize/array_plan.cpp) whose bounds, product counts and layout are compared with the
model.  No GPU, no launch.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import array_model as am
import borrow_model as bm
import lookup_model as lm
from helpers import as_bytes, bit_ints, keys, masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRESH = 192
COUNTS = (2, 3, 4, 5, 16, 256)


@pytest.fixture(scope="module")
def H():
    import homomorph
    homomorph.lib()
    return homomorph


def bound_families(n, step=37):
    """Uniform; skewed up; skewed down; with zeros (null bit positions)."""
    i = np.arange(n)
    holes = np.where(i % 3 == 1, 0, FRESH + 5 * i)
    return [np.full(n, FRESH, np.uint32), (FRESH + step * i).astype(np.uint32),
            (FRESH + step * i[::-1]).astype(np.uint32), holes.astype(np.uint32)]


def bits_of(x, n):
    return [(int(x) >> i) & 1 for i in range(n)]


# ------------------------------------------------------------------ the model circuits
@pytest.mark.parametrize("count", COUNTS)
def test_model_on_plain_bits_is_indexing(count):
    """On 0 / 1 polynomials a read is arr[i] and a write a copy with one element replaced; an
    index >= count reads 0 and writes nowhere."""
    rng = np.random.default_rng(count)
    k = am.index_bits(count)
    arr = [int(x) for x in rng.integers(0, 256, count)]
    arr[0] = 0xA5
    els = [bits_of(a, 8) for a in arr]
    indices = range(1 << k) if count <= 16 else [0, 1, 127, 128, 254, 255]
    for i in indices:
        s = bits_of(i, 8)  # (bits above k are not read)
        got = am.circuit_read(els, s)
        assert all(p in (0, 1) for p in got)
        want = arr[i] if i < count else 0
        assert sum(p << j for j, p in enumerate(got)) == want == am.int_read(arr, i, count)
        x = 0x3C ^ i
        out = am.circuit_write(els, s, bits_of(x, 8))
        vals = [sum(p << j for j, p in enumerate(el)) for el in out]
        assert vals == am.int_write(arr, i, x, count)
        if i >= count:
            assert vals == arr
        else:
            assert vals[i] == x and vals[:i] == arr[:i] and vals[i + 1:] == arr[i + 1:]
    # bits of the index above k are ignored
    assert am.circuit_read(els, bits_of(1, k) + [1] * (8 - k)) == am.circuit_read(els, bits_of(1, 8))


@pytest.mark.parametrize("count", [2, 3, 4, 5, 7, 16])
def test_tree_equals_the_indicator_sum(count):
    """The multiplexer tree and the sum of indicator times element are the same polynomials, for
    random polynomials, with null and unit ones among the index bits and the elements."""
    rng = np.random.default_rng(100 + count)
    k = am.index_bits(count)
    rnd = lambda: int.from_bytes(rng.bytes(3), "little") | 1  # noqa: E731
    for trial in range(3):
        s = [rnd() for _ in range(k)]
        arr = [[rnd() for _ in range(3)] for _ in range(count)]
        if trial == 1:
            s[0], arr[0][1], arr[count - 1][2] = 1, 0, 1
        if trial == 2:
            s[k - 1] = 0
        assert am.circuit_read(arr, s) == am.circuit_read_sum(arr, s)
    assert am.read_products(1, count) == sum(-(-count // (1 << t)) for t in range(1, k + 1))
    if count & (count - 1) == 0:
        assert am.read_products(8, count) == 8 * (count - 1)


@pytest.mark.parametrize("params,count", [((5, 8, 1, 8), 2), ((7, 8, 1, 8), 3), ((7, 8, 1, 8), 4)])
def test_model_decrypts_at_the_edge_of_the_requirement(H, oracle, model, params, count):
    """Fresh ciphertexts at d = (2k + 3) delta: both circuits decrypt to the integer semantics and
    their degrees stay within the bounds."""
    d, dp, delta, tau = params
    k = am.index_bits(count)
    for marker in (H.HomomorphicArrayRead, H.HomomorphicArrayWrite):
        assert marker.min_d_over_delta(k) == 2 * k + 3 == d // delta
    sk, pk, _ = keys(d, dp, delta, tau, 47)
    sec = model.limbs_to_int(sk)
    n = 1 << k  # every index of k bits, those >= count among them
    rng = np.random.default_rng(count)
    av = rng.integers(0, 256, n * count).astype(np.uint8)
    iv = np.arange(n, dtype=np.uint8) | np.uint8(0xF0)  # (high bits set: not read)
    xv = rng.integers(0, 256, n).astype(np.uint8)
    b8 = np.full(8, d + dp, np.uint32)
    la, da = oracle.encrypt_batch(pk, as_bytes(av), masks(len(av), 8, tau, 1), b8)
    li, di = oracle.encrypt_batch(pk, as_bytes(iv), masks(n, 8, tau, 2), b8)
    lx, dx = oracle.encrypt_batch(pk, as_bytes(xv), masks(n, 8, tau, 3), b8)
    rb, wb = am.read_bounds(b8, count, b8), am.write_bounds(b8, b8, count, b8)
    for e in range(n):
        arr = [bit_ints(la, da, b8, e * count + v) for v in range(count)]
        s, x = bit_ints(li, di, b8, e), bit_ints(lx, dx, b8, e)
        plain = [int(a) for a in av[e * count:(e + 1) * count]]
        got = am.circuit_read(arr, s)
        assert all(model.degree(p) <= int(rb[j]) for j, p in enumerate(got))
        assert bm.decrypt_value(got, sec) == am.int_read(plain, e, count), (count, e)
        out = am.circuit_write(arr, s, x)
        assert all(model.degree(p) <= int(wb[j]) for el in out for j, p in enumerate(el))
        assert [bm.decrypt_value(el, sec) for el in out] == am.int_write(plain, e, int(xv[e]), count)


@pytest.mark.parametrize("count", [2, 4, 16])
def test_read_of_trivial_elements_is_the_lookup_model(count):
    """Elements that are null / unit polynomials from a plaintext table: the multilinear form is
    unique, so the read gives the lookup's polynomials for the same table."""
    rng = np.random.default_rng(count)
    k = am.index_bits(count)
    table = rng.integers(0, 256, count).astype(np.uint8)
    s = [int.from_bytes(rng.bytes(3), "little") | 1 for _ in range(k)]
    s[0] = 1 if count == 4 else s[0]
    arr = [bits_of(t, 8) for t in table]
    assert am.circuit_read(arr, s) == lm.lookup_circuit(s, table)


# ------------------------------------------------------------------ the bounds entry points
@pytest.mark.parametrize("count", COUNTS)
def test_bounds_equal_the_model(H, count):
    k = am.index_bits(count)
    for nbits in (1, 8, 32):
        for ab, xb in zip(bound_families(nbits), bound_families(nbits)[::-1]):
            for sb in bound_families(8, 11):
                r = H.array_read_out_bounds(ab, count, sb)
                w = H.array_write_out_bounds(ab, xb, count, sb)
                assert r.dtype == w.dtype == np.uint32 and r.size == w.size == nbits
                assert np.array_equal(r, am.read_bounds(ab, count, sb)), (count, nbits)
                assert np.array_equal(w, am.write_bounds(ab, xb, count, sb)), (count, nbits)
                S = int(sb[:k].sum())
                assert r.tolist() == [S + int(b) for b in ab]
                assert np.array_equal(H.array_read_out_bounds(ab, count, sb[:k]), r)
    # the headline shape: u8 x 16 at D = 256 under a u8 index
    D = np.full(8, 256, np.uint32)
    assert H.array_read_out_bounds(D, 16, D).tolist() == [1280] * 8
    assert H.batch_stride(H.array_read_out_bounds(D, 16, D)) == 168
    assert H.array_write_out_bounds(D, D, 256, D).tolist() == [2304] * 8


def test_bounds_reject_bad_arguments(H):
    from homomorph import _lib
    L = _lib.lib()
    a = np.full(256, 10, np.uint32)
    out = np.zeros(256, np.uint32)
    p32 = lambda x: x.ctypes.data_as(_lib.u32p)  # noqa: E731
    INV, UNS = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_UNSUPPORTED
    for count in (2, 3, 255, 256):
        assert L.hm_array_read_out_bounds(8, p32(a), count, p32(a), p32(out)) == _lib.OK
        assert L.hm_array_write_out_bounds(8, p32(a), p32(a), count, p32(a), p32(out)) == _lib.OK
    for count in (0, 1, 257, 1 << 16):
        assert L.hm_array_read_out_bounds(8, p32(a), count, p32(a), p32(out)) == INV
        assert L.hm_array_write_out_bounds(8, p32(a), p32(a), count, p32(a), p32(out)) == INV
    for nbits in (0, 129):
        assert L.hm_array_read_out_bounds(nbits, p32(a), 4, p32(a), p32(out)) == INV
        assert L.hm_array_write_out_bounds(nbits, p32(a), p32(a), 4, p32(a), p32(out)) == INV
    assert L.hm_array_read_out_bounds(8, None, 4, p32(a), p32(out)) == INV
    assert L.hm_array_read_out_bounds(8, p32(a), 4, None, p32(out)) == INV
    assert L.hm_array_read_out_bounds(8, p32(a), 4, p32(a), None) == INV
    assert L.hm_array_write_out_bounds(8, p32(a), None, 4, p32(a), p32(out)) == INV
    # beyond the engine's degree range: an element bound, or the index bounds' sum
    big = a.copy()
    big[3] = 1 << 30
    half = np.full(8, 1 << 27, np.uint32)
    assert L.hm_array_read_out_bounds(8, p32(big), 4, p32(a), p32(out)) == UNS
    assert L.hm_array_read_out_bounds(8, p32(a), 256, p32(half), p32(out)) == UNS
    assert L.hm_array_read_out_bounds(8, p32(a), 16, p32(half), p32(out)) == _lib.OK
    assert L.hm_array_write_out_bounds(8, p32(a), p32(big), 4, p32(a), p32(out)) == UNS
    # the batch entries refuse null pointers before they need a device
    assert L.hm_array_read_batch(None, None, 4, None, None) == INV
    assert L.hm_array_write_batch(None, None, 4, None, None, None) == INV
    with pytest.raises(ValueError):
        H.array_read_out_bounds(a[:8], 16, a[:3])  # four index bits are read
    with pytest.raises(ValueError):
        H.array_read_out_bounds(a[:8], 257, a[:8])


def test_requirement_numbers(H):
    from homomorph import _lib
    L = _lib.lib()
    assert L.hm_abi_version() >= 11
    assert (_lib.OP_ARRAY_READ, _lib.OP_ARRAY_WRITE) == (28, 29) == (am.CODES["read"], am.CODES["write"])
    for marker, code in ((H.HomomorphicArrayRead, 28), (H.HomomorphicArrayWrite, 29)):
        assert marker.CODE == code and marker.MIN_D_OVER_DELTA is None
        assert [marker.min_d_over_delta(marker.index_bits(c)) for c in (2, 4, 16, 256)] == [5, 7, 11, 19]
        assert [marker.index_bits(c) for c in (2, 3, 4, 5, 16, 17, 255, 256)] == [1, 2, 2, 3, 4, 5, 8, 8]
        for k in range(1, 9):
            assert marker.min_d_over_delta(k) == 2 * am.degree_of(k) + 1 == 2 * k + 3
        for bad in (0, 9):
            with pytest.raises(ValueError):
                marker.min_d_over_delta(bad)
        for bad in (1, 257):
            with pytest.raises(ValueError):
                marker.index_bits(bad)
        # hm_validate_operation has no width; without a context hm_validate_operation_bits can
        # only refuse (tests/test_gpu_array.py reads the engine's numbers)
        req = ctypes.c_uint16()
        assert L.hm_validate_operation(None, code, ctypes.byref(req)) == _lib.ERR_INVALID_ARGUMENT
        assert (L.hm_validate_operation_bits(None, code, 4, ctypes.byref(req))
                == _lib.ERR_INVALID_ARGUMENT)


# ------------------------------------------------------------------ the planner, stand-alone
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("array_plan") / "array_plan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "sanitize", "array_plan.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    return exe


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
           UBSAN_OPTIONS="print_stacktrace=1")


def case_line(op, count, ab, xb, sb):
    k = am.index_bits(count)
    xs = list(xb) if op == "write" else []
    return " ".join(str(int(x)) for x in [am.CODES[op], len(ab), count, *ab, *xs, *sb[:k]])


def run_cases(driver, cases):
    r = subprocess.run([driver], input="\n".join(case_line(*c) for c in cases) + "\n",
                       capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines()]
    assert len(lines) == len(cases) + 1
    return lines


def words(bound):
    """What a buffer must hold of a polynomial within bound: wave_mul's nu + nv <= bound / 32 + 2
    words, which covers a loaded bit's whole limbs."""
    return max(int(bound) // 32 + 2, 2 * (int(bound) // 64 + 1))


def check_layout(got, op, count, ab, xb, sb):
    """Every buffer covers the words its polynomial can have at the bounds, in order and without
    overlap, within the slice."""
    k = am.index_bits(count)
    ab, xb, sb = [int(b) for b in ab], [int(b) for b in xb], [int(b) for b in sb[:k]]
    amax, S = max(ab), sum(sb)
    soff = got["soff"][:k]
    assert got["oN"] == 0 and got["k"] == k
    regions = [(soff[t], 2 * (sb[t] // 64 + 1)) for t in range(k)]
    if op == "read":
        assert soff[0] >= 16 and got["shared"] == 0
        lvl = [amax + sum(sb[:t]) for t in range(k + 1)]
        regions += [(got["oL"], words(lvl[0])), (got["oX"], words(lvl[k - 1])),
                    (got["oP"], words(lvl[k])), (got["oP"] + got["cP"], words(lvl[k]))]
        assert got["cP"] >= words(lvl[k])
        regions += [(got["slot"][t], words(lvl[t])) for t in range(k)]
    else:
        wide = max(amax, max(xb))
        assert soff[0] >= 16 + len(ab) and got["sb"][:k] == sb
        regions += [(got["oU"], words(max(sb))), (got["oT"], words(amax)), (got["oX"], words(wide)),
                    (got["oO"], words(S + wide))]
        regions += [(got["qoff"][t], words(sum(sb[t:]))) for t in range(k)]
        regions += [(got["oV"], sum(2 * (b // 64 + 1) for b in xb))]
    regions.sort()
    for (o, w), (nxt, _) in zip(regions, regions[1:] + [(got["lds_per_wave"], 0)]):
        assert o + w <= nxt, (op, count, regions)
    assert got["lds_per_wave"] <= 2560  # the bit counts' rule: 4 blocks a CU


def test_planner_under_asan_ubsan(driver):
    """Bounds, product counts and layout of the stand-alone planner against the model; the driver's
    own last case, 256 elements at bound 2048, does not fit."""
    from homomorph import _lib
    cases = []
    for count in COUNTS + (7, 255):
        for nbits in (1, 8, 32):
            fam = bound_families(nbits)
            for ab, xb in zip(fam, fam[::-1]):
                for sb in (bound_families(8, 11)[1], bound_families(8, 11)[3]):
                    if nbits == 32:  # (bounds that fit a wave's share of LDS at this width)
                        ab, xb = ab // 2, xb // 2
                    for op in ("read", "write"):
                        cases.append((op, count, ab, xb, sb))
    lines = run_cases(driver, cases)
    for (op, count, ab, xb, sb), got in zip(cases, lines):
        nbits = len(ab)
        assert (got["which"], got["nbits"], got["count"]) == (am.CODES[op], nbits, count)
        assert got["m"] == am.degree_of(am.index_bits(count))
        want = am.read_bounds(ab, count, sb) if op == "read" else am.write_bounds(ab, xb, count, sb)
        assert got["bounds"] == want.tolist()
        assert got["indicator_products"] == am.indicator_products(count)
        assert got["products"] == (am.read_products(nbits, count) if op == "read"
                                   else am.write_products(nbits, count))
        assert got["status"] == 0, (op, count, nbits, got)
        check_layout(got, op, count, ab, xb, sb)
    big = lines[-1]
    assert big["status"] == _lib.ERR_UNSUPPORTED and (big["count"], big["nbits"]) == (256, 8)
    assert big["bounds"] == [9 * 2048] * 8
    # product counts: a power of two reads with count - 1 products per bit; about two indicator
    # products per element
    assert am.read_products(8, 16) == 8 * 15 and am.read_products(8, 5) == 8 * 6
    assert am.indicator_products(2) == 0 and am.indicator_products(4) == 1 + 1 + 2
    assert am.indicator_products(256) == 7 + sum(
        ((v & -v).bit_length() - (v == 128)) for v in range(1, 256)) < 2 * 256


def test_what_fits(driver):
    """The rule must admit every count <= 256 at D = 256: the read at any element width, the write
    with elements up to 32 bits.  k = 8 at bound 2048 is refused, over arguments."""
    from homomorph import _lib
    cases = []
    for count in (2, 3, 16, 17, 255, 256):
        for nbits in (8, 32, 128):
            D = np.full(nbits, 256, np.uint32)
            cases.append(("read", count, D, D, np.full(8, 256, np.uint32)))
            if nbits <= 32:
                cases.append(("write", count, D, D, np.full(8, 256, np.uint32)))
    lines = run_cases(driver, cases)
    read256 = set()
    for c, got in zip(cases, lines):
        assert got["status"] == 0 and got["lds_per_wave"] <= 2560, (c[0], c[1], got)
        check_layout(got, *c)
        if c[0] == "read" and c[1] == 256:
            read256.add(got["lds_per_wave"])
    assert len(read256) == 1 and 550 <= read256.pop() <= 750  # no dependence on the element width
    w32 = next(g for c, g in zip(cases, lines) if c[0] == "write" and c[1] == 256 and len(c[2]) == 32)
    assert 700 <= w32["lds_per_wave"] <= 1300
    D = np.full(8, 2048, np.uint32)
    r = subprocess.run([driver] + case_line("read", 256, D, D, D).split(), capture_output=True,
                       text=True, timeout=60, env=ENV)
    assert r.returncode == 0, r.stderr[-2000:]
    one, big = [json.loads(x) for x in r.stdout.splitlines()]
    assert one["status"] == big["status"] == _lib.ERR_UNSUPPORTED
    refused = [("write", 256, D, D, D), ("write", 256, np.full(128, 512, np.uint32),
                                         np.full(128, 512, np.uint32), np.full(8, 512, np.uint32))]
    for got in run_cases(driver, refused)[:-1]:
        assert got["status"] == _lib.ERR_UNSUPPORTED
    # a malformed case is refused: a missing bound, a count of 1 or 257, a which outside the two
    for bad in (["28", "8", "4"] + ["10"] * 9, ["28", "8", "1"] + ["10"] * 8,
                ["28", "8", "257"] + ["10"] * 17, ["27", "8", "4"] + ["10"] * 10,
                ["29", "8", "4"] + ["10"] * 10, ["28", "0", "4", "1", "1"]):
        r = subprocess.run([driver] + bad, capture_output=True, text=True, env=ENV)
        assert r.returncode == 2
