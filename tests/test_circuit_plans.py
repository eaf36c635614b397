"""The planner of the gates, the ripple-borrow chain, min / max and select
(homomorph-rust_amd/csrc/circuit_host.h) against the plans recorded before it was moved out of
capi.cpp (CPU only).

tests/golden/circuit_plans.json holds, for a grid of (circuit, nbits, bounds), the status and every
layout field as the inline lines of ABI version 9 computed them: the gates AND, OR, XOR, NOT; the
chain's sub, lt, eq; min / max; select with a condition bound of 0, of a fresh bit and of wb_nbits
of the same operands; nbits 1, 8, 16, 32, 64, 128; uniform bounds 63/64, 192, 256, 1023/1024 and
192 + 37 i on one operand and on both; and per circuit the largest uniform u8 bound that is
planned and the next one, which is refused.  (The layouts' word counts are even, so no circuit
meets 10240 or 10241 words exactly with every bound: the rule itself is asked at both.)

The cases run through tests/sanitize/circuit_plan.cpp, the header compiled alone into an ASan +
UBSan driver run as its own process, and must agree field by field.
"""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "circuit_plans.json")
UNSUPPORTED = 7  # HM_ERR_UNSUPPORTED
LDS_WORDS = 10240  # a wave's share of a CU's 160 KiB among the four waves of a block
VARIANTS = {("and", None), ("or", None), ("xor", None), ("not", None), ("sub", None), ("lt", None),
            ("eq", None), ("minmax", None), ("select", "zero"), ("select", "fresh"),
            ("select", "wb")}


def expand(spec, nbits):
    if isinstance(spec, int):
        return [spec] * nbits
    base, step = spec
    return [base + step * i for i in range(nbits)]


def case_line(c):
    words = [c["circuit"], c["nbits"], c["cond"]] + expand(c["a"], c["nbits"])
    if c["b"] is not None:
        words += expand(c["b"], c["nbits"])
    return " ".join(str(w) for w in words)


@pytest.fixture(scope="module")
def cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def planned(cases, tmp_path_factory):
    """(the rule at its edge, the driver's plan of every recorded case)"""
    exe = str(tmp_path_factory.mktemp("circuit_plan") / "circuit_plan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "sanitize", "circuit_plan.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input="\n".join(case_line(c) for c in cases) + "\n",
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(x) for x in r.stdout.splitlines()]
    assert len(rows) == len(cases) + 1
    return rows[0], rows[1:]


def test_recorded_grid(cases):
    """The recorded table itself: the issue's grid, and per circuit both outcomes at the edge."""
    assert {(c["circuit"], c["cond_kind"]) for c in cases} == VARIANTS
    grid = [c for c in cases if c["where"] == "grid"]
    for v in VARIANTS:
        mine = [c for c in grid if (c["circuit"], c["cond_kind"]) == v]
        assert {c["nbits"] for c in mine} == {1, 8, 16, 32, 64, 128}
        for nbits in (1, 8, 16, 32, 64, 128):
            specs = [(c["a"], c["b"]) for c in mine if c["nbits"] == nbits]
            other = None if v[0] == "not" else 192
            both = None if v[0] == "not" else [192, 37]
            want = [(u, None if v[0] == "not" else u) for u in (63, 64, 192, 256, 1023, 1024)]
            assert specs == want + [([192, 37], other), ([192, 37], both)], (v, nbits)
        edge = [c for c in cases if c["where"] == "edge" and (c["circuit"], c["cond_kind"]) == v]
        assert [c["plan"]["status"] for c in edge] == [0, UNSUPPORTED], v
        inside, outside = edge
        assert inside["a"] + 1 == outside["a"] and inside["nbits"] == outside["nbits"] == 8
        assert inside["plan"]["lds_per_wave"] <= LDS_WORDS < outside["plan"]["lds_per_wave"]
    for c in cases:
        if c["cond_kind"] == "wb":  # the last borrow's bound, as a < b of the same operands has it
            w = 0
            for x, y in zip(expand(c["a"], c["nbits"]), expand(c["b"], c["nbits"])):
                w = max(x + y, max(x, y) + w)
            assert c["cond"] == w
        else:
            assert c["cond"] == {None: 0, "zero": 0, "fresh": 192}[c["cond_kind"]]


def test_plans_equal_the_recorded_plans(cases, planned):
    rule, rows = planned
    assert rule == {"fits_10240": 1, "fits_10241": 0}
    bad = []
    for c, got in zip(cases, rows):
        want = c["plan"]
        if set(got) != set(want) or any(got[k] != want[k] for k in want):
            bad.append((case_line(c)[:80], want, got))
    assert not bad, (len(bad), bad[:3])
    for v in VARIANTS:  # planned and refused, every circuit
        sts = {r["status"] for c, r in zip(cases, rows) if (c["circuit"], c["cond_kind"]) == v}
        assert sts == {0, UNSUPPORTED}, v


def test_layouts_hold_what_the_kernels_write(cases, planned):
    """The structural facts the kernels rely on, on the driver's own output: rows in order and
    disjoint; an operand row holds the 2 cap words of its operand's widest bit (and two spare
    words); the borrow buffers SX + chain / 32 + 3 words each; select's product buffer the
    condition's plus the operands' words; the slice ends at lds_per_wave; a status of 0 exactly
    when the slice is within the rule."""
    cap = lambda b: b // 64 + 1  # noqa: E731
    for c, p in zip(cases, planned[1]):
        assert "lds_per_wave" in p, p  # (no case of the grid leaves the engine's degree range)
        n = c["nbits"]
        a, b = expand(c["a"], n), None if c["b"] is None else expand(c["b"], n)
        SA, SB = 2 * max(map(cap, a)), 2 if b is None else 2 * max(map(cap, b))
        assert (p["SA"], p["SB"], p["SX"]) == (SA, SB, max(SA, SB)), c
        SX, end = p["SX"], p["lds_per_wave"]
        assert (p["status"] == 0) == (end <= LDS_WORDS) and p["status"] in (0, UNSUPPORTED)
        if c["circuit"] in ("and", "or", "xor", "not"):
            # the result's buffer: a product of up to SA + SB + 1 words and (OR) x_i behind it
            rows = [(p["oA"], SA + 2), (p["oB"], SB + 2), (p["oT"], 2 * (SA + SB) + 8)]
            assert rows[2][1] >= (SA + SB + 2) + SX
        elif c["circuit"] == "select":
            SC = 2 * cap(c["cond"])
            assert p["SC"] == SC
            rows = [(p["oC"], SC + 2), (p["oA"], SA + 2), (p["oB"], SB + 2), (p["oX"], SX + 2),
                    (p["oT"], SC + SX + 2)]
        else:
            assert p["cw"] == SX + p["chain"] // 32 + 3
            rows = [(p["oA"], SA + 2), (p["oB"], SB + 2), (p["oX"], SX + 2), (p["oP"], SX + 2),
                    (p["oG"], SA + SB + 2), (p["oW"], 2 * p["cw"])]
        at = 0
        for off, words in rows:
            assert off == at, (c, rows)
            at += words
        assert at == end, (c, rows)
