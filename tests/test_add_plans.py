"""The adder's planner (homomorph-rust_amd/csrc/add_host.h plan_add) against the plans recorded
before it was moved out of hm_add_batch (CPU only).

tests/golden/add_plans.json holds, for a grid of (nbits, n, add_chain, fp4_mfma, bounds), the
status and every plan field of AddArgs as the inline planner of ABI version 7 computed them.  The
grid reaches every branch of the planner: n on both sides of the values-per-wave gate (16384) and
of the `want` thresholds; nbits 8 .. 128 (ceil(L / 64) binds at 128) and 1, 2, 4, 12, 24; uniform
bounds at 127/128, 255/256 (the uniform prep taken, and missed by one bit or one operand),
266/267, 522/523, 1023/1024; the per-bit cases of synth.ADD_CASES; the three chain options with
and without the fp4 MFMA; and cases refused at the prep LDS limit, at the chain LDS limit and for
an explicit MFMA chain that has no plan.  (The fourth refusal, more than 64 bits per prep wave,
cannot be reached with nbits <= 128: wpv >= ceil(L / 64).)

The cases run through tests/sanitize/add_census.cpp, the planner compiled alone into an ASan +
UBSan driver, and must agree field by field.
"""
import json
import os
import shutil

import pytest

import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "add_plans.json")
UNSUPPORTED = 7  # HM_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def table():
    if not os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("make") is None:
        pytest.skip("needs hipcc and make")
    with open(GOLDEN) as f:
        return json.load(f)


def test_recorded_grid_reaches_every_branch(table):
    """The recorded table itself: a few hundred cases, each planner branch taken and not taken."""
    f = {k: i for i, k in enumerate(table["fields"])}
    plans = [c[7] for c in table["cases"] if c[6] == 0]
    assert 200 <= len(table["cases"]) <= 600
    assert {c[6] for c in table["cases"]} == {0, UNSUPPORTED}
    for key, values in (("top1", {0, 1}), ("ucap", {0, 5}), ("pad", {0, 1}), ("staged", {0, 1}),
                        ("mfma", {0, 7, 13, 25}), ("vpw", {1, 2, 4, 8})):
        assert {p[f[key]] for p in plans} == values, key
    assert {p[f["wpv"]] for p in plans} >= {1, 2, 4, 8}
    assert {c[0] for c in table["cases"]} >= {1, 8, 16, 32, 64, 128}
    assert {c[1] for c in table["cases"]} >= {1, 16383, 16384, 16385, 131072}
    assert {(c[2], c[3]) for c in table["cases"]} == {(ch, fp) for ch in (0, 1, 2) for fp in (0, 1)}


def test_plan_add_equals_the_recorded_plans(table):
    fields = table["fields"]
    bad = []
    for L, n, chain, fp4, a, b, status, plan in table["cases"]:
        ba = tuple([a] * L if isinstance(a, int) else a)
        bb = tuple([b] * L if isinstance(b, int) else b)
        cen = synth.add_census(n, chain, fp4, ba, bb)
        got = [cen[k] for k in fields] if cen["status"] == 0 else None
        if cen["status"] != status or got != plan:
            bad.append(((L, n, chain, fp4, a, b), (status, plan), (cen["status"], got)))
    assert not bad, (len(bad), bad[:3])
