"""SURVEY.md s5 "race detection / sanitizers": ASan + UBSan builds of the CPU oracle and of the
engine library's host code, run on the CPU (GPU sanitizers are not available on this pool).

- tests/sanitize/oracle_san.c: the reference's polynomial KATs and an encrypt -> add / mul /
  gates -> decrypt round trip through oracle/homomorph_oracle.c;
- tests/sanitize/capi_san.cpp: every host-only C-ABI entry point (status strings, bounds, the
  multiplier cost model, strides, the wire-format parser under 20k corrupted headers, NULL
  contexts), with the device kernels linked in unsanitised;
- tests/sanitize/plan_split.cpp: the multiplier planner (mul_plan.h, host only, nothing linked):
  its split Karatsuba plans, the same leaf products as the breadth-first plans at K = 16, K = 21
  planned, and the byte image of a plan's tables (aligned offsets, equal bytes);
- tests/sanitize/plan_census.cpp: one plan's launches and sizes as JSON (mul_plan.h, host only),
  the source of the full-bounds tier's multiplier path assertions (tests/synth.py mul_census);
- tests/sanitize/add_census.cpp: one adder plan (add_host.h plan_add) as JSON, the planner
  compiled alone into the driver (tests/synth.py add_census, tests/test_add_plans.py);
- tests/sanitize/capi_oom.cpp (not sanitised): every allocation inside the multiplier's plan
  builder failed in turn, each call returning HM_ERR_OUT_OF_MEMORY instead of throwing across
  the C ABI.
Any sanitizer report aborts the binary (-fno-sanitize-recover=all) and fails the test.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "sanitize")


@pytest.fixture(scope="module")
def built():
    if shutil.which("gcc") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("needs gcc and hipcc")
    eng = os.path.join(ROOT, "homomorph-rust_amd")
    subprocess.run(["make", "-s", "-C", eng], check=True, timeout=1200)
    subprocess.run(["make", "-s", "-j4", "-C", SAN], check=True, timeout=1200)
    return os.path.join(SAN, "_build")


def _run(path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([path], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_oracle_under_asan_ubsan(built):
    assert "ok" in _run(os.path.join(built, "oracle_san"))


def test_engine_host_code_under_asan_ubsan(built):
    assert "ok" in _run(os.path.join(built, "capi_san"))


def test_engine_abi_returns_oom_instead_of_throwing(built):
    out = _run(os.path.join(built, "capi_oom"))
    assert "ok" in out and "allocation points" in out


def test_split_karatsuba_plans_under_asan_ubsan(built):
    assert "ok" in _run(os.path.join(built, "plan_split"))


def test_plan_census_under_asan_ubsan(built):
    """tests/sanitize/plan_census.cpp (the driver behind synth.mul_census): the full signed u8
    plan at bounds 640 with its Karatsuba programs, and a refused argument list."""
    import json
    exe = os.path.join(built, "plan_census")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "8", "8", "1", "256", "256", "1"] + ["640"] * 16, capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    cen = json.loads(r.stdout)
    assert len(cen["cols"]) == 8 and cen["pp_instance"] == "mul_ppg_kernel<17>"
    assert sum(len(col["ka"]) for col in cen["cols"]) == 5
    r = subprocess.run([exe, "8", "4", "0", "256", "256", "1", "640"], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 2 and "expected" in r.stderr


def test_add_census_under_asan_ubsan(built):
    """tests/sanitize/add_census.cpp (the driver behind synth.add_census): the headline plan (u8,
    bounds 256, 131072 values: the uniform prep and the NC = 13 MFMA chain), the same on the VALU
    chain, a refused plan and a refused argument list."""
    import json
    exe = os.path.join(built, "add_census")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")

    def run(*args):
        return subprocess.run([exe] + [str(x) for x in args], capture_output=True, text=True,
                              timeout=300, env=env)
    r = run(8, 131072, 0, 1, *[256] * 16)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    cen = json.loads(r.stdout)
    assert cen["status"] == 0 and cen["ucap"] == 5 and cen["mfma"] == 13
    assert cen["prep_instance"] == "add_prep_uniform_kernel<5>"
    assert cen["chain_instance"] == "add_chain_mfma_kernel<13>"
    r = run(8, 131072, 2, 1, *[256] * 16)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    cen = json.loads(r.stdout)
    assert cen["mfma"] == 0 and cen["mf_cw"] == 0 and cen["staged"] == 1
    assert cen["chain_instance"] == "add_chain_staged_kernel<4>"
    r = run(8, 64, 1, 0, *[256] * 16)  # an explicit MFMA chain without the fp4 MFMA
    assert r.returncode == 0 and json.loads(r.stdout) == {"status": 7}
    r = run(8, 64, 0, 1, 256)
    assert r.returncode == 2 and "expected" in r.stderr
