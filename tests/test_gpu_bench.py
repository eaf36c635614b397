"""bench.py on the GPU: the measurement contract of every line, and the multi-rank path with the
real engine.

  - every `secondary` line of `bench.py --full` carries a `roofline` and a `cpu_baseline` (the
    oracle's 1-thread rate, measured or labelled extrapolated), and the lines that verify their
    results report them correct;
  - `bench.py --gpus 2 --workload mixed` with the gloo backend (two ranks sharing the one GPU of a
    test box: the rehearsal mode of bench.setup_dist, never the measured configuration) runs the
    engine on both ranks: rank 1 loads the keys rank 0 broadcast (bench.make_context), each rank
    runs its shard of configs[4] through the strong-scaling chunk loop, the decrypted results are
    gathered, and every sum and product is correct.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(args, env=None, timeout=280):
    e = dict(os.environ, **(env or {}))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=e,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")]
    assert lines, p.stdout[-2000:]
    return json.loads(lines[-1])


def test_bench_every_line_has_roofline_and_cpu_baseline():
    d = _run_bench(["--full", "--steps", "4", "--warmup", "2", "--cpu-seconds", "3"])
    assert d["roofline"]["frac"] > 0 and d["cpu_baseline"]["value"] > 0
    sec = d["secondary"]
    assert "error" not in sec, sec.get("error")
    for name in ("u32_encrypt_decrypt", "u32_encrypt", "u32_decrypt_fresh", "u32_decrypt_after_add",
                 "u32_add_pcie_inclusive", "u8_mul", "u8_decrypt_after_mul", "u32_mul_low12",
                 "u32_mul_low16", "u32_mul_low16_batch16384", "u32_mul_low20", "u32_mul_low24_batch2",
                 "u32_mul_full_extrapolated", "mixed_config4",
                 "config0_u8_encrypt", "config0_u8_decrypt", "config0_u8_add"):
        line = sec[name]
        assert line["value"] > 0, name
        r = line["roofline"]
        assert r["bound"] in ("hbm", "mfma", "pcie") and r["peak"] > 0 and r["achieved"] > 0, name
        assert (r["bound"] == "pcie") == (name == "u32_add_pcie_inclusive"), name
        assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9, name
        assert r["frac"] <= 1.0, (name, r["frac"])  # issued work, never an algorithm's count
        c = line["cpu_baseline"]
        assert c["value"] > 0 and c["cores"] == 1 and c["kind"] == "port", name
    assert sec["u8_mul"]["verified"] and sec["u8_decrypt_after_mul"]["verified"]
    assert sec["config0_u8_decrypt"]["verified"]
    assert sec["config0_u8_add"]["verified"]["correct_sums"] == sec["config0_u8_add"]["batch"]
    assert sec["u32_mul_low16"]["cpu_baseline"]["extrapolated"] is True
    # configs[3] names batch 1024; the batch-16384 rate is a labelled aside
    assert sec["u32_mul_low12"]["batch"] == sec["u32_mul_low16"]["batch"] == 1024
    assert sec["u32_mul_low20"]["batch"] == 1024  # result bits 16..19 at configs[3]'s batch
    assert sec["u32_mul_low16_batch16384"]["batch"] == 16384
    assert sec["u32_mul_low20_batch16"]["batch"] == 16
    assert sec["u32_mul_low24_batch2"]["batch"] == 2  # result bits 20..23 (split plans)
    assert sec["u32_mul_low12"]["cpu_baseline"].get("extrapolated") is None
    m = sec["mixed_config4"]
    assert m["verified"]["correct_sums"] == m["verified"]["correct_products"] == m["global_batch"]


def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path, oracle):
    """A plain run prints the headline only (nothing that takes a run of its own), times exactly
    --steps steps, and --dump-outputs writes the last step's output as float .npy files: the same
    files from run to run (identical inputs), degrees that are the top bits of the limbs written,
    and ciphertexts bit-identical to the oracle's sums of the same seeded inputs."""
    import numpy as np
    from helpers import as_bytes, assert_batches_equal, seeded_value_masks
    n, runs = 512, []
    for name in ("a", "b"):
        out = tmp_path / name
        d = _run_bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(n),
                        "--dump-outputs", str(out)], timeout=120)
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
        assert d["unit"] == "u32 homomorphic adds/s" and d["dtype"] == "u32" and d["higher_is_better"]
        assert abs(d["value"] - n / (d["ms_per_step"] / 1e3)) <= 1e-6 * d["value"]
        assert d["roofline"]["frac"] > 0 and "sustained" not in d["roofline"]
        for key in ("cpu_baseline", "secondary", "verified"):
            assert key not in d, key
        files = sorted(p.name for p in out.iterdir())
        assert files == ["add_out_bound.npy", "add_out_degree.npy", "add_out_limbs.npy",
                         "add_out_values.npy"]
        assert sum(p.stat().st_size for p in out.iterdir()) <= 64 << 20
        runs.append({f[:-4]: np.load(out / f, allow_pickle=False) for f in files})
    a, b = runs
    for key, arr in a.items():
        assert arr.dtype in (np.float32, np.float64), key
        assert np.array_equal(arr, b[key]), key
    idx = a["add_out_values"].astype(np.int64)
    k = len(idx)
    assert 0 < k <= n and len(set(idx.tolist())) == k and idx.min() >= 0 and idx.max() < n
    limbs, deg = a["add_out_limbs"], a["add_out_degree"]
    cap = a["add_out_bound"].astype(np.int64) // 64 + 1
    assert limbs.shape == (k, 8 * cap.sum()) and deg.shape == (k, 32) and cap.shape == (32,)
    assert limbs.min() >= 0 and limbs.max() <= 255 and np.array_equal(limbs, np.round(limbs))
    # every polynomial's degree word is the top set bit of its limbs (0 for a null polynomial)
    bits = np.unpackbits(limbs.astype(np.uint8), axis=1, bitorder="little")
    off = 0
    for i in range(32):
        seg = bits[:, 64 * off: 64 * (off + cap[i])]
        top = np.where(seg.any(axis=1), seg.shape[1] - 1 - np.argmax(seg[:, ::-1], axis=1), 0)
        assert np.array_equal(top, deg[:, i].astype(np.int64)), i
        off += cap[i]
    assert deg.max() > 256  # sums of fresh ciphertexts: carry polynomials far above d + d'
    # the first sampled values against the oracle: bench.py's keys (seed 0xB0B), shard 0's
    # plaintexts and the seeded engine CSPRNG's masks (draws 0 and 1: the two encrypt calls)
    rng = np.random.default_rng(1000)  # bench.shard_inputs(0, n)
    x = rng.integers(0, 2**32, size=n, dtype=np.uint32)
    y = rng.integers(0, 2**32, size=n, dtype=np.uint32)
    some, params = idx[:4], (128, 128, 1, 128)
    _, pk, _ = oracle.keygen(*params, 0xB0B)
    fresh = np.full(32, params[0] + params[1], dtype=np.uint32)
    ob = a["add_out_bound"].astype(np.uint32)
    mb = (params[3] + 7) // 8
    ma, my = (seeded_value_masks(0xB0B, draw, some, 32, mb) for draw in (0, 1))
    la, da = oracle.encrypt_batch(pk, as_bytes(x[some]), ma, fresh)
    lb, db = oracle.encrypt_batch(pk, as_bytes(y[some]), my, fresh)
    rl, rd = oracle.add_batch(la, da, fresh, lb, db, fresh, 32, len(some), ob)
    gl = np.ascontiguousarray(limbs[:4].astype(np.uint8)).view("<u8").reshape(-1)
    assert_batches_equal(gl, deg[:4].astype(np.uint32), rl, rd, ob, len(some), "dumped sums")


def test_bench_two_ranks_run_the_engine():
    n = 262144
    d = _run_bench(["--gpus", "2", "--workload", "mixed", "--batch", str(n), "--steps", "1",
                    "--warmup", "1"], env={"HM_BENCH_BACKEND": "gloo"})
    assert d["world_size_seen"] == 2 and d["n_gpus"] == 2
    assert d["config"]["batch_per_gpu"] == n // 2
    assert d["verified"] == {"correct_sums": n, "correct_products": n, "of": n}


def test_bench_two_ranks_headline_add():
    """The headline add path (run_add) at world size 2 on one card (gloo): each rank adds its own
    4096-value shard (weak scaling), the sustained-clock replays run per rank, and rank 0 gathers
    every sum for the check (the driver's N-GPU runs take this path over RCCL)."""
    d = _run_bench(["--gpus", "2", "--full", "--steps", "3", "--warmup", "1"],
                   env={"HM_BENCH_BACKEND": "gloo"})
    assert d["world_size_seen"] == 2 and d["n_gpus"] == 2 and d["scaling"] == "weak"
    assert d["config"]["global_batch"] == 8192 and d["verified"]["of"] == 8192
    assert d["verified"]["correct_sums"] >= 8192 - 16  # (the scheme's noise aside)
    assert d["roofline"]["sustained"]["kernel_ms"] > 0
