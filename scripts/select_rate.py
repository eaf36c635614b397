"""Rates of min / max and select at u32, d = dp = tau = 128, batch 4096.

Times, with preallocated outputs and device events on the engine's stream around LAUNCHES
back-to-back launches ending in a synchronise (the method of scripts/compare_rate.py):
  - hm_minmax_batch(MIN), the fused kernel;
  - the composition hm_compare_batch(LT) then hm_select_batch (two launches, the condition
    through device memory);
  - hm_select_batch alone, on that condition.
The three are timed in turn, ROUNDS times over in one process (so clock and thermal drift hit all
alike); the median and the minimum of the rounds are reported.  All 4096 results of the fused min,
the fused max and the composed min are decrypted and checked against numpy, and the fused and the
composed min must be the same ciphertexts; the script writes the JSON and exits non-zero when any
of that fails.

usage: select_rate.py [--out profiles/select/rates.json] [--n 4096] [--launches 50] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "homomorph-rust_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import homomorph as H  # noqa: E402

PARAMS = (128, 128, 1, 128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select", "rates.json"))
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    n, K = args.n, max(args.launches, 20)

    ctx = H.Context(H.Parameters(*PARAMS), device="cuda:0")
    ctx.seed_rng(11)
    ctx.generate_secret_key()
    ctx.generate_public_key()
    av = np.random.default_rng(3).integers(0, 2**32, size=n, dtype=np.uint32)
    bv = np.random.default_rng(4).integers(0, 2**32, size=n, dtype=np.uint32)
    bv[: n // 16] = av[: n // 16]  # some equal pairs
    a, b = ctx.encrypt(av), ctx.encrypt(bv)
    dev, u32 = ctx.device, np.dtype(np.uint32)
    LT, MIN, MAX = H.HomomorphicLessThan, H.HomomorphicMin, H.HomomorphicMax

    mm_bound = H.minmax_out_bounds(a.bound, b.bound)
    min_out = H.Ciphered.empty(n, mm_bound, dev, u32)
    max_out = H.Ciphered.empty(n, mm_bound, dev, u32)
    lt_out = H.Ciphered.empty(n, H.compare_out_bounds(LT, a.bound, b.bound), dev,
                              np.dtype(np.bool_))
    sel_out = H.Ciphered.empty(n, H.select_out_bounds(lt_out.bound[0], a.bound, b.bound), dev, u32)

    def composed():
        H.compare_into(ctx, LT, a, b, lt_out, False)
        H.select_into(ctx, lt_out, a, b, sel_out)

    legs = {
        "minmax_fused": lambda: H.minmax_into(ctx, MIN, a, b, min_out, False),
        "compare_lt_then_select": composed,
        "select_alone": lambda: H.select_into(ctx, lt_out, a, b, sel_out),
    }
    out_bytes = {"minmax_fused": min_out.stride * 8,
                 "compare_lt_then_select": sel_out.stride * 8,
                 "select_alone": sel_out.stride * 8}
    cond_bytes = lt_out.stride * 8

    for fn in legs.values():  # warm-up: code objects
        for _ in range(3):
            fn()
    H.minmax_into(ctx, MAX, a, b, max_out, False)
    ctx.synchronize()
    d_min, d_max, d_sel = ctx.decrypt(min_out), ctx.decrypt(max_out), ctx.decrypt(sel_out)
    wrong = {"min_fused": int((d_min != np.minimum(av, bv)).sum()),
             "max_fused": int((d_max != np.maximum(av, bv)).sum()),
             "min_composed": int((d_sel != np.minimum(av, bv)).sum())}
    same = bool(torch.equal(min_out.limbs, sel_out.limbs)
                and torch.equal(min_out.degree, sel_out.degree))

    times = {k: [] for k in legs}
    with torch.cuda.stream(ctx.stream):
        for _ in range(args.rounds):
            for name, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(ctx.stream)
                for _ in range(K):
                    fn()
                e1.record(ctx.stream)
                ctx.synchronize()
                times[name].append(e0.elapsed_time(e1) / K)

    res = {"script": "scripts/select_rate.py", "params": list(PARAMS), "dtype": "u32", "batch": n,
           "launches_per_timing": K, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0),
           "values_checked": n, "values_decrypting_wrongly": wrong,
           "fused_and_composed_min_are_the_same_ciphertexts": same,
           "condition_bytes_per_value": cond_bytes, "legs": {}}
    for name, ts in times.items():
        med = statistics.median(ts)
        res["legs"][name] = {"ms_per_call_median": med, "ms_per_call_min": min(ts),
                             "ms_per_call_rounds": ts, "values_per_s_median": n / (med * 1e-3),
                             "out_bytes_per_value": out_bytes[name]}
    f, c = res["legs"]["minmax_fused"], res["legs"]["compare_lt_then_select"]
    res["fused_over_composed_median"] = f["ms_per_call_median"] / c["ms_per_call_median"]
    res["fused_faster_than_composed"] = bool(f["ms_per_call_median"] < c["ms_per_call_median"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    if any(wrong.values()) or not same:
        sys.exit("decrypted results or ciphertexts disagree")


if __name__ == "__main__":
    main()
