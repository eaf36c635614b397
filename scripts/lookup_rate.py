"""Rates of the table lookup at d = dp = tau = 128, batch 4096.

Times, with preallocated outputs and device events on the engine's stream around LAUNCHES
back-to-back launches ending in a synchronise (the method of scripts/select_rate.py):
  - u8 -> u8 with a random table (every monomial, up to 15 products per output bit);
  - u8 -> u8 with the identity table (no product at all: what the plaintext sparsity saves);
  - u8 -> u32 with a random table (32 output bits);
  - hm_select_batch on u8 operands under a fresh condition, the yardstick from the same family
    (8 products per value).
The legs are timed in turn, ROUNDS times over in one process (so clock and thermal drift hit all
alike); the median and the minimum of the rounds are reported.  All results of every leg are
decrypted and checked against table[v] (the select against numpy); the script writes the JSON and
exits non-zero when any value disagrees.

usage: lookup_rate.py [--out profiles/lookup/rates.json] [--n 4096] [--launches 50] [--rounds 7]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup", "rates.json"))
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    n, K = args.n, max(args.launches, 20)

    ctx = H.Context(H.Parameters(*PARAMS), device="cuda:0")
    ctx.seed_rng(11)
    ctx.generate_secret_key()
    ctx.generate_public_key()
    rng = np.random.default_rng(3)
    av = rng.integers(0, 256, size=n, dtype=np.uint8)
    bv = rng.integers(0, 256, size=n, dtype=np.uint8)
    cv = rng.integers(0, 2, size=n, dtype=np.uint8)
    a, b, c = ctx.encrypt(av), ctx.encrypt(bv), ctx.encrypt(cv)
    dev = ctx.device
    tables = {
        "lookup_u8_u8_random": rng.integers(0, 256, size=256, dtype=np.uint8),
        "lookup_u8_u8_identity": np.arange(256, dtype=np.uint8),
        "lookup_u8_u32_random": rng.integers(0, 2**32, size=256, dtype=np.uint32),
    }
    outs = {k: H.Ciphered.empty(n, H.lookup_out_bounds(a.bound, t), dev, t.dtype)
            for k, t in tables.items()}
    sel_out = H.Ciphered.empty(n, H.select_out_bounds(c.bound[0], a.bound, b.bound), dev,
                               np.dtype(np.uint8))

    def leg(k):
        return lambda: H.lookup_into(ctx, a, tables[k], outs[k])
    legs = {k: leg(k) for k in tables}
    legs["select_u8"] = lambda: H.select_into(ctx, c, a, b, sel_out)
    out_bytes = {k: o.stride * 8 for k, o in outs.items()}
    out_bytes["select_u8"] = sel_out.stride * 8

    for fn in legs.values():  # warm-up: code objects
        for _ in range(3):
            fn()
    ctx.synchronize()
    wrong = {k: int((ctx.decrypt(outs[k]) != t[av]).sum()) for k, t in tables.items()}
    wrong["select_u8"] = int((ctx.decrypt(sel_out) != np.where(cv, av, bv)).sum())

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

    res = {"script": "scripts/lookup_rate.py", "params": list(PARAMS), "batch": n,
           "launches_per_timing": K, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0),
           "values_checked_per_leg": n, "values_decrypting_wrongly": wrong, "legs": {}}
    for name, ts in times.items():
        med = statistics.median(ts)
        res["legs"][name] = {"ms_per_call_median": med, "ms_per_call_min": min(ts),
                             "ms_per_call_rounds": ts, "values_per_s_median": n / (med * 1e-3),
                             "out_bytes_per_value": out_bytes[name]}
    sel = res["legs"]["select_u8"]["ms_per_call_median"]
    res["over_select_median"] = {k: res["legs"][k]["ms_per_call_median"] / sel for k in tables}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    if any(wrong.values()):
        sys.exit("decrypted results disagree with the table")


if __name__ == "__main__":
    main()
