"""Rates of the shift by an encrypted amount at d = dp = tau = 128, u32, batch 4096 (DESIGN.md
s4.4d).

Times, with preallocated outputs and device events on the engine's stream around LAUNCHES
back-to-back launches ending in a synchronise (the method of scripts/lookup_rate.py):
  - hm_shift_batch(SHL) and hm_shift_batch(ROTL) on fresh u32 values under a fresh u8 amount;
  - the composition the engine offered before: five hm_select_batch launches on preallocated
    operands that carry the five stages' bounds (D, 2 D, .. 5 D in, 2 D .. 6 D out), the moved copy
    of each stage standing ready, i.e. WITHOUT the bit permutations and the Ciphered<bool> a real
    composition would also have to make, which flatters it;
  - one hm_select_batch on fresh u32 operands, the yardstick from the same family.
The legs are timed in turn, ROUNDS times over in one process (so clock and thermal drift hit all
alike); the median and the minimum of the rounds are reported.  All results of the two shift legs
are decrypted and checked against numpy; the script writes the JSON and exits non-zero when any
value disagrees.

usage: shift_rate.py [--out profiles/shift/rates.json] [--n 4096] [--launches 50] [--rounds 7]
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
STAGES = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shift", "rates.json"))
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
    av = rng.integers(0, 2**32, size=n, dtype=np.uint32)
    bv = rng.integers(0, 2**32, size=n, dtype=np.uint32)
    sv = rng.integers(0, 256, size=n, dtype=np.uint8)
    cv = rng.integers(0, 2, size=n, dtype=np.uint8)
    a, b, s, c = ctx.encrypt(av), ctx.encrypt(bv), ctx.encrypt(sv), ctx.encrypt(cv)
    dev = ctx.device
    ops = {"shift_shl_u32": H.HomomorphicShiftLeft, "shift_rotl_u32": H.HomomorphicRotateLeft}
    outs = {k: H.Ciphered.empty(n, H.shift_out_bounds(op, a.bound, s.bound), dev, av.dtype)
            for k, op in ops.items()}
    # the composition's operands: x[t] the running value, m[t] a second batch at the same bounds
    # (standing in for the moved copy), both at (t + 1) D; x[t + 1] = select(c, m[t], x[t])
    x, m = [a], [b]
    for t in range(STAGES):
        x.append(ctx.select(c, m[t], x[t]))
        m.append(ctx.select(c, x[t], m[t]))
    assert np.array_equal(x[STAGES].bound, outs["shift_shl_u32"].bound)
    sel_out = H.Ciphered.empty(n, H.select_out_bounds(c.bound[0], a.bound, b.bound), dev, av.dtype)

    def five_selects():
        for t in range(STAGES):
            H.select_into(ctx, c, m[t], x[t], x[t + 1])

    def leg(k):
        return lambda: H.shift_into(ctx, ops[k], a, s, outs[k])
    legs = {k: leg(k) for k in ops}
    legs["five_selects_u32"] = five_selects
    legs["select_u32"] = lambda: H.select_into(ctx, c, a, b, sel_out)
    out_bytes = {k: o.stride * 8 for k, o in outs.items()}
    out_bytes["five_selects_u32"] = sum(x[t + 1].stride * 8 for t in range(STAGES))
    out_bytes["select_u32"] = sel_out.stride * 8

    for fn in legs.values():  # warm-up: code objects
        for _ in range(3):
            fn()
    ctx.synchronize()
    k32 = (sv % 32).astype(np.uint32)
    want = {"shift_shl_u32": av << k32,
            "shift_rotl_u32": (av << k32) | (av >> ((32 - k32) % 32).astype(np.uint32))}
    wrong = {k: int((ctx.decrypt(outs[k]) != want[k]).sum()) for k in ops}
    wrong["select_u32"] = int((ctx.decrypt(sel_out) != np.where(cv, av, bv)).sum())

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

    res = {"script": "scripts/shift_rate.py", "params": list(PARAMS), "batch": n,
           "launches_per_timing": K, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0),
           "values_checked_per_leg": n, "values_decrypting_wrongly": wrong, "legs": {}}
    for name, ts in times.items():
        med = statistics.median(ts)
        res["legs"][name] = {"ms_per_call_median": med, "ms_per_call_min": min(ts),
                             "ms_per_call_rounds": ts, "values_per_s_median": n / (med * 1e-3),
                             "out_bytes_per_value": out_bytes[name]}
    five = res["legs"]["five_selects_u32"]["ms_per_call_median"]
    res["over_five_selects_median"] = {k: res["legs"][k]["ms_per_call_median"] / five for k in ops}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    if any(wrong.values()):
        sys.exit("decrypted results disagree with numpy")


if __name__ == "__main__":
    main()
