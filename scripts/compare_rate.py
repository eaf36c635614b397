"""Rates of the ripple-borrow operations at u32, d = dp = tau = 128, batch 4096.

Times, with preallocated outputs and device events on the engine's stream around LAUNCHES
back-to-back launches ending in a synchronise:
  - hm_sub_batch;
  - hm_compare_batch(LT) and hm_compare_batch(EQ);
  - the only subtraction the engine offered before them, a - b = NOT(NOT a + b): NOT, then ADD,
    then NOT through hm_gate_batch and hm_add_batch.
The four are timed in turn, ROUNDS times over in one process (so clock and thermal drift hit all
alike); the median and the minimum of the rounds are reported.  Both subtractions must decrypt to
the same values (and to a - b): the script counts the values each gets wrong (and the adder's own
on the same batch, whose noise degree passes d = 128 in a u32's high bits), writes the JSON, and
exits non-zero when they disagree.  Writes the times, rates and bytes per value as JSON.

usage: compare_rate.py [--out profiles/compare/rates.json] [--n 4096] [--launches 50] [--rounds 7]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "homomorph-rust_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import homomorph as H  # noqa: E402
from homomorph import lib  # noqa: E402

PARAMS = (128, 128, 1, 128)


def gate_into(ctx, op, a, b, out):
    """hm_gate_batch into a preallocated output (b = None for NOT)."""
    ca, co = a._c(), out._c()
    cb = b._c() if b is not None else None
    ctx._launch(lambda: lib().hm_gate_batch(ctx._h, op.CODE, ctypes.byref(ca),
                                            ctypes.byref(cb) if cb is not None else None,
                                            ctypes.byref(co)), "hm_gate_batch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare", "rates.json"))
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
    a, b = ctx.encrypt(av), ctx.encrypt(bv)
    dev, u32 = ctx.device, np.dtype(np.uint32)

    sub_out = H.Ciphered.empty(n, H.sub_out_bounds(a.bound, b.bound), dev, u32)
    lt_out = H.Ciphered.empty(n, H.compare_out_bounds(H.HomomorphicLessThan, a.bound, b.bound),
                              dev, np.dtype(np.bool_))
    eq_out = H.Ciphered.empty(n, H.compare_out_bounds(H.HomomorphicEqual, a.bound, b.bound),
                              dev, np.dtype(np.bool_))
    not_a = H.Ciphered.empty(n, H.gate_out_bounds(H.HomomorphicNotGate, a.bound), dev, u32)
    comp_out = H.Ciphered.empty(n, H.add_out_bounds(not_a.bound, b.bound), dev, u32)

    def composed():  # NOT(NOT a + b); the last NOT in place, as Context.apply1 runs it
        gate_into(ctx, H.HomomorphicNotGate, a, None, not_a)
        H.add_into(ctx, not_a, b, comp_out)
        gate_into(ctx, H.HomomorphicNotGate, comp_out, None, comp_out)

    legs = {
        "sub": lambda: H.sub_into(ctx, a, b, sub_out),
        "sub_composed_not_add_not": composed,
        "compare_lt": lambda: H.compare_into(ctx, H.HomomorphicLessThan, a, b, lt_out, False),
        "compare_eq": lambda: H.compare_into(ctx, H.HomomorphicEqual, a, b, eq_out, False),
    }
    out_bytes = {"sub": sub_out.stride * 8, "sub_composed_not_add_not": comp_out.stride * 8,
                 "compare_lt": lt_out.stride * 8, "compare_eq": eq_out.stride * 8}

    for fn in legs.values():  # warm-up: workspaces, code objects
        for _ in range(3):
            fn()
    ctx.synchronize()
    want = (av - bv).astype(np.uint32)
    d_sub, d_comp = ctx.decrypt(sub_out), ctx.decrypt(comp_out)
    same = bool(np.array_equal(d_sub, d_comp))
    sub_wrong, comp_wrong = int((d_sub != want).sum()), int((d_comp != want).sum())
    # the adder alone on the same batch: its noise degree at bit i is about 3 i (delta + 1), past
    # d = 128 for the high bits of a u32, so some of its sums decrypt wrongly at these parameters
    plain_add = H.Ciphered.empty(n, H.add_out_bounds(a.bound, b.bound), dev, u32)
    H.add_into(ctx, a, b, plain_add)
    add_wrong = int((ctx.decrypt(plain_add) != (av + bv).astype(np.uint32)).sum())
    del plain_add
    cmp_ok = bool(np.array_equal(ctx.decrypt(lt_out), av < bv)
                  and np.array_equal(ctx.decrypt(eq_out), av == bv))

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

    res = {"script": "scripts/compare_rate.py", "params": list(PARAMS), "dtype": "u32", "batch": n,
           "launches_per_timing": K, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0),
           "both_subtractions_decrypt_equal": same, "comparisons_decrypt_correctly": cmp_ok,
           "values_decrypting_wrongly": {"sub": sub_wrong, "sub_composed_not_add_not": comp_wrong,
                                         "add_alone": add_wrong},
           "legs": {}}
    for name, ts in times.items():
        med = statistics.median(ts)
        res["legs"][name] = {"ms_per_call_median": med, "ms_per_call_min": min(ts),
                             "ms_per_call_rounds": ts, "values_per_s_median": n / (med * 1e-3),
                             "out_bytes_per_value": out_bytes[name]}
    s, c = res["legs"]["sub"], res["legs"]["sub_composed_not_add_not"]
    res["sub_over_composed_median"] = s["ms_per_call_median"] / c["ms_per_call_median"]
    res["sub_no_slower_than_composed"] = bool(s["ms_per_call_median"] <= c["ms_per_call_median"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not same:
        print(f"the two subtractions decrypt differently: {sub_wrong} values of the dedicated one "
              f"and {comp_wrong} of the composition differ from a - b", file=sys.stderr)
    if sub_wrong or not cmp_ok or not same:
        sys.exit("decrypted results disagree")


if __name__ == "__main__":
    main()
