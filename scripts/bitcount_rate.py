"""Rates of the bit counts, batch 4096, on one MI355X.

Two shapes, each leg captured as a graph of LAUNCHES back-to-back calls into a preallocated output
and timed by device events around one replay, after warm-up replays; the legs alternate over
ROUNDS rounds in one process (so clock and thermal drift hit all alike) and the median and the
minimum of the rounds are reported:
  - u32 at (128,128,1,128): hm_bitcount_batch(COUNT_ONES) and (LEADING_ZEROS).  Nothing else
    computes these functions at 32 bits: the figures stand alone.
  - u8 at (64,64,1,64): the same two ops against hm_lookup_batch with the same function's
    256-entry table, the way a caller had before; the ratio op / lookup is reported.
With each leg go the updates its circuit takes per value and the products among them (the others
multiply by the unit polynomial: an XOR or a copy).  All results of every leg are decrypted and
checked against int.bit_count and a bit scan; the script writes the JSON and exits non-zero when
any value disagrees.  "library" in the JSON names the engine library that ran: a variant build is
timed by running this script once more with HOMOMORPH_GPU_LIB naming it and another --out
(profiles/bitcount/rates_per_output_bit.json is such a run).

usage: bitcount_rate.py [--out profiles/bitcount/rates.json] [--n 4096] [--launches 20]
                        [--rounds 7]
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

SHAPES = {"u32": ((128, 128, 1, 128), np.uint32), "u8": ((64, 64, 1, 64), np.uint8)}


def needed(n, i, j):
    T = 1
    while T <= n:
        if j <= T and T - j <= n - i:
            return True
        T <<= 1
    return False


def work(op, n):
    """(updates, products) per value: engine.h bitcount_needed, restated."""
    if op is H.HomomorphicLeadingZeros:
        return n, n - 1
    live = [(i, j) for i in range(1, n + 1) for j in range(1, i + 1) if needed(n, i, j)]
    return len(live), sum(j >= 2 for _, j in live)


def reference(op, v):
    n = 8 * v.dtype.itemsize
    if op is H.HomomorphicCountOnes:
        return np.array([int(x).bit_count() for x in v], np.uint8)
    return np.array([n - int(x).bit_length() for x in v], np.uint8)  # leading zeros


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bitcount", "rates.json"))
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    n, K = args.n, args.launches
    ops = {"count_ones": H.HomomorphicCountOnes, "leading_zeros": H.HomomorphicLeadingZeros}

    legs, outs, want, info, ctxs = {}, {}, {}, {}, {}
    for shape, (params, dtype) in SHAPES.items():
        ctx = H.Context(H.Parameters(*params), device="cuda:0")
        ctx.seed_rng(11)
        ctx.generate_secret_key()
        ctx.generate_public_key()
        rng = np.random.default_rng(3)
        v = rng.integers(0, np.iinfo(dtype).max, size=n, dtype=dtype, endpoint=True)
        v[:4] = [0, np.iinfo(dtype).max, 1, 1 << (8 * v.dtype.itemsize - 1)]
        a = ctx.encrypt(v)
        nbits = a.nbits
        for name, op in ops.items():
            key = f"{name}_{shape}"
            out = H.Ciphered.empty(n, H.bitcount_out_bounds(op, a.bound), ctx.device,
                                   np.dtype(np.uint8))
            legs[key] = (lambda ctx=ctx, op=op, a=a, out=out: H.bitcount_into(ctx, op, a, out))
            outs[key], want[key], ctxs[key] = out, reference(op, v), ctx
            u, p = work(op, nbits)
            info[key] = {"updates_per_value": u, "products_per_value": p,
                         "out_bytes_per_value": out.stride * 8}
            if shape != "u8":
                continue
            table = np.array([reference(op, np.array([x], np.uint8))[0] for x in range(256)], np.uint8)
            key = f"lookup_{name}_u8"
            lout = H.Ciphered.empty(n, H.lookup_out_bounds(a.bound, table), ctx.device,
                                    np.dtype(np.uint8))
            legs[key] = (lambda ctx=ctx, a=a, t=table, out=lout: H.lookup_into(ctx, a, t, out))
            outs[key], want[key], ctxs[key] = lout, reference(op, v), ctx
            info[key] = {"out_bytes_per_value": lout.stride * 8}

    for key, fn in legs.items():  # code objects, and the decrypt tables (a context that builds one
        fn()                      # replaces a buffer, which a captured graph may not outlive)
        ctxs[key].decrypt(outs[key])
    graphs = {}
    for key, fn in legs.items():
        graphs[key] = ctxs[key].graph(lambda fn=fn: [fn() for _ in range(K)])
    for key, g in graphs.items():  # warm-up; the outputs start from -1: the replays write them
        outs[key].limbs.fill_(-1)
        outs[key].degree.fill_(-1)
        torch.cuda.synchronize()
        for _ in range(2):
            g.replay()
        ctxs[key].synchronize()

    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for key, g in graphs.items():
            ctx = ctxs[key]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(ctx.stream):
                e0.record(ctx.stream)
                g.replay()
                e1.record(ctx.stream)
            ctx.synchronize()
            times[key].append(e0.elapsed_time(e1) / K)

    wrong = {k: int((ctxs[k].decrypt(outs[k]) != want[k]).sum()) for k in legs}
    res = {"script": "scripts/bitcount_rate.py", "shapes": {k: list(p) for k, (p, _) in SHAPES.items()},
           "batch": n, "launches_per_graph": K, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "library": os.path.basename(H._lib.LIB_PATH),
           "values_checked_per_leg": n, "values_decrypting_wrongly": wrong, "legs": {}}
    for key, ts in times.items():
        med = statistics.median(ts)
        res["legs"][key] = dict(info[key], ms_per_call_median=med, ms_per_call_min=min(ts),
                                ms_per_call_rounds=ts, values_per_s_median=n / (med * 1e-3))
    res["u8_over_lookup_median"] = {
        name: res["legs"][f"{name}_u8"]["ms_per_call_median"]
        / res["legs"][f"lookup_{name}_u8"]["ms_per_call_median"] for name in ops}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    if any(wrong.values()):
        sys.exit("decrypted results disagree with the integer reference")


if __name__ == "__main__":
    main()
