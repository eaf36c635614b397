"""Rates of the oblivious array read and write, batch 4096, on one MI355X.

Every leg runs at (128,128,1,128) under a fresh u8 index, captured as a graph of LAUNCHES
back-to-back calls into preallocated outputs and timed by device events around one replay, after
two warm-up replays; the legs alternate over ROUNDS rounds in one process (so clock and thermal
drift hit all alike) and the median and the minimum of the rounds are reported:
  - read_u8x16, read_u8x16_shared: hm_array_read_batch of 16 u8 elements, one array per value and
    one shared table;
  - read_u32x16: the same with u32 elements; read_u8x256_shared: a 256-entry shared table;
  - write_u8x16, write_u32x16: hm_array_write_batch;
  - select_tree_u8x16: what a caller had before for the u8 x 16 read, a tree of 15
    hm_select_batch launches over the 16 elements as batches of their own, on conditions packed
    beforehand from the index bits (one call = the 15 launches).
With each leg go the products a value takes at most and the bytes a value reads and writes.  All
results of every leg are decrypted and checked against numpy indexing after the timing; the script
writes the JSON and exits non-zero when any value disagrees.

usage: array_rate.py [--out profiles/array/rates.json] [--n 4096] [--launches 20] [--rounds 7]
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


def read_products(nbits, count):
    k = (count - 1).bit_length()
    return nbits * sum(-(-count // (1 << t)) for t in range(1, k + 1))


def write_products(nbits, count):
    k = (count - 1).bit_length()
    c = k - 1
    for v in range(1, count):
        top = (v & -v).bit_length() - 1
        c += top + 1 - (top == k - 1)
    return c + nbits * count


def condition(idx, t):
    """Bit t of every index value as a Ciphered<bool> (bits 1..7 null): a copy."""
    n, cap = idx.n, int(H.caps(idx.bound)[t])
    off = int(H.caps(idx.bound)[:t].sum())
    limbs = torch.cat([idx.limbs.view(n, idx.stride)[:, off:off + cap],
                       torch.zeros((n, 7), dtype=idx.limbs.dtype, device=idx.limbs.device)], dim=1)
    deg = torch.cat([idx.degree[:, t:t + 1],
                     torch.zeros((n, 7), dtype=idx.degree.dtype, device=idx.degree.device)], dim=1)
    bound = np.array([idx.bound[t]] + [0] * 7, np.uint32)
    return H.Ciphered(limbs.reshape(-1).contiguous(), deg.contiguous(), bound, 8, n, np.dtype(np.bool_))


def element(arr, count, v):
    """Element v of every array as a batch of its own: a copy."""
    n = arr.n // count
    limbs = arr.limbs.view(n, count, arr.stride)[:, v].reshape(-1).contiguous()
    deg = arr.degree.view(n, count, arr.nbits)[:, v].contiguous()
    return H.Ciphered(limbs, deg, arr.bound, arr.nbits, n, arr.plain_dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "array", "rates.json"))
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    n, K = args.n, args.launches

    ctx = H.Context(H.Parameters(*PARAMS), device="cuda:0")
    ctx.seed_rng(11)
    ctx.generate_secret_key()
    ctx.generate_public_key()
    rng = np.random.default_rng(3)
    iv = rng.integers(0, 255, size=n, dtype=np.uint8, endpoint=True)
    iv[:4] = [0, 15, 255, 16]
    idx = ctx.encrypt(iv)
    rows = np.arange(n)

    legs, outs, want, info = {}, {}, {}, {}

    def bytes_of(*batches):
        return int(sum(b.stride * 8 * b.n for b in batches) // n)

    def add_read(key, dtype, count, shared):
        top = np.iinfo(dtype).max
        av = rng.integers(0, top, size=count * (1 if shared else n), dtype=dtype, endpoint=True)
        arr = ctx.encrypt(av)
        out = H.Ciphered.empty(n, H.array_read_out_bounds(arr.bound, count, idx.bound), ctx.device,
                               np.dtype(dtype))
        legs[key] = lambda: H.array_read_into(ctx, arr, idx, count, out)
        sel = iv.astype(np.int64) & ((1 << (count - 1).bit_length()) - 1)
        outs[key] = out
        want[key] = av[sel] if shared else av.reshape(n, count)[rows, sel]
        info[key] = {"products_per_value": read_products(arr.nbits, count), "launches_per_call": 1,
                     "bytes_read_per_value": bytes_of(idx) + (arr.stride * 8 * count),
                     "bytes_written_per_value": bytes_of(out)}
        return arr, av

    def add_write(key, dtype, count):
        top = np.iinfo(dtype).max
        av = rng.integers(0, top, size=count * n, dtype=dtype, endpoint=True)
        xv = rng.integers(0, top, size=n, dtype=dtype, endpoint=True)
        arr, val = ctx.encrypt(av), ctx.encrypt(xv)
        out = H.Ciphered.empty(count * n, H.array_write_out_bounds(arr.bound, val.bound, count,
                                                                   idx.bound),
                               ctx.device, np.dtype(dtype))
        legs[key] = lambda: H.array_write_into(ctx, arr, idx, val, count, out)
        w = av.reshape(n, count).copy()
        w[rows, iv.astype(np.int64) & (count - 1)] = xv
        outs[key], want[key] = out, w.reshape(-1)
        info[key] = {"products_per_value": write_products(arr.nbits, count), "launches_per_call": 1,
                     "bytes_read_per_value": bytes_of(idx, val, arr),
                     "bytes_written_per_value": bytes_of(out)}

    arr8, av8 = add_read("read_u8x16", np.uint8, 16, False)
    add_read("read_u8x16_shared", np.uint8, 16, True)
    add_read("read_u32x16", np.uint32, 16, False)
    add_read("read_u8x256_shared", np.uint8, 256, True)
    add_write("write_u8x16", np.uint8, 16)
    add_write("write_u32x16", np.uint32, 16)

    # the composed tree over the same arrays and index: level t pairs its nodes on condition t
    conds = [condition(idx, t) for t in range(4)]
    level = [element(arr8, 16, v) for v in range(16)]
    steps, read_b, written_b = [], 0, 0
    for t in range(4):
        nxt = []
        for p in range(0, len(level), 2):
            lo, hi = level[p], level[p + 1]
            o = H.Ciphered.empty(n, H.select_out_bounds(conds[t].bound[0], hi.bound, lo.bound),
                                 ctx.device, np.dtype(np.uint8))
            steps.append((conds[t], hi, lo, o))
            read_b += bytes_of(conds[t], hi, lo)
            written_b += bytes_of(o)
            nxt.append(o)
        level = nxt
    legs["select_tree_u8x16"] = lambda: [H.select_into(ctx, c, a, b, o) for c, a, b, o in steps]
    outs["select_tree_u8x16"], want["select_tree_u8x16"] = level[0], want["read_u8x16"]
    info["select_tree_u8x16"] = {"products_per_value": 8 * 15, "launches_per_call": len(steps),
                                 "bytes_read_per_value": read_b, "bytes_written_per_value": written_b}

    for key, fn in legs.items():  # code objects, and the decrypt tables (a context that builds one
        fn()                      # replaces a buffer, which a captured graph may not outlive)
        ctx.decrypt(outs[key])
    graphs = {key: ctx.graph(lambda fn=fn: [fn() for _ in range(K)]) for key, fn in legs.items()}
    for key, g in graphs.items():  # warm-up; the outputs start from -1: the replays write them
        outs[key].limbs.fill_(-1)
        outs[key].degree.fill_(-1)
        torch.cuda.synchronize()
        for _ in range(2):
            g.replay()
        ctx.synchronize()

    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for key, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(ctx.stream):
                e0.record(ctx.stream)
                g.replay()
                e1.record(ctx.stream)
            ctx.synchronize()
            times[key].append(e0.elapsed_time(e1) / K)

    wrong = {k: int((ctx.decrypt(outs[k]) != want[k]).sum()) for k in legs}
    tree_eq = bool(torch.equal(outs["select_tree_u8x16"].limbs, outs["read_u8x16"].limbs) and
                   torch.equal(outs["select_tree_u8x16"].degree, outs["read_u8x16"].degree))
    res = {"script": "scripts/array_rate.py", "parameters": list(PARAMS), "batch": n,
           "launches_per_graph": K, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "library": os.path.basename(H._lib.LIB_PATH),
           "values_checked_per_leg": {k: int(want[k].size) for k in legs},
           "values_decrypting_wrongly": wrong,
           "select_tree_equals_read_limb_for_limb": tree_eq, "legs": {}}
    for key, ts in times.items():
        med = statistics.median(ts)
        res["legs"][key] = dict(info[key], ms_per_call_median=med, ms_per_call_min=min(ts),
                                ms_per_call_max=max(ts), ms_per_call_rounds=ts,
                                values_per_s_median=n / (med * 1e-3))
    res["read_u8x16_over_select_tree_median"] = (res["legs"]["read_u8x16"]["ms_per_call_median"]
                                                 / res["legs"]["select_tree_u8x16"]["ms_per_call_median"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    if any(wrong.values()) or not tree_eq:
        sys.exit("results disagree with the integer reference")


if __name__ == "__main__":
    main()
