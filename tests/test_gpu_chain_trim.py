"""GPU: the MFMA carry chain's top-tile trimming (adder_mfma.hip HM_CHAIN_TRIM) at the edges of
the live-chunk count L, bit-exact against the CPU oracle.

Each bit's top tile T reaches the carry's nc words with its first
L = ceil((nc + np - 32 T) / 2) chunks only (np: words of P_i; engine.h chain_top_live), and a
kernel that trims runs the tile body of the smallest bucket >= L: 13, 12, 8, 4 chunks at NC = 13,
7, 6, 4, 2 at NC = 7 and 25, 24, 16, 8 at NC = 25 (engine.h chain_trim_lc).  The kernel takes nc
and np from the degrees it tracks, not from the static bounds, so the operands here are synthetic
polynomials (Ciphered.from_host) of chosen degrees: every value draws its own degree per bit, and
L of every (value, bit) is computed on the CPU from the same integers (synth.add_trace), so the
coverage below is a fact about the data and not about the bounds.  The tables are asserted before
anything runs on the GPU.

What a trimmed body can get wrong, and the rows that meet it:
  * the edges of L: every L from 1 to NC occurs in each ladder case, so b - 1, b, b + 1 of every
    bucket boundary b, and 1, 2, NC - 1, NC (NC = 25: 1 to 16, all there are: a top tile holds at
    most 32 words of nc + np);
  * a ring-fill stage whose chunk slot is cut off (the stage then runs after the last MFMA): the
    stages sit after chunks kStage = 1, 4, 7 (NC = 7: 0, 2, 4); "cut" below counts the (value, bit)
    pairs whose bucket ends at or before each stage.  With these buckets NC = 13 cuts stages 1
    and 2 (bucket 4), NC = 7 stages 1 and 2 (bucket 2) and stage 2 alone (bucket 4), NC = 25 none
    (its smallest bucket is 8), and no instance cuts stage 0; the test derives which stages can be
    cut from the bucket table and requires each of those to be cut at least once;
  * the top tile that is also the only tile ("one_tile": bits whose nc + np is at most 32 words;
    the narrow values of each ladder, and the first bits of every add);
  * a carry far below its bound: constant bits, a null operand and add(c, c) on genuine
    ciphertexts (the corners of test_gpu_add_prep_uniform.py), where L follows the tracked carry.

All three chain instances run the same cases.  Which of them trim is the build's choice
(HM_CHAIN_TRIM: the 13- and the 25-chunk chains; DESIGN.md 4.1 "Top-tile trimming" has the
measurements).  The 7-chunk chain lost its A/B and is built untrimmed, so its case runs the
untrimmed kernel and its trimmed bodies are compiled out of the library; they passed this file
once through a variant library with every instance trimmed (scripts/mk_variant.sh trimall
"-DHM_CHAIN_TRIM=7" adder_mfma; HOMOMORPH_GPU_LIB selects it), which the build does not make.
"""
import collections

import numpy as np
import pytest

import borrow_model as bm
import synth
from helpers import as_bytes, assert_batches_equal, keys, masks, plain

pytestmark = pytest.mark.gpu

N = 64  # values per ladder case: 16 blocks of four waves

# name: (NC, nbits, bound, degree range of the wide values, seed)
#   the first 48 values draw every a_i, b_i degree in the range; the last 16 are narrow (degrees
#   1 .. 40: one-tile bits over the whole add, and short P_i).
LADDERS = {
    "nc13": (13, 16, 266, (139, 266), 501),
    "nc7": (7, 16, 138, (40, 138), 502),
    "nc25": (25, 8, 522, (267, 522), 503),
}

# Recorded from the data (synth.add_trace; the test recomputes and compares):
#   live: {L: (value, bit) pairs whose top tile has L live chunks}
#   cut: pairs whose bucket cuts off side stage 0, 1, 2;  one_tile: pairs with a single tile
COVERAGE = {
    "nc13": dict(live={1: 53, 2: 60, 3: 62, 4: 66, 5: 40, 6: 51, 7: 63, 8: 62, 9: 48, 10: 55, 11: 64,
                       12: 59, 13: 213},
                 cut=(0, 241, 241), one_tile=233),
    "nc7": dict(live={1: 38, 2: 54, 3: 54, 4: 47, 5: 53, 6: 61, 7: 589},
                cut=(0, 92, 193), one_tile=337),
    # (a top tile holds at most 32 words of nc + np: L <= 16, and the 25-chunk chain's top tile
    # never runs its buckets 24 and 25)
    "nc25": dict(live={1: 22, 2: 35, 3: 34, 4: 30, 5: 37, 6: 33, 7: 25, 8: 18, 9: 16, 10: 15, 11: 20,
                       12: 15, 13: 22, 14: 29, 15: 16, 16: 17},
                 cut=(0, 0, 0), one_tile=96),
}


def buckets(nc):
    s = (nc - 1) // 3
    return (s, 2 * s, 3 * s, nc)


def stages(nc):
    return (0, 2, 4) if nc <= 8 else (1, 4, 7)


def top_live(nc_chunks, row):
    """(tiles, L) of one add_trace row, as engine.h chain_top_live; None: the bit runs no tile."""
    if not row["nprod"]:
        return None
    tiles = (max(row["nc"] + row["np"], row["nab"]) + 31) // 32
    live = (row["nc"] + row["np"] - 32 * (tiles - 1) + 1) >> 1
    return tiles, min(nc_chunks, max(0, live))


def coverage(nc_chunks, A, B):
    live, cut, one = collections.Counter(), [0, 0, 0], 0
    for a, b in zip(A, B):
        for row in synth.add_trace(a, b):
            tl = top_live(nc_chunks, row)
            if tl is None:
                continue
            tiles, L = tl
            live[L] += 1
            one += tiles == 1
            lc = min(x for x in buckets(nc_chunks) if x >= L)
            for k, st in enumerate(stages(nc_chunks)):
                cut[k] += st >= lc
    return dict(live=dict(sorted(live.items())), cut=tuple(cut), one_tile=one)


def ladder(name):
    """(bounds, A, B) of a ladder case: polynomials of exact, per-value degrees."""
    _, nbits, bound, (lo, hi), seed = LADDERS[name]
    rng = np.random.default_rng(seed)
    A, B = [], []
    for e in range(N):
        l, h = (lo, hi) if e < 48 else (1, 40)
        A.append([synth._exact(rng, int(rng.integers(l, h + 1))) for _ in range(nbits)])
        B.append([synth._exact(rng, int(rng.integers(l, h + 1))) for _ in range(nbits)])
    return synth.uniform(nbits, bound), A, B


@pytest.fixture(scope="module")
def H():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import homomorph
    homomorph.lib()  # loud failure if the engine is not built
    return homomorph


@pytest.mark.parametrize("name", list(LADDERS))
def test_every_live_chunk_count(H, oracle, name):
    """Every L from 1 to NC, every cut-off stage and one-tile bits on the forced MFMA chain of
    each instance, limbs and degree words against the oracle's add."""
    nc_chunks, nbits, _, _, _ = LADDERS[name]
    bound, A, B = ladder(name)
    assert synth.add_plan(bound, bound)["nc"] == nc_chunks
    cov = coverage(nc_chunks, A, B)
    print(name, cov)
    assert cov == COVERAGE[name]
    assert set(range(1, min(nc_chunks, 16) + 1)) == set(cov["live"]), "every L from 1 to min(NC, 16)"
    for k, st in enumerate(stages(nc_chunks)):  # every stage some bucket cuts off is cut off here
        assert (cov["cut"][k] > 0) == any(x <= st for x in buckets(nc_chunks)), (k, st)
    assert cov["one_tile"] > 0

    ctx = H.Context(H.Parameters(*synth.PARAMS))
    la, da = bm.pack(A, bound)
    lb, db = bm.pack(B, bound)
    a = H.Ciphered.from_host(la, da, bound, N, ctx.device, None)
    b = H.Ciphered.from_host(lb, db, bound, N, ctx.device, None)
    ctx.set_add_options("mfma")
    out = ctx.apply2(H.HomomorphicAddition, a, b)
    ctx.synchronize()
    assert np.array_equal(out.bound, synth.add_bounds(bound, bound))
    rl, rd = oracle.add_batch(la, da, bound, lb, db, bound, nbits, N, out.bound)
    gl, gd = out.to_host()
    assert_batches_equal(gl, gd, rl, rd, out.bound, N, f"{name}: MFMA chain vs oracle")


def test_short_carry_follows_the_tracked_degree(H, oracle):
    """Genuine u32 ciphertexts at d = d' = tau = 128 (the 13-chunk chain) whose carries are far
    below their bounds: L must come from the carry the kernel tracks.
      0..7    both operands constants in every bit (null or unit carries)
      8..15   every bit of either operand a constant with probability 1/2
      16..23  a is 0 in every bit (one operand all null), b ordinary
      24..31  a all constants, b ordinary
      32..47  b = a, masks included: add(c, c), x_i null in every bit
      48..63  ordinary fresh values"""
    params = (128, 128, 1, 128)
    seed = 511
    ctx = H.Context(H.Parameters(*params))
    ctx.seed_rng(seed)
    ctx.generate_secret_key()
    ctx.generate_public_key()
    _, pk, _ = keys(*params, seed)
    uni = np.full(32, 256, dtype=np.uint32)
    rng = np.random.default_rng(512)
    a, b = plain(N, np.uint32, 513), plain(N, np.uint32, 514)
    ma, mb = masks(N, 32, 128, 515), masks(N, 32, 128, 516)
    ma[0:8] = 0
    mb[0:8] = 0
    ma[8:16][rng.random((8, 32)) < 0.5] = 0
    mb[8:16][rng.random((8, 32)) < 0.5] = 0
    a[16:24] = 0
    ma[16:32] = 0
    b[32:48], mb[32:48] = a[32:48], ma[32:48]
    a[0], b[0] = 0xFFFFFFFF, 0xFFFFFFFF
    a[1], b[1] = 0, 0
    ctx.set_add_options("mfma")
    s = ctx.apply2(H.HomomorphicAddition, ctx.encrypt(a, masks=ma, bound=uni),
                   ctx.encrypt(b, masks=mb, bound=uni))
    dec = ctx.decrypt(s)
    ctx.synchronize()
    la, da = oracle.encrypt_batch(pk, as_bytes(a), ma, uni)
    lb, db = oracle.encrypt_batch(pk, as_bytes(b), mb, uni)
    rl, rd = oracle.add_batch(la, da, uni, lb, db, uni, 32, N, s.bound)
    gl, gd = s.to_host()
    assert_batches_equal(gl, gd, rl, rd, s.bound, N, "short carries: MFMA chain vs oracle")
    assert np.array_equal(dec, (a + b).astype(np.uint32))
