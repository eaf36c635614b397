// add_host.h — the fused adder's planner, host only and header only (inline, so every program
// that links capi.o has it without another object): from the static bounds of a batch pair, its
// size and the context's chain option, every plan field of AddArgs.  No HIP call, no hm_ctx, no
// allocation: hm_add_batch (capi.cpp) validates, plans here, then grows the workspace and launches;
// tests/sanitize/add_census.cpp compiles it alone into a stand-alone driver.
#pragma once
#include <algorithm>

#include "ctx.h"

namespace hm {

// All a plan depends on.  plan_add fills every plan field of AddArgs (the slot sizes, the prep's and
// the chain's fields, ws_stride) and leaves the pointers, n, nbits and the bounds to the caller.
// HM_ERR_UNSUPPORTED: no plan fits the LDS, or add_chain asks for an MFMA chain that has none.
struct AddShape {
    uint32_t nbits;
    const uint32_t *a, *b; // per-bit degree bounds of the operands
    uint64_t n;            // values (> 0)
    uint32_t add_chain;    // HM_ADD_CHAIN_* (hm_ctx_set_add_options)
    bool fp4_mfma;         // the device has the fp4 MFMA
};

namespace add_plan { // the three parts of plan_add

inline uint32_t even(uint32_t v) { return (v + 1) & ~1u; }

// Workspace slots (words) from the static bounds: cntA .. cntX, and in max_prod_words the widest
// carry product along the chain (SC).  Returns the largest input bound.
// (hm_add_out_bounds runs the same carry-bound recurrence but needs the carry before the update
// and nothing else of this walk; a shared walker would be a callback template for three lines.)
inline int64_t slot_walk(const AddShape &S, AddArgs &A) {
    const uint32_t L = S.nbits;
    uint32_t cntA = 0, cntB = 0, cntAB = 0, cntP = 0, cntX = 1, SC = 2;
    int64_t maxb = 0; // the largest input bound
    int64_t cb = -1;
    for (uint32_t i = 0; i < L; ++i) {
        const int64_t ba = S.a[i], bb = S.b[i];
        cntA = std::max(cntA, 2 * cap_of(S.a[i]));
        cntB = std::max(cntB, 2 * cap_of(S.b[i]));
        cntX = std::max(cntX, words_of_bound(std::max(ba, bb)));
        maxb = std::max(maxb, std::max(ba, bb));
        if (i + 1 < L) {
            const int64_t x = std::max(ba, bb), ab = ba + bb, p = x + ab;
            cntAB = std::max(cntAB, words_of_bound(ab));
            cntP = std::max(cntP, words_of_bound(p));
            SC = std::max(SC, std::max(words_of_bound(p) + words_of_bound(cb), words_of_bound(ab)) + 2);
            cb = (cb < 0) ? ab : std::max(ab, p + cb);
        }
    }
    // (one bit: no product at all, the slots keep one word; the widest P_i is cntP from here on)
    cntAB = std::max(cntAB, 1u), cntP = std::max(cntP, 1u);
    A.cntA = cntA, A.cntB = cntB, A.cntAB = cntAB, A.cntP = cntP, A.cntX = cntX;
    A.max_prod_words = SC;
    return maxb;
}

// prep: enough waves per value to keep the chip busy, and at least enough that one wave's
// product rows (bits x multiplier words) fit its 64 lanes in two passes (bits are dealt in
// contiguous ranges)
inline hm_status plan_prep(const AddShape &S, int64_t maxb, AddArgs &A) {
    const uint32_t L = S.nbits;
    const uint32_t cntA = A.cntA, cntB = A.cntB, cntAB = A.cntAB, cntP = A.cntP, cntX = A.cntX;
    const uint64_t want = (16384 + S.n - 1) / S.n;
    // (rows_fit: waves per value for one pass of a wave's rows; big batches take two passes
    // per wave -- half the waves: configs[4]'s prep 7.8 -> 5.7 ms per 131,072 adds, the
    // headline's 4 waves per value unchanged, since its `want` is 4 already)
    auto waves = [&](uint32_t rows) { // rows: product rows per bit
        const uint64_t rows_fit = (L + std::max<uint32_t>(1, 64 / rows) - 1) /
                                  std::max<uint32_t>(1, 64 / rows);
        // (never fewer than ceil(L / 64): a wave's range is at most 64 bits -- a u128 add with
        // one row per bit at a big batch asked for 1)
        return (uint32_t)std::max<uint64_t>(
            (L + 63) / 64, std::min<uint64_t>({std::max(want, (rows_fit + 1) / 2), 8, (uint64_t)L}));
    };
    // the top word of every a_i, b_i, x_i holds at most bit 32 (cntX - 1) = maxb: the prep can
    // add its multiples as shifted copies instead of product rows -- worth it when the shorter
    // rows save waves per value or row passes per wave (waves x passes; the headline: 2 passes
    // -> 1 at 4 waves; one wave and one pass per value only pays for the copy passes, +8 us
    // per 65,536 u8 adds)
    const bool t1ok = cntX >= 2 && maxb % 32 == 0;
    // row passes per wave at w waves per value (rows per bit)
    auto passes = [&](uint32_t w, uint32_t rows) { return (((L + w - 1) / w) * rows + 63) / 64; };
    const uint32_t w0 = waves(cntX), w1 = t1ok ? waves(cntX - 1) : w0;
    A.top1 = t1ok && (uint64_t)w1 * passes(w1, cntX - 1) < (uint64_t)w0 * passes(w0, cntX);
    A.wpv = waves(cntX - A.top1);
    // one wave per value already (short values, big batch): several whole values per wave
    // instead when their rows fit one pass (L a power of two: configs[0]'s u8 add, 2 values
    // of 8 bits x 4 rows with the top-word copies; its prep cost is per wave)
    A.vpw = 1, A.lgL = 0;
    if (A.wpv == 1 && (L & (L - 1)) == 0 && S.n >= 16384) {
        const uint32_t rows = cntX - (t1ok ? 1u : 0u);
        const uint32_t v = std::min<uint32_t>(8, 64 / std::max<uint32_t>(1, L * rows));
        if (v >= 2) {
            A.vpw = v, A.top1 = t1ok;
            while ((1u << A.lgL) < L) ++A.lgL;
        }
    }
    // both operands of one bound 64 (CAP - 1), as fresh ciphertexts of d + d' = 64 (CAP - 1)
    // are: the uniform prep (adder.hip add_prep_uniform_kernel), whose slot sizes are
    // compile-time and which always takes the top-word copies, whatever A.top1 says; CAP = 5
    // is the instance built (the headline)
    A.ucap = 0;
    if (A.vpw == 1 && t1ok) {
        const uint32_t ub = S.a[0], cap = cap_of(ub);
        bool uni = cap == 5 && ub == 64 * (cap - 1);
        for (uint32_t i = 0; i < L && uni; ++i) uni = S.a[i] == ub && S.b[i] == ub;
        if (uni && cntA == 2 * cap && cntB == 2 * cap && cntX == 2 * cap - 1 &&
            cntAB == 4 * cap - 3 && cntP == 6 * cap - 5)
            A.ucap = cap;
    }
    const uint32_t bpw = A.vpw > 1 ? A.vpw * L : (L + A.wpv - 1) / A.wpv;
    // (+ 2 bpw: with dAB / dP, stage_ab's bound / offset tables; a wave's range is at most 64 bits)
    if (bpw > 64) return HM_ERR_UNSUPPORTED;
    A.prep_lds = even(bpw * (cntA + cntB + cntX + cntAB + cntP) + 6 * bpw);
    if ((size_t)A.prep_lds * 4 * 4 > 160 * 1024) return HM_ERR_UNSUPPORTED;
    return HM_OK;
}

// chain: a carry buffer holds a whole tile of the widest width instantiated (PAD mode);
// each buffer sits above a zero halo of kHalo words
inline hm_status plan_chain(const AddShape &S, AddArgs &A) {
    const uint32_t L = S.nbits, SC = A.max_prod_words;
    const uint32_t cntAB = A.cntAB, cntP = A.cntP, cntX = A.cntX;
    const uint32_t need_w = (SC + 63) / 64;
    const uint32_t wmax = need_w <= 4 ? 4 : need_w <= 8 ? 8 : need_w <= 12 ? 12 : need_w <= 16 ? 16 : 24;
    // PAD needs one tile per product (need_w <= 24) and one uniform chunk (P within kQBig
    // words) so that window reads stay inside [-kHalo, 64*wmax)
    A.pad = need_w <= 24 && cntP <= 25;
    uint32_t cw = SC;
    if (A.pad) cw = std::max(cw, 64 * wmax);
    A.cw = even(cw);
    // staged chain (PAD only): one in-place carry buffer, and everything the chain reads per bit
    // (x_i, ab_i, P_i, degrees) in LDS, so the loop issues no global loads at all
    const uint32_t staged_lds =
        even(A.cw + kHalo + (L - 1) * (cntP + cntAB) + L * cntX + 2 * L);
    A.staged = A.pad && (size_t)staged_lds * 4 * kAddWavesPerBlock <= 160 * 1024;
    A.chain_lds = A.staged ? staged_lds : even(2 * (A.cw + kHalo) + (L - 1) * cntP);
    if ((size_t)A.chain_lds * 4 * kAddWavesPerBlock > 160 * 1024) return HM_ERR_UNSUPPORTED;
    // MFMA chain (adder_mfma.hip): P_i within 2*kMfmaChunks-1 words, ab_i within 64 words (two
    // tiles), a bit's workspace record (x, P, ab, two degrees) within one 64-lane LDS-DMA; carry
    // bits for every tile plus the 64-word window overhang of the ring fill
    const uint32_t tiles = (SC + 31) / 32;
    const uint32_t mf_cw = 32 * tiles + 64;
    // the smallest chunk count whose plan fits: P_i within 2 NC - 1 words, ab_i within 64
    // words (two tiles), the bit's record within kRecWords, and x_i below 32 words (the
    // kernel XORs x into sum words 0..31 only; words from 32 up are the carry's, stored by the
    // tiles), for the last bit as for every other; LDS (dynamic + the static record stage)
    // for one block
    auto plan = [&](auto cfg) -> uint32_t {
        using Cfg = decltype(cfg);
        const uint32_t lds = Cfg::kHalo + mf_cw + Cfg::kRingWords + Cfg::kRsWords;
        const bool fits = cntP <= 2 * Cfg::kChunks - 1 && cntAB <= 64 && cntX <= 32 &&
                          cntX + cntP + cntAB + 2 <= (uint32_t)Cfg::kRecWords &&
                          (256 + (size_t)lds * kAddWavesPerBlock + Cfg::kStageWords) * 4 <=
                              160 * 1024;
        return fits ? lds : 0u;
    };
    uint32_t nc = 0, lds = 0;
    if ((lds = plan(MfmaCfg<7>{}))) nc = 7;
    else if ((lds = plan(MfmaCfg<13>{}))) nc = 13;
    else if ((lds = plan(MfmaCfg<25>{}))) nc = 25;
    if (!S.fp4_mfma) nc = 0;
    A.mfma = S.add_chain != HM_ADD_CHAIN_VALU ? nc : 0u;
    if (S.add_chain == HM_ADD_CHAIN_MFMA && !nc) return HM_ERR_UNSUPPORTED;
    A.mf_cw = A.mfma ? mf_cw : 0u;
    if (A.mfma) A.chain_lds = lds;
    return HM_OK;
}

// MFMAs the NC-chunk chain issues for one bit whose carry has nc words, P_i np and ab_i nab
// (adder_mfma.hip's tile loop): NC per tile, and with trimming the top tile's bucket of live chunks
// (engine.h chain_trim_bucket).  A null carry or P_i runs no tile.
constexpr uint32_t chain_bit_mfmas(int NC, int nc, int np, int nab, bool trim) {
    if (nc <= 0 || np <= 0) return 0;
    const int tiles = ((nc + np > nab ? nc + np : nab) + 31) >> 5;
    const int top = trim ? chain_trim_bucket(NC, chain_top_live(NC, nc, np, tiles)) : NC;
    return (uint32_t)(NC * (tiles - 1) + top);
}

// ... and for one value over the whole add when every degree is at its static bound (slot_walk's
// carry-bound recurrence); a(i), b(i): the operands' bounds.  top_live, when given, counts the
// bits by their top tile's live chunks (NC + 1 entries).
template <class FA, class FB>
constexpr uint64_t chain_mfma_walk(uint32_t nbits, FA a, FB b, int NC, bool trim, uint32_t *top_live = nullptr) {
    uint64_t count = 0;
    int64_t cb = -1;
    for (uint32_t i = 0; i + 1 < nbits; ++i) {
        const int64_t ba = a(i), bb = b(i);
        const int64_t x = ba > bb ? ba : bb, ab = ba + bb, p = x + ab;
        const int nc = (int)words_of_bound(cb), np = (int)words_of_bound(p), nab = (int)words_of_bound(ab);
        count += chain_bit_mfmas(NC, nc, np, nab, trim);
        if (top_live && nc > 0) ++top_live[chain_top_live(NC, nc, np, ((nc + np > nab ? nc + np : nab) + 31) >> 5)];
        cb = (cb < 0) ? ab : (ab > p + cb ? ab : p + cb);
    }
    return count;
}
inline uint64_t chain_mfma_count(const AddShape &S, int NC, bool trim, uint32_t *top_live = nullptr) {
    return chain_mfma_walk(S.nbits, [&](uint32_t i) { return S.a[i]; }, [&](uint32_t i) { return S.b[i]; }, NC,
                           trim, top_live);
}
// The headline (u32, every bound d + d' = 256): DESIGN.md 4.1's 4,979 MFMAs per value untrimmed,
// 4,860 with the buckets 13, 12, 8, 4 (4,791 if every dead chunk were skipped); configs[0]'s u8
// add at 128 and configs[4]'s u32 add at 512 beside it.
constexpr uint64_t chain_mfma_uniform(uint32_t nbits, uint32_t B, int NC, bool trim) {
    return chain_mfma_walk(nbits, [B](uint32_t) { return B; }, [B](uint32_t) { return B; }, NC, trim);
}
static_assert(chain_mfma_uniform(32, 256, 13, false) == 4979 && chain_mfma_uniform(32, 256, 13, true) == 4860);
static_assert(chain_mfma_uniform(8, 128, 7, false) == 91 && chain_mfma_uniform(8, 128, 7, true) == 83);
static_assert(chain_mfma_uniform(32, 512, 25, false) == 18750 && chain_mfma_uniform(32, 512, 25, true) == 18360);

} // namespace add_plan

inline hm_status plan_add(const AddShape &S, AddArgs &A) {
    const int64_t maxb = add_plan::slot_walk(S, A);
    if (hm_status st = add_plan::plan_prep(S, maxb, A); st) return st;
    if (hm_status st = add_plan::plan_chain(S, A); st) return st;
    A.ws_stride = ((uint64_t)S.nbits * (A.cntAB + A.cntP + 2 + A.cntX) + 63) & ~(uint64_t)63;
    return HM_OK;
}

} // namespace hm
