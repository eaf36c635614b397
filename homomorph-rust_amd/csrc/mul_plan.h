// mul_plan.h — the column-parallel carry-save multiplier's planner, host only and header only
// (inline): from the static bounds of an operand pair and the context's multiplier options, the
// whole MulPlan -- slots, task tables, every launch's sizes -- plus the launch parameters that are
// functions of the plan alone and the byte image of its tables.  No HIP call, no hm_ctx: get_plan
// (mul_host.cpp) builds a plan here, uploads the image and caches it; mul_columns / run_ka launch
// from it; hm_mul_out_bounds / hm_mul_cost (capi.cpp) use mul_result_bounds / mul_cost_model;
// tests/sanitize/plan_census.cpp and plan_split.cpp compile this header alone into stand-alone
// drivers.
//
// A plan is the symbolic run of mul_unsigned_internal / mul_signed_internal
// (src/impls/numbers/common.rs:66-155) over static degree bounds: every polynomial the reference
// builds gets a slot (a static offset in a per-value arena of u32 words, capacity from its bound)
// and a degree slot, and every column becomes three launches over the whole batch:
//   partial products  pp_j = a_j * b_{i-j}              (j = 0..i; +1 at the signed corners)
//   prefix scan       p_t = x_0 ^ .. ^ x_{t-1}, result_i = p_n (written to the output bit)
//   carry products    c_t = p_t * x_t                    (t >= 1; column i < K-1 only)
// Items are the column's partial products, then the previous column's carries, in the
// reference's order.  Polynomials that are null by construction (the carry pushed before a
// column's first item: result_i is still zero) are not materialised: XOR with null is the
// identity and a product with null is null, so dropping them changes no output bit.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>

#include "circuit_host.h"

// Karatsuba lanes: a column's Karatsuba products alternate between two scratch regions and two
// streams (the context stream and its auxiliary stream), so one product's HBM-bound operand sums
// and recombinations, and the tail of its leaf launch, overlap the next product's leaves
#ifndef HM_KA_LANES
#define HM_KA_LANES 2
#endif
// the deepest Karatsuba level's operand sums (lo + hi) are not formed in HBM by ka_sum_kernel:
// the MFMA leaves read both halves and XOR them while building their operand images
#ifndef HM_KA_FUSE_SUMS
#define HM_KA_FUSE_SUMS 1
#endif
// schoolbook products whose uniform operand has at least this many words run on the matrix cores
// (mfma plans); narrower ones keep the VALU tiles
#ifndef HM_MF_MIN_WORDS
#define HM_MF_MIN_WORDS 4
#endif
#ifndef HM_PPV
#define HM_PPV 1 // (A/B knob) 0: the partial products on the matrix cores (mul_ppg_kernel) always
#endif
#ifndef HM_ROWS
#define HM_ROWS 1 // (A/B knob) 0: the small products stay in the MFMA tiny class
#endif

namespace hm {

constexpr uint32_t kKaLanes = HM_KA_LANES;
constexpr bool kFuseLeafSums = HM_KA_FUSE_SUMS;
constexpr uint32_t kMfMinWords = HM_MF_MIN_WORDS;
constexpr uint32_t kNW = sizeof(kMulTileW) / sizeof(kMulTileW[0]);
// default Karatsuba scratch limit, words per value and lane (hm_ctx_set_mul_scratch): above it a
// product is planned one subtree at a time (KaProduct::plan); every K <= 20 plan stays below it
constexpr uint64_t kKaScratchWords = 200000000u;

// One Karatsuba product (see "Karatsuba" below): its launches, in order.
struct KaProg {
    uint32_t u, v, out;                          // slots (exact degrees: deg1)
    uint32_t lane = 0;                           // scratch region / stream (mul_columns)
    std::vector<std::array<uint32_t, 3>> sums;   // per level 1..k: (first KaSum, count, h)
    uint32_t vtask = 0, nvtask = 0;              // leaf products (MulVTask range)
    uint32_t leaf_umax = 0, leaf_vmax = 0, leaf_omax = 0; // their largest operands and output
    uint32_t tiles[kNW] = {}, ntiles[kNW] = {};  // their tiles (MulVTile ranges) per width class
    std::vector<std::array<uint32_t, 3>> combs;  // per level k..1: (first KaComb, count, h)
    bool deg = true; // then the product's exact degree (false: a subtree of a split product)
};

// One launch of MFMA products (mul_mfma_kernel<false>): spans of `span` output tiles, the LDS
// slices sized by its largest operands.  A column's schoolbook products are split by the shorter
// operand's size into launches of their own, so the narrow products' small slices are not sized
// for the wide products' (and their spans cover their outputs, not 16 tiles of mostly nothing).
struct MfLaunch {
    uint32_t spans = 0, nspans = 0; // MulTile range in mspans
    uint32_t vmax = 0, umax = 0, span = 0;
    bool lean = false; // wide class on the lean windowed instance
};

struct MulPlan {
    // key
    uint32_t L = 0, K = 0;
    bool is_signed = false;
    uint32_t ka_min = 0, ka_leaf = 0;           // Karatsuba options (hm_ctx_set_mul_options)
    uint64_t ka_scratch = 0;                    // ... and hm_ctx_set_mul_scratch
    bool mfma = false;                          // products on the matrix cores (hm_ctx_set_mul_products)
    std::vector<uint32_t> ab, bb;
    // geometry
    std::vector<MulSlot> slots;
    uint64_t astride = 0; // arena words per value
    std::vector<int64_t> res_bound;
    struct Col {
        uint32_t pp, npp;          // MulPPTask offset / count (in tasks): the VALU partial products
        uint32_t ppm;              // MFMA partial products: MulProdTask offset (ppm list)
        MfLaunch ppl;              // ... their launch
        uint32_t items, nitems;    // u32 offset of the item slot ids
        uint32_t prefix;           // u32 offset of the prefix slot ids (nitems - 1)
        uint32_t res;              // result degree slot
        uint32_t maxwords;         // widest prefix / result
        uint32_t prod;             // MulProdTask offset (in tasks)
        uint32_t tiles[kNW], ntiles[kNW]; // MulTile offsets (in tiles) / counts per width class
        MfLaunch mfl[3];                  // MFMA schoolbook products: tiny, narrow, wide
        uint32_t rows = 0, nrows = 0;     // ... small ones on the VALU by rows (row_tasks range)
        uint32_t rows_uw = 0, rows_vw = 0, rows_ow = 0, rows_qw = 0;
        std::vector<KaProg> ka;           // this column's Karatsuba products
    };
    std::vector<Col> cols;
    std::vector<uint32_t> res_slots;
    // host tables, then one device copy (for_each_table, pack_tables)
    std::vector<MulPPTask> pp;
    std::vector<uint32_t> lists;
    std::vector<MulProdTask> prod;
    std::vector<MulTile> tiles;
    std::vector<MulTile> mspans; // MFMA spans {task, first output word} of the schoolbook products
    std::vector<MulSpanRec> mrecs; // ... resolved (parallel to mspans; built after the regions)
    std::vector<MulProdTask> ppm; // partial products a_j * b_k run on the matrix cores
    std::vector<MulProdTask> row_tasks; // small carry products on the VALU (Col::rows)
    std::vector<MulSpanRec> row_recs;   // ... resolved (built after the regions)
    size_t off_rows = 0;
    // ... or, when every one fits (kMfPPGWords), all of them in one launch before the columns,
    // grouped by a_j (mul_ppg_kernel)
    bool ppg = false;
    std::vector<MulPPGroup> ppg_groups;
    std::vector<MulPPItem> ppg_items;
    uint32_t ppg_umax = 0, ppg_vmax = 0, ppg_span = 0;
    size_t off_ppg_groups = 0, off_ppg_items = 0;
    // ... or on the VALU by rows (mul_ppv_kernel) when every factor fits kPPVWords words: the same
    // items flattened to tasks {a_j slot, b_k slot, out slot}
    bool ppv = false;
    std::vector<MulPPTask> ppv_tasks;
    uint32_t ppv_inw = 0, ppv_outw = 0;
    size_t off_ppv = 0;
    std::vector<KaSum> ka_sums;
    std::vector<MulVTask> ka_vtasks;
    std::vector<MulVTile> ka_vtiles;
    std::vector<KaComb> ka_combs;
    uint8_t *d_tab = nullptr; // the device copy of the tables' image (mul_host.cpp upload_plan)
    size_t tab_bytes = 0;
    size_t off_slots = 0, off_pp = 0, off_lists = 0, off_prod = 0, off_tiles = 0, off_res = 0;
    size_t off_mspans = 0, off_ppm = 0, off_mrecs = 0;
    size_t off_ka_sums = 0, off_ka_vtasks = 0, off_ka_vtiles = 0, off_ka_combs = 0;
    uint64_t work = 0; // word-pair products (statistics)
    std::vector<double> prod_pairs; // per carry product (P.prod): its schoolbook word pairs
};

// ---------------------------------------------------------------------------------------------
// Launch parameters that are functions of the plan alone: each function fills those fields of a
// launch's argument block and leaves the pointers to the caller.  mul_columns / run_ka
// (mul_host.cpp) and the census driver call the same functions.  (Which instance a launch then
// takes by its umax is decided in launch_mul_mfma / launch_mul_ppg, mul_mfma.hip.)

// the MFMA kernels' blocks are four waves' slices and 256 words: four such blocks (16 waves)
// within a CU's 160 KiB of LDS
inline bool mf_blocks_fit_cu(uint32_t wave_words) {
    return (256 + 4 * (size_t)wave_words) * 4 * 4 <= 160 * 1024;
}
// a wave's slice on the lean (windowed) instances, the Karatsuba leaves' and the wide class's:
// the U image is one group's window
constexpr uint32_t mul_mfma_lean_leaf_wave_words(uint32_t vmax, uint32_t span, uint32_t umax) {
    return mf_win_words(kMfG + 1) + mf_vi_words(vmax, span, umax) + 32 * span;
}
// A Karatsuba program's leaves on the matrix cores, one wave per (value, leaf): one span, the
// whole leaf output; the lean instance for leaves of kMfLeanLeafMin .. kMfLeanLeafWords words when
// 16 waves' slices (4 blocks of 4) fit a CU's LDS
inline void ka_leaf_launch(const KaProg &pg, MulMfmaArgs &a) {
    a.span = std::max(1u, (pg.leaf_omax + 31) / 32), a.nspans = 1;
    a.nitems = pg.nvtask;
    a.vmax = pg.leaf_vmax, a.umax = pg.leaf_umax;
    a.wave_words = mf_wave_words(a.vmax, a.span, a.umax);
    const uint32_t lw = mul_mfma_lean_leaf_wave_words(a.vmax, a.span, a.umax);
    if (a.umax <= kMfLeanLeafWords && a.umax >= kMfLeanLeafMin && mf_blocks_fit_cu(lw))
        a.lean = 1, a.wave_words = lw;
}
// one launch of MFMA schoolbook products
inline void mf_launch(const MfLaunch &m, MulMfmaArgs &a) {
    a.nitems = m.nspans, a.span = m.span, a.vmax = m.vmax, a.umax = m.umax, a.lean = m.lean;
    a.wave_words = m.lean ? mul_mfma_lean_leaf_wave_words(a.vmax, a.span, a.umax)
                          : mf_wave_words(a.vmax, a.span, a.umax);
}
// which launch computes the grouped partial products before the columns, if any
inline bool runs_ppv(const MulPlan &P) { return P.ppg && P.ppv && !P.ppv_tasks.empty(); }
inline bool runs_ppg(const MulPlan &P) { return !runs_ppv(P) && P.ppg && !P.ppg_groups.empty(); }
// mul_ppv_kernel: a wave stages the 2 K input slots, then holds every product
inline uint64_t ppv_wave_words(const MulPlan &P) {
    return (uint64_t)2 * P.K * (P.ppv_inw + 1) + (uint64_t)P.ppv_tasks.size() * P.ppv_outw;
}
inline void ppv_launch(const MulPlan &P, MulPPVArgs &v) {
    v.ntasks = (uint32_t)P.ppv_tasks.size();
    v.nin = 2 * P.K, v.inw = P.ppv_inw, v.qw = P.ppg_umax, v.outw = P.ppv_outw;
    v.wave_words = (uint32_t)ppv_wave_words(P);
}
inline void ppg_launch(const MulPlan &P, MulPPGArgs &g) {
    g.ngroups = (uint32_t)P.ppg_groups.size();
    g.umax = P.ppg_umax, g.vmax = P.ppg_vmax, g.span = P.ppg_span;
    g.wave_words = mf_wave_words(g.vmax, g.span, g.umax) + 64 * kMfPPGBatch;
}
// mul_rows_kernel: per task its u, v and product, 2 spare words and 6 of bookkeeping
inline uint64_t rows_wave_words(const MulPlan::Col &c) {
    return (uint64_t)c.nrows * (c.rows_uw + c.rows_vw + c.rows_ow + 2 + 6);
}
inline void rows_launch(const MulPlan::Col &c, MulRowArgs &r) {
    r.ntasks = c.nrows, r.uw = c.rows_uw, r.vw = c.rows_vw, r.ow = c.rows_ow;
    r.qw = std::min(c.rows_qw, c.rows_uw);
    r.wave_words = (uint32_t)rows_wave_words(c);
}

// ---------------------------------------------------------------------------------------------
// The plan's host tables as one byte image: each table at a 16-byte aligned offset, in this order.
template <class Plan, class F> void for_each_table(Plan &P, F f) {
    f(P.off_slots, P.slots), f(P.off_pp, P.pp), f(P.off_lists, P.lists), f(P.off_prod, P.prod);
    f(P.off_rows, P.row_recs), f(P.off_tiles, P.tiles), f(P.off_res, P.res_slots);
    f(P.off_mspans, P.mspans), f(P.off_mrecs, P.mrecs), f(P.off_ppm, P.ppm);
    f(P.off_ppg_groups, P.ppg_groups), f(P.off_ppg_items, P.ppg_items), f(P.off_ppv, P.ppv_tasks);
    f(P.off_ka_sums, P.ka_sums), f(P.off_ka_vtasks, P.ka_vtasks);
    f(P.off_ka_vtiles, P.ka_vtiles), f(P.off_ka_combs, P.ka_combs);
}
template <class T> size_t table_bytes(const std::vector<T> &v) { return v.size() * sizeof(T); }
// sets the plan's offsets and returns the image (at least 16 bytes)
inline std::vector<uint8_t> pack_tables(MulPlan &P) {
    size_t o = 0;
    for_each_table(P, [&](size_t &off, const auto &v) { off = o, o = (o + table_bytes(v) + 15) & ~(size_t)15; });
    std::vector<uint8_t> h(std::max<size_t>(o, 16), 0);
    for_each_table(P, [&](size_t &off, const auto &v) {
        if (!v.empty()) std::memcpy(h.data() + off, v.data(), table_bytes(v));
    });
    return h;
}

namespace mul_plan { // the parts of build_plan

constexpr int64_t kBoundLimit = (int64_t)1 << 30;

inline uint32_t slot_words(int64_t bound) { return ((uint32_t)(bound / 32) + 1 + 3) & ~3u; }

// signed circuit: pp[0][L-1] and pp[L-1][0] get ^1 (common.rs:123-126); at L = 1 both are pp[0][0]
inline bool pp_flip(bool is_signed, uint32_t L, uint32_t i, uint32_t j) {
    if (!is_signed || i != L - 1) return false;
    const int f = (j == 0) + (j == L - 1);
    return f & 1;
}

// the narrowest per-lane VALU tile width (class of kMulTileW) that covers an output in one tile,
// else the widest
inline uint32_t tile_class(uint32_t out_words) {
    for (uint32_t q = 0; q < kNW; ++q)
        if (kMulTileW[q] * 64 >= out_words) return q;
    return kNW - 1;
}

struct Region {
    uint64_t used = 0, max = 0;
    uint64_t base = 0;
};

// ---------------------------------------------------------------------------------------------
// Karatsuba.  A carry product u * v whose shorter operand has at least ka_min words is computed
// as a Karatsuba recursion instead of schoolbook tiles: operands padded to N = leaf * 2^k words
// split into halves lo/hi, the three half-size products z0 = lo_u lo_v, z1 = hi_u hi_v,
// z2 = (lo_u + hi_u)(lo_v + hi_v), and u v = z0 + (z0 + z1 + z2) X^h + z1 X^2h (h = half size).
// Exact over GF(2)[X] (the same polynomial as the reference's bit-serial product,
// polynomial.rs:252-310), 3^k leaf products of leaf x leaf words instead of 4^k.  Every node is
// static (slot capacities are static), so the whole recursion is planned here: views into the
// arena, sums and child results in a scratch region (KA) reused product after product.  A
// subtree whose high halves are all padding (zero) is dropped: z1 = 0.

// Views while planning: (region << 28) | word offset relative to the region (regions are placed
// after the symbolic run); kKaNone stays as is.
constexpr uint32_t kRegShift = 28, kRelMask = (1u << kRegShift) - 1;

struct KaBuild {
    uint32_t ka_region, leaf;
    bool fuse_leaf_sums = false; // the deepest level's sums are read by the leaves (MFMA plans)
    uint64_t top = 0, max = 0; // scratch bump allocator in the KA region (words)
    std::vector<std::vector<KaSum>> sums;   // by split depth
    std::vector<std::vector<KaComb>> combs; // by split depth
    std::vector<MulVTask> leaves;

    uint32_t alloc(uint64_t words) {
        const uint64_t o = top;
        top += (words + 3) & ~(uint64_t)3;
        max = std::max(max, top);
        return (ka_region << kRegShift) | (uint32_t)o;
    }
    void comb(uint32_t lvl, const KaComb &c) {
        if (combs.size() <= lvl) combs.resize(lvl + 1);
        combs[lvl].push_back(c);
    }
    // An operand view (o, len valid words) of a node at depth lvl split at h: its halves, and its
    // sum lo + hi as the z2 child reads it -- lo alone when hi is all padding, lo and hi as two
    // views when the child is a leaf that XORs them itself (fuse), else formed in scratch (a KaSum)
    struct Half {
        uint32_t lo_n, hi_o, hi_n, s_o, s_n;
        uint32_t s2_o = kKaNone, s2_n = 0; // (fused leaf sums) the sum's second view
    };
    Half half(uint32_t lvl, uint32_t o, uint32_t len, uint32_t h, bool fuse) {
        Half x;
        x.lo_n = std::min(len, h);
        x.hi_o = o + h;
        x.hi_n = len > h ? len - h : 0u;
        if (x.hi_n == 0) { // lo + hi = lo: no sum to form
            x.s_o = o, x.s_n = x.lo_n;
        } else if (fuse) { // lo_n = h >= hi_n
            x.s_o = o, x.s_n = x.lo_n, x.s2_o = x.hi_o, x.s2_n = x.hi_n;
        } else {
            x.s_o = alloc(h), x.s_n = h;
            if (sums.size() <= lvl) sums.resize(lvl + 1);
            sums[lvl].push_back({o, len, x.s_o});
        }
        return x;
    }
    // r[0:min(2n, rcap)) = U * V for views u (un valid words), v (vn), both of logical size n
    // u2 / v2 (nu2 / nv2 valid words): a second view XORed into the operand (fused leaf sums)
    void node(uint32_t lvl, uint32_t uo, uint32_t un, uint32_t vo, uint32_t vn, uint32_t n,
              uint32_t r, uint32_t rcap, uint32_t u2 = kKaNone, uint32_t nu2 = 0,
              uint32_t v2 = kKaNone, uint32_t nv2 = 0) {
        if (n == leaf) {
            leaves.push_back({uo, std::min(un, n), vo, std::min(vn, n), r, std::min(2 * n, rcap),
                              u2, std::min(nu2, n), v2, std::min(nv2, n)});
            return;
        }
        const uint32_t h = n / 2;
        if (un <= h && vn <= h) {
            // both high halves are padding: u v = lo_u lo_v (one child, not three); the
            // recombination with z2 = z0, z1 = 0 copies it and zero-fills r above it
            const uint32_t z0 = alloc(2 * h);
            node(lvl + 1, uo, un, vo, vn, h, z0, 2 * h);
            return comb(lvl, {z0, kKaNone, z0, r, rcap});
        }
        // children that are leaves read lo + hi as two views instead of a formed sum
        const bool fuse = fuse_leaf_sums && h == leaf;
        const Half U = half(lvl, uo, un, h, fuse), V = half(lvl, vo, vn, h, fuse);
        const bool has_z1 = U.hi_n && V.hi_n;
        const uint32_t z0 = alloc(2 * h), z2 = alloc(2 * h);
        const uint32_t z1 = has_z1 ? alloc(2 * h) : kKaNone;
        node(lvl + 1, uo, U.lo_n, vo, V.lo_n, h, z0, 2 * h);
        if (has_z1) node(lvl + 1, U.hi_o, U.hi_n, V.hi_o, V.hi_n, h, z1, 2 * h);
        node(lvl + 1, U.s_o, U.s_n, V.s_o, V.s_n, h, z2, 2 * h, U.s2_o, U.s2_n, V.s2_o, V.s2_n);
        comb(lvl, {z0, z1, z2, r, rcap});
    }

    // The root of node(0, ...) without its recursion, for a product planned one subtree at a time:
    // the root's operand sums (sums[0]; always formed, the children are not leaves), its z buffers
    // and its recombination (combs[0]).  Returns the children, each to be planned into its z
    // (2h words) with scratch above this builder's top.
    struct Child {
        uint32_t uo, un, vo, vn, z;
    };
    std::vector<Child> split(uint32_t uo, uint32_t un, uint32_t vo, uint32_t vn, uint32_t n,
                             uint32_t r, uint32_t rcap) {
        const uint32_t h = n / 2;
        std::vector<Child> ch;
        if (un <= h && vn <= h) {
            const uint32_t z0 = alloc(2 * h);
            ch.push_back({uo, un, vo, vn, z0});
            comb(0, {z0, kKaNone, z0, r, rcap});
            return ch;
        }
        const Half U = half(0, uo, un, h, false), V = half(0, vo, vn, h, false);
        const bool has_z1 = U.hi_n && V.hi_n;
        const uint32_t z0 = alloc(2 * h), z2 = alloc(2 * h);
        const uint32_t z1 = has_z1 ? alloc(2 * h) : kKaNone;
        ch.push_back({uo, U.lo_n, vo, V.lo_n, z0});
        if (has_z1) ch.push_back({U.hi_o, U.hi_n, V.hi_o, V.hi_n, z1});
        ch.push_back({U.s_o, U.s_n, V.s_o, V.s_n, z2});
        comb(0, {z0, z1, z2, r, rcap});
        return ch;
    }
};

// Symbolic run.  Slot offsets are first relative to their region (in / pp / prefix / carries of
// even columns / carries of odd columns / ...); regions are placed once their maxima are known.
// The shared state of the steps of build_plan, which calls them in order.
struct PlanBuild {
    enum { IN, PP, PRE, CA, CB, KA, PPA, KA2, NREG };
    struct Item {
        uint32_t slot;
        int64_t bound;
    };
    MulPlan &P;
    Region reg[NREG];
    std::vector<uint8_t> slot_reg;
    std::vector<int64_t> slot_bnd; // each slot's degree bound
    // slots of the partial products a_j * b_k the grouped launch computes (~0u: not grouped)
    std::vector<std::vector<uint32_t>> pp_slot;
    std::vector<Item> prev; // the previous column's carries

    int64_t slot_bound(uint32_t s) const { return std::max<int64_t>(slot_bnd[s], 0); }
    uint32_t words(uint32_t s) const { return P.slots[s].words; }
    uint32_t new_slot(int r, int64_t bound) {
        slot_bnd.push_back(bound);
        const uint32_t w = bound < 0 ? 0u : slot_words(bound);
        P.slots.push_back({(uint32_t)reg[r].used, w});
        slot_reg.push_back((uint8_t)r);
        reg[r].used += w;
        reg[r].max = std::max(reg[r].max, reg[r].used);
        return (uint32_t)P.slots.size() - 1;
    }
    // a slot as a planning view
    uint32_t view(uint32_t slot) const {
        return ((uint32_t)slot_reg[slot] << kRegShift) | P.slots[slot].off;
    }

    // the input slots: a_j -> slot j, b_j -> slot K + j
    explicit PlanBuild(MulPlan &plan) : P(plan), pp_slot(plan.K, std::vector<uint32_t>(plan.K, ~0u)) {
        for (uint32_t j = 0; j < P.K; ++j) new_slot(IN, P.ab[j]);
        for (uint32_t j = 0; j < P.K; ++j) new_slot(IN, P.bb[j]);
    }

    // Step 1.  Grouped partial products: every a_j * b_k (j + k < K) on the matrix cores, all in
    // one launch, when every factor has at most kMfPPGWords words (and at least kMfMinWords); their
    // slots live in a region of their own (PPA), not reused column by column.  The signed
    // corners (+1, column L-1) stay VALU tasks of their column.
    void grouped_pp() {
        const uint32_t K = P.K;
        P.ppg = P.mfma;
        for (uint32_t j = 0; j < K && P.ppg; ++j) {
            const uint32_t wa = (uint32_t)(P.ab[j] / 32 + 1), wb = (uint32_t)(P.bb[j] / 32 + 1);
            if (std::max(wa, wb) > kMfPPGWords || std::min(wa, wb) < kMfMinWords) P.ppg = false;
        }
        if (!P.ppg) return;
        uint32_t omax = 0;
        for (uint32_t j = 0; j < K; ++j) {
            MulPPGroup g{j, (uint32_t)P.ppg_items.size(), 0};
            for (uint32_t k = 0; j + k < K; ++k) {
                if (pp_flip(P.is_signed, P.L, j + k, j)) continue;
                const uint32_t s = new_slot(PPA, (int64_t)P.ab[j] + P.bb[k]);
                pp_slot[j][k] = s;
                P.ppg_items.push_back({K + k, s});
                omax = std::max(omax, words(s));
                P.ppg_vmax = std::max(P.ppg_vmax, (uint32_t)(P.bb[k] / 32 + 1));
            }
            g.count = (uint32_t)P.ppg_items.size() - g.first;
            P.ppg_umax = std::max(P.ppg_umax, (uint32_t)(P.ab[j] / 32 + 1));
            if (g.count) P.ppg_groups.push_back(g);
        }
        P.ppg_span = std::min<uint32_t>(kMfSpan, std::max<uint32_t>(1, (omax + 31) / 32));
        // ... on the VALU by rows when every factor is short
        P.ppv = HM_PPV && std::max(P.ppg_umax, P.ppg_vmax) <= kPPVWords;
        if (!P.ppv) return;
        for (const MulPPGroup &g : P.ppg_groups)
            for (uint32_t it = g.first; it < g.first + g.count; ++it)
                P.ppv_tasks.push_back({g.u, P.ppg_items[it].v, P.ppg_items[it].out, 0u});
        for (uint32_t s = 0; s < 2 * K; ++s) P.ppv_inw = std::max(P.ppv_inw, words(s));
        P.ppv_outw = std::max(omax, P.ppg_umax + P.ppg_vmax + 1);
        // a block's four waves within one CU's LDS, else the MFMA form
        if (!fits_cu_lds(ppv_wave_words(P))) P.ppv = false, P.ppv_tasks.clear();
    }

    // Step 2a.  Column i's partial products a_j * b_{i-j} as items: the grouped launch's slots, or
    // slots of this column with a VALU task (P.pp) or an MFMA task (P.ppm, launch col.ppl) each.
    // False: a bound past the engine's limit.
    bool column_pp(uint32_t i, MulPlan::Col &col, std::vector<Item> &items) {
        const uint32_t K = P.K;
        col.pp = (uint32_t)P.pp.size();
        col.ppm = (uint32_t)P.ppm.size();
        uint32_t ppm_omax = 0;
        for (uint32_t j = 0; j <= i; ++j) {
            const int64_t bnd = (int64_t)P.ab[j] + P.bb[i - j];
            if (bnd > kBoundLimit) return false;
            if (pp_slot[j][i - j] != ~0u) { // computed by the grouped launch
                items.push_back({pp_slot[j][i - j], bnd});
                continue;
            }
            const uint32_t s = new_slot(PP, bnd);
            const bool flip = pp_flip(P.is_signed, P.L, i, j);
            const uint32_t sa = j, sb = K + (i - j);
            const uint32_t wa = words(sa), wb = words(sb);
            // on the matrix cores unless a signed corner (+1) or a narrow operand
            if (P.mfma && !flip && std::min(wa, wb) >= kMfMinWords) {
                P.ppm.push_back(wa <= wb ? MulProdTask{sa, sb, s} : MulProdTask{sb, sa, s});
                col.ppl.vmax = std::max(col.ppl.vmax, std::max(wa, wb));
                col.ppl.umax = std::max(col.ppl.umax, std::min(wa, wb));
                ppm_omax = std::max(ppm_omax, words(s));
            } else {
                P.pp.push_back({sa, sb, s, flip ? 1u : 0u});
            }
            items.push_back({s, bnd});
        }
        col.npp = (uint32_t)P.pp.size() - col.pp;
        // spans of the partial products: their whole (short) outputs, at most kMfSpan tiles
        col.ppl.span = std::min<uint32_t>(kMfSpan, (ppm_omax + 31) / 32);
        col.ppl.spans = (uint32_t)P.mspans.size();
        for (uint32_t t = 0; t < (uint32_t)P.ppm.size() - col.ppm; ++t)
            for (uint32_t base = 0; base < words(P.ppm[col.ppm + t].out); base += 32 * col.ppl.span)
                P.mspans.push_back({t, base});
        col.ppl.nspans = (uint32_t)P.mspans.size() - col.ppl.spans;
        return true;
    }

    // Step 2b.  The walk of common.rs:66-105 over column i's items (its partial products, then the
    // previous column's carries): the prefixes p_t, the carries p_t * x_t into `cur` (carry region
    // creg; none from the last column) and the result's bound.  False: a bound past the limit.
    bool column_walk(uint32_t i, int creg, MulPlan::Col &col, const std::vector<Item> &items,
                     std::vector<Item> &cur) {
        const bool push = i + 1 < P.K;
        col.items = (uint32_t)P.lists.size();
        col.nitems = (uint32_t)items.size();
        for (auto &x : items) P.lists.push_back(x.slot);
        col.prefix = (uint32_t)P.lists.size();
        col.prod = (uint32_t)P.prod.size();
        int64_t pb = -1;          // bound of p_t (the running result before item t)
        uint32_t pslot = 0;       // slot of p_t (t >= 1)
        uint32_t maxw = 0;
        for (size_t t = 0; t < items.size(); ++t) {
            const Item &x = items[t];
            if (push && pb >= 0) { // carries.push(result & x_t) (common.rs:83-87, :93-96)
                const int64_t cbnd = pb + x.bound;
                if (cbnd > kBoundLimit) return false;
                const uint32_t cs = new_slot(creg, cbnd);
                // the operand with fewer words is the uniform one (its bits are the decisions)
                if (words(pslot) <= words(x.slot)) P.prod.push_back({pslot, x.slot, cs});
                else P.prod.push_back({x.slot, pslot, cs});
                P.work += (uint64_t)(pb / 32 + 1) * (uint64_t)(x.bound / 32 + 1);
                P.prod_pairs.push_back((double)(pb / 32 + 1) * (double)(x.bound / 32 + 1));
                cur.push_back({cs, cbnd});
            }
            pb = std::max(pb, x.bound); // result ^= x_t
            maxw = std::max(maxw, slot_words(pb));
            if (t + 1 < items.size()) {
                pslot = new_slot(PRE, pb);
                P.lists.push_back(pslot);
            }
        }
        col.maxwords = maxw;
        col.res = new_slot(PRE, -1); // degree-only slot (the output bit)
        P.res_slots.push_back(col.res);
        P.res_bound[i] = pb;
        return true;
    }

    // Step 3.  Karatsuba for the column's big products (their slots are final now: region offsets
    // are fixed when the regions are placed, so views are recorded relative and fixed up in
    // place_regions).  Returns, per product of the column, whether it is one.
    std::vector<bool> column_karatsuba(MulPlan::Col &col);

    // Step 4.  The column's schoolbook products by class, each class with its tiles or spans: the
    // small ones on the VALU by rows, MFMA spans (tiny / narrow / wide) where the uniform operand
    // has at least kMfMinWords words (mfma plans), the rest grouped by per-lane VALU tile width.
    bool rows_ok(const MulPlan::Col &col, const std::vector<bool> &is_ka, uint32_t k) const {
        const uint32_t uw = words(P.prod[k].u), vw = words(P.prod[k].v);
        return HM_ROWS && P.mfma && !is_ka[k - col.prod] && uw >= kMfMinWords && uw <= kRowsU &&
               vw <= kRowsV;
    }
    void column_schoolbook(MulPlan::Col &col, const std::vector<bool> &is_ka) {
        std::vector<MulTile> byw[kNW];
        std::vector<uint32_t> mfk[3]; // MFMA schoolbook products by class
        uint32_t omax[3] = {0, 0, 0};
        col.rows = (uint32_t)P.row_tasks.size();
        for (uint32_t k = col.prod; k < P.prod.size(); ++k)
            if (rows_ok(col, is_ka, k)) {
                col.rows_uw = std::max(col.rows_uw, words(P.prod[k].u));
                col.rows_qw = std::max(col.rows_qw, (uint32_t)(slot_bound(P.prod[k].u) / 32 + 1));
                col.rows_vw = std::max(col.rows_vw, words(P.prod[k].v));
                col.rows_ow = std::max(col.rows_ow, words(P.prod[k].out));
                ++col.nrows;
            }
        col.rows_ow = std::max(col.rows_ow, col.rows_uw + col.rows_vw + 1);
        // the column's small products on the VALU when a block's four waves' LDS fits one CU
        const bool use_rows = col.nrows && fits_cu_lds(rows_wave_words(col));
        if (!use_rows) col.nrows = 0;
        for (uint32_t k = col.prod; k < P.prod.size(); ++k) {
            if (is_ka[k - col.prod]) continue;
            const uint32_t uw = words(P.prod[k].u), nout = words(P.prod[k].out);
            if (use_rows && rows_ok(col, is_ka, k)) {
                P.row_tasks.push_back(P.prod[k]);
            } else if (P.mfma && uw >= kMfMinWords) {
                const int cl = uw <= kMfTinyWords ? 0 : uw <= kMfNarrowWords ? 1 : 2;
                mfk[cl].push_back(k);
                col.mfl[cl].vmax = std::max(col.mfl[cl].vmax, words(P.prod[k].v));
                col.mfl[cl].umax = std::max(col.mfl[cl].umax, uw);
                omax[cl] = std::max(omax[cl], nout);
            } else {
                const uint32_t wc = tile_class(nout);
                for (uint32_t base = 0; base < nout; base += 64 * kMulTileW[wc])
                    byw[wc].push_back({k - col.prod, base});
            }
        }
        for (int cl = 0; cl < 3; ++cl) {
            MfLaunch &m = col.mfl[cl];
            m.lean = cl == 2 && kMfWideLean;
            m.span = std::min<uint32_t>(cl == 2 ? kMfWideSpan : kMfNarrowSpan,
                                        std::max<uint32_t>(1, (omax[cl] + 31) / 32));
            m.spans = (uint32_t)P.mspans.size();
            for (uint32_t k : mfk[cl])
                for (uint32_t base = 0; base < words(P.prod[k].out); base += 32 * m.span)
                    P.mspans.push_back({k - col.prod, base});
            m.nspans = (uint32_t)P.mspans.size() - m.spans;
        }
        for (uint32_t q = 0; q < kNW; ++q) {
            col.tiles[q] = (uint32_t)P.tiles.size();
            col.ntiles[q] = (uint32_t)byw[q].size();
            P.tiles.insert(P.tiles.end(), byw[q].begin(), byw[q].end());
        }
    }

    // Column i, steps 2 to 4.  The pp and prefix regions are reused column by column, the carries'
    // by parity (a column reads the previous column's while it writes its own).
    bool column(uint32_t i) {
        MulPlan::Col col{};
        const int creg = (i & 1) ? CB : CA;
        reg[PP].used = reg[PRE].used = reg[creg].used = 0;
        std::vector<Item> items, cur;
        if (!column_pp(i, col, items)) return false;
        items.insert(items.end(), prev.begin(), prev.end());
        if (!column_walk(i, creg, col, items, cur)) return false;
        column_schoolbook(col, column_karatsuba(col));
        P.cols.push_back(col);
        prev.swap(cur);
        return true;
    }

    // Step 5.  Place the regions and make the offsets absolute: slots, then the Karatsuba views
    // (region, relative offset) -> arena offset.  False: the arena cannot be placed.
    bool place_regions() {
        for (int r = 0; r < NREG; ++r)
            if (reg[r].max >= (1ull << kRegShift)) return false; // planning views hold 28-bit offsets
        uint64_t base = 0;
        for (int r = 0; r < NREG; ++r) {
            reg[r].base = base;
            base += (reg[r].max + 3) & ~(uint64_t)3;
        }
        if (base >= (1ull << 32)) return false;
        for (size_t s = 0; s < P.slots.size(); ++s) P.slots[s].off += (uint32_t)reg[slot_reg[s]].base;
        auto fix = [&](uint32_t o) -> uint32_t {
            return o == kKaNone ? o : (uint32_t)(reg[o >> kRegShift].base + (o & kRelMask));
        };
        for (auto &t : P.ka_sums) t.src = fix(t.src), t.dst = fix(t.dst);
        for (auto &t : P.ka_vtasks)
            t.u = fix(t.u), t.v = fix(t.v), t.out = fix(t.out), t.u2 = fix(t.u2), t.v2 = fix(t.v2);
        for (auto &t : P.ka_combs) t.z0 = fix(t.z0), t.z1 = fix(t.z1), t.z2 = fix(t.z2), t.r = fix(t.r);
        P.astride = std::max<uint64_t>(base, 4);
        return true;
    }

    // Step 6.  The MFMA spans resolved: every launch's span range of mspans, task indices relative
    // to the column's product list (ppm for the partial products' launch, prod for the carries);
    // and the row products (base: the operands' slot capacities, u | v << 16).
    MulSpanRec span_rec(const MulProdTask &t, uint32_t base) const {
        return MulSpanRec{P.slots[t.u].off, P.slots[t.v].off, P.slots[t.out].off, words(t.out),
                          t.u, t.v, t.out, base};
    }
    void resolve(const MfLaunch &m, const std::vector<MulProdTask> &tasks, uint32_t t0) {
        for (uint32_t i = m.spans; i < m.spans + m.nspans; ++i)
            P.mrecs[i] = span_rec(tasks[t0 + P.mspans[i].task], P.mspans[i].base);
    }
    void resolve_spans() {
        P.mrecs.assign(P.mspans.size(), MulSpanRec{});
        for (const auto &col : P.cols) {
            resolve(col.ppl, P.ppm, col.ppm);
            for (const MfLaunch &m : col.mfl) resolve(m, P.prod, col.prod);
        }
        for (const MulProdTask &t : P.row_tasks)
            P.row_recs.push_back(span_rec(t, words(t.u) | (words(t.v) << 16)));
    }
};

// One Karatsuba product T of a column (leaves of `leaf` words, scratch region and stream `lane`)
// planned into the column's programs.
// A product whose breadth-first recursion needs more scratch than the plan's ka_scratch (words per
// value, per lane; default kKaScratchWords) is planned one subtree at a time: the root's sums and
// z buffers, then each child's own program above them (one after another on the lane's stream,
// reusing the same scratch), then the root's recombination -- recursively.  The planning views
// hold 28-bit word offsets per region, so a breadth-first K = 21 product (3.1e8 words) cannot be
// planned whole; K <= 20 (1.94e8 at most) keeps its one-program plans.
struct KaProduct {
    PlanBuild &B;
    MulPlan::Col &col;
    const MulProdTask T;
    uint32_t leaf, lane, region;
    bool fuse; // KaBuild::fuse_leaf_sums
    std::map<std::array<uint32_t, 3>, uint64_t> memo;

    // the scratch words KaBuild::node allocates for a (n, un, vn) node, without building it
    // (the same recursion, memoised: few distinct operand lengths per depth)
    uint64_t scratch(uint32_t n, uint32_t un, uint32_t vn) {
        if (n == leaf) return 0;
        const auto key = std::array<uint32_t, 3>{n, un, vn};
        if (auto it = memo.find(key); it != memo.end()) return it->second;
        const uint32_t h = n / 2;
        uint64_t s;
        if (un <= h && vn <= h) {
            s = 2ull * h + scratch(h, un, vn);
        } else {
            const uint32_t ulo = std::min(un, h), uhi = un > h ? un - h : 0u;
            const uint32_t vlo = std::min(vn, h), vhi = vn > h ? vn - h : 0u;
            const bool formed = !(fuse && h == leaf);
            s = 4ull * h + (uhi && vhi ? 2ull * h : 0) + (formed && uhi ? h : 0) + (formed && vhi ? h : 0);
            s += scratch(h, ulo, vlo) + (uhi && vhi ? scratch(h, uhi, vhi) : 0) +
                 scratch(h, uhi ? h : ulo, vhi ? h : vlo);
        }
        memo[key] = s;
        return s;
    }

    // one program from a builder rooted at size n: its sums by depth, its leaves, its
    // recombinations bottom-up (deg: the product's exact degree after them)
    void push_prog(const KaBuild &kb, uint32_t n, bool deg) {
        MulPlan &P = B.P;
        KaProg pg;
        pg.u = T.u, pg.v = T.v, pg.out = T.out;
        pg.lane = lane;
        pg.deg = deg;
        for (uint32_t l = 0; l < kb.sums.size(); ++l) {
            if (kb.sums[l].empty()) continue;
            pg.sums.push_back({(uint32_t)P.ka_sums.size(), (uint32_t)kb.sums[l].size(), n >> (l + 1)});
            P.ka_sums.insert(P.ka_sums.end(), kb.sums[l].begin(), kb.sums[l].end());
        }
        pg.vtask = (uint32_t)P.ka_vtasks.size(), pg.nvtask = (uint32_t)kb.leaves.size();
        for (const MulVTask &t : kb.leaves) {
            pg.leaf_umax = std::max(pg.leaf_umax, t.nu);
            pg.leaf_vmax = std::max(pg.leaf_vmax, t.nv);
            pg.leaf_omax = std::max(pg.leaf_omax, t.nout);
        }
        P.ka_vtasks.insert(P.ka_vtasks.end(), kb.leaves.begin(), kb.leaves.end());
        const uint32_t wc = tile_class(2 * leaf);
        pg.tiles[wc] = (uint32_t)P.ka_vtiles.size();
        for (uint32_t t = 0; t < pg.nvtask; ++t)
            for (uint32_t b0 = 0; b0 < 2 * leaf; b0 += 64 * kMulTileW[wc])
                P.ka_vtiles.push_back({t, b0});
        pg.ntiles[wc] = (uint32_t)P.ka_vtiles.size() - pg.tiles[wc];
        for (uint32_t l = (uint32_t)kb.combs.size(); l-- > 0;) {
            if (kb.combs[l].empty()) continue;
            pg.combs.push_back({(uint32_t)P.ka_combs.size(), (uint32_t)kb.combs[l].size(), n >> (l + 1)});
            P.ka_combs.insert(P.ka_combs.end(), kb.combs[l].begin(), kb.combs[l].end());
        }
        B.reg[region].max = std::max(B.reg[region].max, kb.max);
        col.ka.push_back(std::move(pg));
    }

    // u * v (views, logical size n) into r; scratch from `top` up
    void plan(uint32_t uo, uint32_t un, uint32_t vo, uint32_t vn, uint32_t n, uint32_t r,
              uint32_t rcap, uint64_t top, bool deg) {
        if (scratch(n, std::min(un, n), std::min(vn, n)) <= B.P.ka_scratch || n <= 2 * leaf) {
            KaBuild kb{region, leaf};
            kb.fuse_leaf_sums = fuse;
            kb.top = kb.max = top;
            kb.node(0, uo, un, vo, vn, n, r, rcap);
            return push_prog(kb, n, deg);
        }
        KaBuild rb{region, leaf};
        rb.top = rb.max = top;
        const std::vector<KaBuild::Child> ch = rb.split(uo, un, vo, vn, n, r, rcap);
        KaBuild rs = rb; // the root's sums first (no leaves, no recombination)
        rs.combs.clear();
        push_prog(rs, n, false);
        for (const KaBuild::Child &x : ch) plan(x.uo, x.un, x.vo, x.vn, n / 2, x.z, n, rb.top, false);
        rb.sums.clear(); // ... and its recombination last
        push_prog(rb, n, deg);
    }
};

inline std::vector<bool> PlanBuild::column_karatsuba(MulPlan::Col &col) {
    std::vector<bool> is_ka(P.prod.size() - col.prod, false);
    uint32_t nka = 0; // this column's Karatsuba products so far: they alternate lanes
    for (uint32_t k = col.prod; k < P.prod.size() && P.ka_min; ++k) {
        const MulProdTask &T = P.prod[k];
        const uint32_t nu = words(T.u), nv = words(T.v), mx = std::max(nu, nv);
        if (std::min(nu, nv) < P.ka_min) continue;
        uint32_t lk = 0;
        while (((uint64_t)P.ka_leaf << lk) < mx) ++lk;
        if (lk == 0) continue;
        // leaf: the smallest multiple of 32 words with leaf * 2^lk >= max(nu, nv)
        const uint32_t leaf = (((mx + (1u << lk) - 1) >> lk) + 31) & ~31u;
        // two lanes (kKaLanes): products alternate between two scratch regions, so that
        // mul_columns can run consecutive products on two streams
        const uint32_t lane = kKaLanes > 1 ? (nka++ & 1u) : 0u;
        KaProduct ka{*this, col, T, leaf, lane, lane ? (uint32_t)KA2 : (uint32_t)KA,
                     P.mfma && kFuseLeafSums, {}};
        ka.plan(view(T.u), nu, view(T.v), nv, leaf << lk, view(T.out), words(T.out), 0, true);
        is_ka[k - col.prod] = true;
    }
    return is_ka;
}

} // namespace mul_plan

// The plan of P's key fields (L .. bb).  False: a bound past the engine's 2^30 limit, or an arena
// that cannot be placed.
inline bool build_plan(MulPlan &P) {
    mul_plan::PlanBuild b(P);
    b.grouped_pp();
    P.res_bound.assign(P.K, -1);
    for (uint32_t i = 0; i < P.K; ++i)
        if (!b.column(i)) return false;
    if (!b.place_regions()) return false;
    b.resolve_spans();
    return true;
}

// Degree bounds of the K low output bits of the nbits-bit circuit (-1 = always null); false when a
// bound exceeds the engine's 2^30 limit or the arena cannot be placed.  The plan's symbolic walk.
inline bool mul_result_bounds(uint32_t nbits, uint32_t K, const uint32_t *a, const uint32_t *b,
                              bool is_signed, std::vector<int64_t> &res) {
    MulPlan P;
    P.L = nbits, P.K = K, P.is_signed = is_signed;
    P.ab.assign(a, a + K), P.bb.assign(b, b + K);
    if (!build_plan(P)) return false;
    res = P.res_bound;
    return true;
}

// The plan's recursion over bounds only (no slots, no limits): the cost model of hm_mul_cost --
// word-pair products, output bytes, max degree.
inline void mul_cost_model(uint32_t nbits, uint32_t K, const uint32_t *a, const uint32_t *b,
                           double &pairs, double &out_bytes, double &maxdeg) {
    (void)nbits;
    std::vector<double> prev, cur;
    pairs = 0, out_bytes = 0, maxdeg = 0;
    for (uint32_t i = 0; i < K; ++i) {
        std::vector<double> items;
        for (uint32_t j = 0; j <= i; ++j) items.push_back((double)a[j] + (double)b[i - j]);
        items.insert(items.end(), prev.begin(), prev.end());
        const bool push = i + 1 < K;
        cur.clear();
        double pb = -1;
        for (double x : items) {
            if (push && pb >= 0) {
                pairs += (std::floor(pb / 32) + 1) * (std::floor(x / 32) + 1);
                cur.push_back(pb + x);
                maxdeg = std::max(maxdeg, pb + x);
            }
            pb = std::max(pb, x);
            maxdeg = std::max(maxdeg, pb);
        }
        out_bytes += 8 * (std::floor(std::max(pb, 0.0) / 64) + 1);
        prev.swap(cur);
    }
}

} // namespace hm
