// mul_host.cpp — the column-parallel carry-save multiplier (mul_engine.hip, mul_mfma.hip) on a
// context: what needs an hm_ctx or HIP.  The plan itself -- the symbolic run of the reference's
// circuit over static bounds, every table and every launch's sizes -- is built by the host-only
// planner mul_plan.h; here plans are uploaded and cached per context, keyed by the operand bounds
// and the context's multiplier options (get_plan), and run (mul_columns: per chunk of values the
// staging, the grouped partial products, then per column partial products, prefix scan and carry
// products, and the final copy-out).  A chunk holds as many values as fit half of the free device
// memory, so on an empty device every batch is one chunk; the chunk loop itself (e0 > 0, a short
// last chunk, an arena last written by another chunk) runs under hm_ctx_set_mul_chunk, a test hook
// (tests/test_gpu_mul_chunks.py).
#include <algorithm>
#include <memory>

#include "ctx.h"
#include "mul_plan.h"

namespace hm {

namespace {

hm_status upload_plan(hm_ctx *c, MulPlan &P) {
    const std::vector<uint8_t> h = pack_tables(P);
    DeviceGuard g(c->device);
    HM_HIP(c, hipStreamSynchronize(c->stream));
    HM_HIP(c, hipMalloc(&P.d_tab, h.size()));
    P.tab_bytes = h.size();
    HM_HIP(c, hipMemcpy(P.d_tab, h.data(), h.size(), hipMemcpyHostToDevice));
    return HM_OK;
}

constexpr size_t kMaxPlans = 8;

hm_status get_plan(hm_ctx *c, uint32_t L, uint32_t K, const uint32_t *ab, const uint32_t *bb,
                   bool is_signed, MulPlan *&out) {
    for (MulPlan *p : c->mul_plans)
        if (p->L == L && p->K == K && p->is_signed == is_signed && p->ka_min == c->ka_min &&
            p->ka_leaf == c->ka_leaf && p->ka_scratch == c->ka_scratch && p->mfma == mul_on_mfma(c) &&
            std::equal(p->ab.begin(), p->ab.end(), ab) && std::equal(p->bb.begin(), p->bb.end(), bb)) {
            out = p;
            return HM_OK;
        }
    auto P = std::make_unique<MulPlan>();
    P->L = L, P->K = K, P->is_signed = is_signed;
    P->ka_min = c->ka_min, P->ka_leaf = c->ka_leaf, P->ka_scratch = c->ka_scratch;
    P->mfma = mul_on_mfma(c);
    P->ab.assign(ab, ab + K), P->bb.assign(bb, bb + K);
    if (!build_plan(*P)) return HM_ERR_UNSUPPORTED;
    if (hm_status st = upload_plan(c, *P); st) {
        if (P->d_tab) (void)hipFree(P->d_tab);
        return st;
    }
    if (c->mul_plans.size() >= kMaxPlans) { // a captured graph may still hold the table: retire it
        MulPlan *old = c->mul_plans.front();
        retire(c, old->d_tab, old->tab_bytes, false);
        delete old;
        c->mul_plans.erase(c->mul_plans.begin());
    }
    out = P.release();
    c->mul_plans.push_back(out);
    return HM_OK;
}

} // namespace

hm_status mul_plan_work(hm_ctx *c, uint32_t nbits, uint32_t K, const uint32_t *a, const uint32_t *b,
                        bool is_signed, double &executed) {
    MulPlan *P = nullptr;
    if (hm_status st = get_plan(c, nbits, K, a, b, is_signed, P); st) return st;
    // carries as the plan runs them: a schoolbook product's word pairs at its static bounds (as
    // hm_mul_cost counts them), a Karatsuba product's leaf products instead (a product's output
    // slot is its own, so it identifies the product)
    executed = 0;
    std::vector<bool> ka(P->slots.size(), false);
    for (const auto &col : P->cols)
        for (const KaProg &pg : col.ka) {
            ka[pg.out] = true;
            for (uint32_t t = pg.vtask; t < pg.vtask + pg.nvtask; ++t)
                executed += (double)P->ka_vtasks[t].nu * (double)P->ka_vtasks[t].nv;
        }
    for (size_t k = 0; k < P->prod.size(); ++k)
        if (!ka[P->prod[k].out]) executed += P->prod_pairs[k];
    return HM_OK;
}

void mul_plans_release(hm_ctx *c) {
    for (MulPlan *p : c->mul_plans) {
        if (p->d_tab) (void)hipFree(p->d_tab);
        delete p;
    }
    c->mul_plans.clear();
}

namespace {

// One chunk of values of a multiply: the plan, its device tables and the chunk's argument base.
struct MulRun {
    hm_ctx *c;
    const MulPlan &P;
    MulBase B;
    template <class T> const T *tab(size_t off) const { return (const T *)(P.d_tab + off); }
};

// the launches of one Karatsuba product: sums by depth, leaf products, recombination bottom-up,
// and the exact output degree
hm_status run_ka(const MulRun &R, const KaProg &pg, hipStream_t st) {
    const MulPlan &P = R.P;
    for (const auto &lv : pg.sums) {
        KaSumArgs a{};
        a.B = R.B, a.t = R.tab<KaSum>(P.off_ka_sums) + lv[0], a.nt = lv[1], a.h = lv[2];
        if (launch_ka_sum(a, st)) return hip_fail(R.c, hipGetLastError());
    }
    if (!pg.nvtask) {
        // (a split product's root sums or recombination: no leaves)
    } else if (P.mfma) {
        // the leaves on the matrix cores: one wave per (value, leaf)
        MulMfmaArgs a{};
        a.B = R.B, a.tasks = R.tab<MulVTask>(P.off_ka_vtasks) + pg.vtask;
        ka_leaf_launch(pg, a);
        if (launch_mul_mfma(a, true, st)) return hip_fail(R.c, hipGetLastError());
    } else {
        for (uint32_t q = 0; q < kNW; ++q) {
            if (!pg.ntiles[q]) continue;
            MulVProdArgs a{};
            a.B = R.B, a.tasks = R.tab<MulVTask>(P.off_ka_vtasks) + pg.vtask;
            a.tiles = R.tab<MulVTile>(P.off_ka_vtiles) + pg.tiles[q], a.ntiles = pg.ntiles[q];
            if (launch_mul_vprod(a, kMulTileW[q], st)) return hip_fail(R.c, hipGetLastError());
        }
    }
    for (const auto &lv : pg.combs) {
        KaCombArgs a{};
        a.B = R.B, a.t = R.tab<KaComb>(P.off_ka_combs) + lv[0], a.nt = lv[1], a.h = lv[2];
        if (launch_ka_comb(a, st)) return hip_fail(R.c, hipGetLastError());
    }
    if (!pg.deg) return HM_OK;
    MulDegArgs d{};
    d.B = R.B, d.u = pg.u, d.v = pg.v, d.out = pg.out;
    if (launch_mul_deg(d, st)) return hip_fail(R.c, hipGetLastError());
    return HM_OK;
}

// the grouped partial products, before the columns: on the VALU by rows, or on the matrix cores
hm_status run_grouped_pp(const MulRun &R) {
    const MulPlan &P = R.P;
    if (runs_ppv(P)) {
        MulPPVArgs v{};
        v.B = R.B, v.tasks = R.tab<MulPPTask>(P.off_ppv);
        ppv_launch(P, v);
        if (launch_mul_ppv(v, R.c->stream)) return hip_fail(R.c, hipGetLastError());
    } else if (runs_ppg(P)) {
        MulPPGArgs g{};
        g.B = R.B;
        g.groups = R.tab<MulPPGroup>(P.off_ppg_groups);
        g.items = R.tab<MulPPItem>(P.off_ppg_items);
        ppg_launch(P, g);
        if (launch_mul_ppg(g, R.c->stream)) return hip_fail(R.c, hipGetLastError());
    }
    return HM_OK;
}

// one launch of MFMA schoolbook products: tasks task0.. of the table at task_off
hm_status run_mf(const MulRun &R, const MfLaunch &m, size_t task_off, uint32_t task0) {
    if (!m.nspans) return HM_OK;
    MulMfmaArgs mf{};
    mf.B = R.B, mf.tasks = R.tab<MulProdTask>(task_off) + task0;
    mf.spans = R.tab<MulTile>(R.P.off_mspans) + m.spans;
    mf.recs = R.tab<MulSpanRec>(R.P.off_mrecs) + m.spans;
    mf_launch(m, mf);
    if (launch_mul_mfma(mf, false, R.c->stream)) return hip_fail(R.c, hipGetLastError());
    return HM_OK;
}

// One column: its own partial products, the prefix scan (its last prefix is output bit `sc.out`),
// then the carry products by class.  sc: the scan's output fields, filled by the caller.
hm_status run_column(const MulRun &R, const MulPlan::Col &col, MulScanArgs sc) {
    hm_ctx *c = R.c;
    const MulPlan &P = R.P;
    MulPPArgs pp{};
    pp.B = R.B, pp.tasks = R.tab<MulPPTask>(P.off_pp) + col.pp, pp.ntasks = col.npp;
    if (launch_mul_pp(pp, c->stream)) return hip_fail(c, hipGetLastError());
    if (hm_status st = run_mf(R, col.ppl, P.off_ppm, col.ppm); st) return st;
    sc.B = R.B;
    sc.items = R.tab<uint32_t>(P.off_lists) + col.items;
    sc.prefix = R.tab<uint32_t>(P.off_lists) + col.prefix;
    sc.nitems = col.nitems;
    sc.res = col.res;
    sc.chunks = (std::max(col.maxwords, 2 * sc.out_cap) + 255) / 256;
    if (launch_mul_scan(sc, c->stream)) return hip_fail(c, hipGetLastError());
    if (col.nrows) {
        MulRowArgs ra{};
        ra.B = R.B, ra.recs = R.tab<MulSpanRec>(P.off_rows) + col.rows;
        rows_launch(col, ra);
        if (launch_mul_rows(ra, c->stream)) return hip_fail(c, hipGetLastError());
    }
    for (const MfLaunch &m : col.mfl)
        if (hm_status st = run_mf(R, m, P.off_prod, col.prod); st) return st;
    for (uint32_t q = 0; q < kNW; ++q) {
        if (!col.ntiles[q]) continue;
        MulProdArgs pr{};
        pr.B = R.B;
        pr.tasks = R.tab<MulProdTask>(P.off_prod) + col.prod;
        pr.tiles = R.tab<MulTile>(P.off_tiles) + col.tiles[q];
        pr.ntiles = col.ntiles[q];
        if (launch_mul_prod(pr, kMulTileW[q], c->stream)) return hip_fail(c, hipGetLastError());
    }
    // Karatsuba products: lane 0 on the context stream, lane 1 on the auxiliary stream
    // (each lane's products one at a time: they share the lane's scratch region); the
    // lanes fork after this column's scan and schoolbook launches (the products read its
    // prefixes) and join before the next column's scan (which reads their carries)
    const bool two = col.ka.size() > 1 && kKaLanes > 1;
    if (two) {
        if (hm_status st = ensure_aux_stream(c); st) return st;
        HM_HIP(c, hipEventRecord(c->ev_fork, c->stream));
        HM_HIP(c, hipStreamWaitEvent(c->aux_stream, c->ev_fork, 0));
    }
    hm_status kst = HM_OK;
    for (const KaProg &pg : col.ka)
        if ((kst = run_ka(R, pg, two && pg.lane ? c->aux_stream : c->stream))) break;
    if (two) {
        // joined on every path, a failed lane's too: no unjoined fork under capture, and
        // no auxiliary-stream work left running behind a caller that syncs c->stream only
        const hipError_t e1 = hipEventRecord(c->ev_join, c->aux_stream);
        const hipError_t e2 = hipStreamWaitEvent(c->stream, c->ev_join, 0);
        if (kst == HM_OK && e1 != hipSuccess) return hip_fail(c, e1);
        if (kst == HM_OK && e2 != hipSuccess) return hip_fail(c, e2);
    }
    return kst;
}

} // namespace

hm_status mul_columns(hm_ctx *c, const hm_batch *a, const hm_batch *b, uint32_t K, bool is_signed,
                      hm_batch *out) {
    const uint32_t L = a->nbits;
    if (b->nbits != L || K == 0 || K > L || out->nbits != K) return HM_ERR_INVALID_ARGUMENT;
    const bool flip = is_signed && K == L; // the signed corners are in column L-1 only
    MulPlan *P = nullptr;
    if (hm_status st = get_plan(c, L, K, a->bound, b->bound, flip, P); st) return st;
    for (uint32_t i = 0; i < K; ++i)
        if (out->bound[i] < (uint32_t)std::max<int64_t>(P->res_bound[i], 0))
            return HM_ERR_INVALID_ARGUMENT;
    if (a->n == 0) return HM_OK;
    // workspace: arena + degree rows, chunked over values to a memory budget
    DeviceGuard g(c->device);
    const uint64_t nslots = P->slots.size();
    const uint64_t per_value = P->astride * 4 + nslots * 4;
    size_t freeb = 0, totalb = 0;
    HM_HIP(c, hipMemGetInfo(&freeb, &totalb));
    const uint64_t budget = std::max<uint64_t>((uint64_t)(freeb + c->mws_bytes) / 2, 1ull << 28);
    uint64_t chunk = std::min<uint64_t>(a->n, budget / per_value);
    if (c->mul_chunk) chunk = std::min(chunk, c->mul_chunk); // (a zero chunk stays refused below)
    if (chunk == 0) return HM_ERR_UNSUPPORTED;
    const uint64_t arena_words = ((P->astride * chunk) + 63) & ~(uint64_t)63;
    HM_HIP(c, grow(c, c->d_mws, c->mws_bytes, (size_t)(arena_words + nslots * chunk) * 4));

    MulRun R{c, *P, MulBase{}};
    MulBase &B = R.B;
    B.arena = c->d_mws;
    B.astride = P->astride;
    B.deg1 = c->d_mws + arena_words;
    B.slots = R.tab<MulSlot>(P->off_slots);
    B.status = c->d_status;
    const BatchArg oa = batch_arg(out);
    std::vector<uint32_t> ooff(K);
    for (uint32_t i = 0, o = 0; i < K; ++i) ooff[i] = o, o += cap_of(out->bound[i]);
    for (uint64_t e0 = 0; e0 < a->n; e0 += chunk) {
        B.e0 = e0;
        B.nv = std::min<uint64_t>(chunk, a->n - e0);
        HM_HIP(c, hipMemsetAsync(B.deg1, 0, (size_t)nslots * B.nv * 4, c->stream));
        MulStageArgs S{};
        S.B = B, S.a = batch_arg(a), S.b = batch_arg(b), S.K = K;
        fill_bounds(S.ab, a), fill_bounds(S.bb, b);
        if (launch_mul_stage(S, c->stream)) return hip_fail(c, hipGetLastError());
        if (hm_status st = run_grouped_pp(R); st) return st;
        for (uint32_t i = 0; i < K; ++i) {
            MulScanArgs sc{};
            sc.out = oa, sc.out_off = ooff[i], sc.out_cap = cap_of(out->bound[i]);
            if (hm_status st = run_column(R, P->cols[i], sc); st) return st;
        }
        MulFinalArgs F{};
        F.B = B, F.res = R.tab<uint32_t>(P->off_res), F.K = K, F.out = oa;
        fill_bounds(F.ob, out);
        if (launch_mul_final(F, c->stream)) return hip_fail(c, hipGetLastError());
    }
    return HM_OK;
}

} // namespace hm
