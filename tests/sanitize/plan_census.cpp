// Host-only census of one multiplier plan (mul_plan.h), under ASan/UBSan: the planner header is
// compiled into this driver and nothing else is linked, no hm_ctx and no GPU.  Built by
// tests/sanitize/Makefile, run by tests/synth.py mul_census (the full-bounds tier's path assertions
// read the planner's own output, not a restatement of its rules).
//
//   plan_census L K signed ka_min ka_leaf mfma  a_0 .. a_{K-1}  b_0 .. b_{K-1}
//
// prints one JSON object: the plan-level choice of the partial products' launch, and per column
// every launch mul_columns would make with the sizes the kernels are given (runs_ppv, runs_ppg,
// ka_leaf_launch: the functions mul_columns and run_ka call).  "instance" is what launch_mul_ppg /
// launch_mul_mfma (mul_mfma.hip) would pick for the launch: only their umax comparisons are
// restated here.
#include "../../homomorph-rust_amd/csrc/mul_plan.h"

#include <cstdio>
#include <cstdlib>
#include <string>

// launch_mul_ppg: `a.umax <= kMfTinyWords` -> mul_ppg_kernel<kMfTinyChunks>, else
// mul_ppg_kernel<kMfG + 1>
static const char *pp_instance(const hm::MulPlan &P) {
    if (hm::runs_ppv(P)) return "mul_ppv_kernel";
    if (hm::runs_ppg(P)) return P.ppg_umax <= hm::kMfTinyWords ? "mul_ppg_kernel<11>" : "mul_ppg_kernel<17>";
    return "";
}

// launch_mul_mfma, leaf = false: `a.umax <= kMfTinyWords` -> the tiny instance
// <false,true,false,11>, `a.umax <= kMfNarrowWords` -> the narrow one <false,true,false,17,16>,
// `a.lean` -> the windowed wide one <false,true,true>, else <false>
static const char *mf_instance(const hm::MfLaunch &m) {
    if (!m.nspans) return "";
    if (m.umax <= hm::kMfTinyWords) return "tiny";
    if (m.umax <= hm::kMfNarrowWords) return "narrow";
    return m.lean ? "wide_win" : "wide";
}

static void put_launch(const hm::MfLaunch &m) {
    std::printf("{\"nspans\": %u, \"umax\": %u, \"vmax\": %u, \"span\": %u, \"lean\": %d, "
                "\"instance\": \"%s\"}",
                m.nspans, m.umax, m.vmax, m.span, (int)m.lean, mf_instance(m));
}

int main(int argc, char **argv) {
    if (argc < 7) {
        std::fprintf(stderr, "usage: plan_census L K signed ka_min ka_leaf mfma a[K] b[K]\n");
        return 2;
    }
    hm::MulPlan P;
    P.L = (uint32_t)std::strtoul(argv[1], nullptr, 10);
    P.K = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    P.is_signed = std::atoi(argv[3]) != 0;
    P.ka_min = (uint32_t)std::strtoul(argv[4], nullptr, 10);
    P.ka_leaf = (uint32_t)std::strtoul(argv[5], nullptr, 10) & ~31u; // as hm_ctx_set_mul_options
    P.mfma = std::atoi(argv[6]) != 0;
    P.ka_scratch = hm::kKaScratchWords;
    if (P.K == 0 || P.K > P.L || argc != 7 + 2 * (int)P.K) {
        std::fprintf(stderr, "plan_census: expected 2 K = %u bounds\n", 2 * P.K);
        return 2;
    }
    for (uint32_t j = 0; j < P.K; ++j) P.ab.push_back((uint32_t)std::strtoul(argv[7 + j], nullptr, 10));
    for (uint32_t j = 0; j < P.K; ++j)
        P.bb.push_back((uint32_t)std::strtoul(argv[7 + P.K + j], nullptr, 10));
    if (!hm::build_plan(P)) {
        std::fprintf(stderr, "plan_census: build_plan refused the bounds\n");
        return 1;
    }
    std::printf("{\"L\": %u, \"K\": %u, \"signed\": %d, \"mfma\": %d, \"ka_min\": %u, \"ka_leaf\": %u,\n",
                P.L, P.K, (int)P.is_signed, (int)P.mfma, P.ka_min, P.ka_leaf);
    std::printf(" \"ppg\": %d, \"ppv\": %d, \"ppg_umax\": %u, \"ppg_vmax\": %u, \"ppg_span\": %u, "
                "\"astride\": %llu, \"pp_instance\": \"%s\",\n",
                (int)P.ppg, (int)P.ppv, P.ppg_umax, P.ppg_vmax, P.ppg_span,
                (unsigned long long)P.astride, pp_instance(P));
    std::printf(" \"cols\": [\n");
    for (uint32_t i = 0; i < P.K; ++i) {
        const hm::MulPlan::Col &c = P.cols[i];
        // (nitems: the scan's items, which launch_mul_scan stages in LDS; maxwords: its widest prefix)
        std::printf("  {\"npp\": %u, \"nitems\": %u, \"maxwords\": %u, \"ppl\": ", c.npp, c.nitems,
                    c.maxwords);
        put_launch(c.ppl);
        std::printf(",\n   \"nrows\": %u, \"rows_uw\": %u, \"rows_vw\": %u, \"rows_ow\": %u, \"rows_qw\": %u,\n",
                    c.nrows, c.rows_uw, c.rows_vw, c.rows_ow, c.rows_qw);
        std::printf("   \"mfl\": [");
        for (int cl = 0; cl < 3; ++cl) {
            if (cl) std::printf(", ");
            put_launch(c.mfl[cl]);
        }
        std::printf("],\n   \"ntiles\": [");
        for (uint32_t q = 0; q < hm::kNW; ++q) std::printf("%s%u", q ? ", " : "", c.ntiles[q]);
        std::printf("],\n   \"ka\": [");
        for (size_t k = 0; k < c.ka.size(); ++k) {
            const hm::KaProg &pg = c.ka[k];
            hm::MulMfmaArgs leaves{};
            hm::ka_leaf_launch(pg, leaves);
            const bool lean = P.mfma && pg.nvtask && leaves.lean;
            std::printf("%s{\"lane\": %u, \"nvtask\": %u, \"leaf_umax\": %u, \"leaf_vmax\": %u, "
                        "\"leaf_omax\": %u, \"deg\": %d, \"lean_leaf\": %d}",
                        k ? ", " : "", pg.lane, pg.nvtask, pg.leaf_umax, pg.leaf_vmax, pg.leaf_omax,
                        (int)pg.deg, (int)lean);
        }
        std::printf("],\n   \"res_bound\": %lld}%s\n", (long long)P.res_bound[i], i + 1 < P.K ? "," : "");
    }
    std::printf(" ]}\n");
    return 0;
}
