// Host-only census of one adder plan (add_host.h), under ASan/UBSan: the planner header is
// compiled into this driver and nothing else is linked, no hm_ctx and no GPU.  Built by
// tests/sanitize/Makefile, run by tests/synth.py add_census (the full-bounds tier's add path
// assertions and tests/test_add_plans.py read the planner's own output).
//
//   add_census L n add_chain fp4  a_0 .. a_{L-1}  b_0 .. b_{L-1}
//
// prints one JSON object: "status" (hm_status of plan_add) and, when it is HM_OK, every plan field
// of AddArgs plus the prep and chain instance launch_add_prep / launch_add_chain_* (adder.hip,
// adder_mfma.hip) would pick for it: only their comparisons are restated here, each beside the
// line it restates.
#include "../../homomorph-rust_amd/csrc/add_host.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

// launch_add_prep (adder.hip:547-564), HM_PREP_FIXED at its default 0: `a.ucap == 5 && a.vpw <= 1`
// -> add_prep_uniform_kernel<5>, `a.ucap` -> none (the launch fails), `a.vpw > 1 && a.top1`,
// `a.vpw > 1`, `a.top1` -> add_prep_kernel<0, 0, TOP1, VPW>
static const char *prep_instance(const hm::AddArgs &a) {
    if (a.ucap == 5 && a.vpw <= 1) return "add_prep_uniform_kernel<5>";
    if (a.ucap) return "";
    if (a.vpw > 1 && a.top1) return "add_prep_kernel<0,0,true,true>";
    if (a.vpw > 1) return "add_prep_kernel<0,0,false,true>";
    if (a.top1) return "add_prep_kernel<0,0,true>";
    return "add_prep_kernel<0,0>";
}

// launch_add (adder.hip:581): `a.mfma` -> launch_add_chain_mfma (adder_mfma.hip:541-544), the
// instance of that chunk count or none; else launch_add_chain_valu (adder.hip:589-607):
// need = ceil(max_prod_words / 64) picks WM of 4, 8, 12, 16, 24, `a.staged` the staged kernel,
// else add_chain_kernel<WM, pad>
static std::string chain_instance(const hm::AddArgs &a) {
    if (a.mfma) {
        if (a.mfma == hm::MfmaCfg<7>::kChunks || a.mfma == hm::MfmaCfg<13>::kChunks ||
            a.mfma == hm::MfmaCfg<25>::kChunks)
            return "add_chain_mfma_kernel<" + std::to_string(a.mfma) + ">";
        return "";
    }
    const uint32_t need = (a.max_prod_words + 63) / 64;
    const std::string wm = need <= 4 ? "4" : need <= 8 ? "8" : need <= 12 ? "12" : need <= 16 ? "16" : "24";
    if (a.staged) return "add_chain_staged_kernel<" + wm + ">";
    return "add_chain_kernel<" + wm + (a.pad ? ",true>" : ",false>");
}

int main(int argc, char **argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: add_census L n add_chain fp4 a[L] b[L]\n");
        return 2;
    }
    hm::AddShape S{};
    S.nbits = (uint32_t)std::strtoul(argv[1], nullptr, 10);
    S.n = std::strtoull(argv[2], nullptr, 10);
    S.add_chain = (uint32_t)std::strtoul(argv[3], nullptr, 10);
    S.fp4_mfma = std::atoi(argv[4]) != 0;
    // (what hm_add_batch has checked before it plans: check_batch, hm_ctx_set_add_options, n > 0)
    if (S.nbits == 0 || S.nbits > HM_MAX_BITS || S.n == 0 || S.add_chain > HM_ADD_CHAIN_VALU ||
        argc != 5 + 2 * (int)S.nbits) {
        std::fprintf(stderr, "add_census: expected n > 0, a chain option and 2 L = %u bounds\n",
                     2 * S.nbits);
        return 2;
    }
    std::vector<uint32_t> ab, bb;
    for (uint32_t i = 0; i < S.nbits; ++i) ab.push_back((uint32_t)std::strtoul(argv[5 + i], nullptr, 10));
    for (uint32_t i = 0; i < S.nbits; ++i)
        bb.push_back((uint32_t)std::strtoul(argv[5 + S.nbits + i], nullptr, 10));
    S.a = ab.data(), S.b = bb.data();
    hm::AddArgs A{};
    const hm_status st = hm::plan_add(S, A);
    std::printf("{\"status\": %d", (int)st);
    if (st == HM_OK) {
        std::printf(", \"cntA\": %u, \"cntB\": %u, \"cntAB\": %u, \"cntP\": %u, \"cntX\": %u, \"top1\": %u,\n"
                    " \"wpv\": %u, \"vpw\": %u, \"lgL\": %u, \"ucap\": %u, \"prep_lds\": %u, \"pad\": %u,\n"
                    " \"cw\": %u, \"staged\": %u, \"chain_lds\": %u, \"max_prod_words\": %u, \"mfma\": %u,\n"
                    " \"mf_cw\": %u, \"ws_stride\": %llu,\n",
                    A.cntA, A.cntB, A.cntAB, A.cntP, A.cntX, A.top1, A.wpv, A.vpw, A.lgL, A.ucap,
                    A.prep_lds, A.pad, A.cw, A.staged, A.chain_lds, A.max_prod_words, A.mfma, A.mf_cw,
                    (unsigned long long)A.ws_stride);
        std::printf(" \"prep_instance\": \"%s\", \"chain_instance\": \"%s\"", prep_instance(A),
                    chain_instance(A).c_str());
    }
    std::printf("}\n");
    return 0;
}
