// Host-only account of the shifter's plans (shift_host.h), under ASan/UBSan: the planner header is
// compiled into this driver and nothing else is linked, no hm_ctx and no GPU.  Built and run by
// tests/test_shift_host.py (g++ -std=c++17 -fsanitize=address,undefined), as its own process.
//
//   shift_plan [which is_signed nbits a_0 .. a_{nbits-1} s_0 .. s_{L-1}]      L = log2 nbits
//
// which is the hm_op code (18..21).  Without arguments the cases are read from stdin, one per
// line in the same form.  Every case prints one JSON object: "status" (hm_status of the bounds,
// then of plan_shift), the output bounds, the source map of every stage ("src"[t][i], -1 = the
// null polynomial) and, when the plan fits, the wave's LDS layout.  A last line is the plan of a
// u32 value at bound 20 000 per bit, which exceeds a wave's share of a block's LDS.
#include "../../homomorph-rust_amd/csrc/shift_host.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

// (what hm_shift_batch has checked before it plans)
static bool run_case(const std::vector<std::string> &w) {
    if (w.size() < 3) return false;
    const hm_op which = (hm_op)std::strtoul(w[0].c_str(), nullptr, 10);
    const bool sgn = std::strtoul(w[1].c_str(), nullptr, 10) != 0;
    const uint32_t nbits = (uint32_t)std::strtoul(w[2].c_str(), nullptr, 10);
    const uint32_t L = hm::shift_plan::stages(nbits);
    if (!hm::shift_plan::is_shift_op(which) || !L || w.size() != 3 + nbits + L) return false;
    std::vector<uint32_t> ab(nbits), sb(L), need(nbits, 0);
    for (uint32_t i = 0; i < nbits; ++i) ab[i] = (uint32_t)std::strtoul(w[3 + i].c_str(), nullptr, 10);
    for (uint32_t t = 0; t < L; ++t)
        sb[t] = (uint32_t)std::strtoul(w[3 + nbits + t].c_str(), nullptr, 10);
    hm::ShiftArgs A{};
    const uint32_t mode = hm::shift_plan::mode_of(which, sgn);
    hm_status st = hm::shift_plan::bounds(which, nbits, ab.data(), sb.data(), need.data());
    if (st == HM_OK) st = hm::plan_shift(mode, nbits, ab.data(), sb.data(), need.data(), A);
    std::printf("{\"status\": %d, \"which\": %d, \"mode\": %u, \"nbits\": %u, \"bounds\": [", (int)st,
                (int)which, mode, nbits);
    for (uint32_t i = 0; i < nbits; ++i) std::printf("%s%u", i ? ", " : "", need[i]);
    std::printf("], \"src\": [");
    for (uint32_t t = 0; t < L; ++t) {
        std::printf("%s[", t ? ", " : "");
        for (uint32_t i = 0; i < nbits; ++i)
            std::printf("%s%d", i ? ", " : "", (int)hm::shift_src(mode, nbits, 1u << t, i));
        std::printf("]");
    }
    std::printf("]");
    if (st == HM_OK) {
        std::printf(", \"L\": %u, \"lds_per_wave\": %u, \"oN\": %u, \"oX\": %u, \"oT\": %u, "
                    "\"oS\": %u, \"oV\": %u, \"cV\": %u, \"soff\": [",
                    A.L, A.lds_per_wave, A.oN, A.oX, A.oT, A.oS, A.oV, A.cV);
        for (uint32_t t = 0; t < L; ++t) std::printf("%s%u", t ? ", " : "", A.soff[t]);
        std::printf("], \"sv\": [");
        for (uint32_t t = 0; t < L; ++t) std::printf("%s%u", t ? ", " : "", A.sv[t]);
        std::printf("], \"off\": [");
        for (uint32_t i = 0; i < nbits; ++i) std::printf("%s%u", i ? ", " : "", A.off[i]);
        std::printf("]");
    }
    std::printf("}\n");
    return true;
}

int main(int argc, char **argv) {
    bool ok = true;
    if (argc > 1) {
        ok = run_case(std::vector<std::string>(argv + 1, argv + argc));
    } else {
        std::string line;
        while (ok && std::getline(std::cin, line)) {
            std::istringstream in(line);
            std::vector<std::string> w;
            for (std::string t; in >> t;) w.push_back(t);
            if (!w.empty()) ok = run_case(w);
        }
    }
    if (!ok) {
        std::fprintf(stderr, "usage: shift_plan [which is_signed nbits a[nbits] s[log2 nbits]]\n");
        return 2;
    }
    // beyond LDS: 32 slots of 6 * 20 000 / 32 words, for four waves
    std::vector<std::string> big = {"18", "0", "32"};
    for (int i = 0; i < 32 + 5; ++i) big.push_back("20000");
    return run_case(big) ? 0 : 1;
}
