// Host-only account of the bit counts' plans (bitcount_host.h), under ASan/UBSan: the planner header
// is compiled into this driver and nothing else is linked, no hm_ctx and no GPU.  Built and run by
// tests/test_bitcount_host.py (g++ -std=c++17 -fsanitize=address,undefined), as its own process.
//
//   bitcount_plan [which nbits a_0 .. a_{nbits-1}]
//
// which is the hm_op code (22..27).  Without arguments the cases are read from stdin, one per line
// in the same form.  Every case prints one JSON object: "status" (hm_status of the bounds, then of
// plan_bitcount), the 8 output bounds, the circuit's degree "m", the updates with and without
// those by the unit polynomial, the needed set ("needed"[i - 1] = a string of '0' / '1' for
// j = 1 .. i) and, when the plan fits, the wave's LDS layout.  A last line is the plan of a u64
// count_ones at bound 256 per bit, which exceeds a wave's share of a block's LDS.
#include "../../homomorph-rust_amd/csrc/bitcount_host.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

// (what hm_bitcount_batch has checked before it plans)
static bool run_case(const std::vector<std::string> &w) {
    if (w.size() < 2) return false;
    const hm_op which = (hm_op)std::strtoul(w[0].c_str(), nullptr, 10);
    const uint32_t nbits = (uint32_t)std::strtoul(w[1].c_str(), nullptr, 10);
    if (!hm::bitcount_plan::is_bitcount_op(which) || nbits == 0 || nbits > HM_MAX_BITS ||
        w.size() != 2 + nbits)
        return false;
    std::vector<uint32_t> ab(nbits);
    for (uint32_t i = 0; i < nbits; ++i) ab[i] = (uint32_t)std::strtoul(w[2 + i].c_str(), nullptr, 10);
    uint32_t need[hm::kBitCountOut] = {0};
    hm::BitCountArgs A{};
    hm_status st = hm::bitcount_plan::bounds(which, nbits, ab.data(), need);
    if (st == HM_OK) st = hm::plan_bitcount(which, nbits, ab.data(), A);
    std::printf("{\"status\": %d, \"which\": %d, \"nbits\": %u, \"run\": %d, \"m\": %u, "
                "\"updates\": %u, \"products\": %u, \"bounds\": [",
                (int)st, (int)which, nbits, (int)hm::bitcount_plan::is_run_op(which),
                hm::bitcount_plan::degree_of(which, nbits),
                hm::bitcount_plan::updates(which, nbits, true),
                hm::bitcount_plan::updates(which, nbits, false));
    for (uint32_t k = 0; k < hm::kBitCountOut; ++k) std::printf("%s%u", k ? ", " : "", need[k]);
    std::printf("], \"needed\": [");
    for (uint32_t i = 1; i <= nbits; ++i) {
        std::printf("%s\"", i > 1 ? ", " : "");
        for (uint32_t j = 1; j <= i; ++j) std::printf("%d", (int)hm::bitcount_needed(nbits, i, j));
        std::printf("\"");
    }
    std::printf("]");
    if (st == HM_OK) {
        std::printf(", \"zeros\": %u, \"leading\": %u, \"K\": %u, \"J\": %u, \"diag\": %u, "
                    "\"a_limbs\": %u, \"lds_per_wave\": %u, \"oN\": %u, \"oU\": %u, \"oT\": %u, "
                    "\"oD\": %u, \"cD\": %u, \"oE\": %u, \"off\": [",
                    A.zeros, A.leading, A.K, A.J, A.diag, A.a_limbs, A.lds_per_wave, A.oN, A.oU,
                    A.oT, A.oD, A.cD, A.oE);
        for (uint32_t j = 0; j <= hm::kBitCountMaxSlots; ++j) std::printf("%s%u", j ? ", " : "", A.off[j]);
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
        std::fprintf(stderr, "usage: bitcount_plan [which nbits a[nbits]]\n");
        return 2;
    }
    // beyond LDS: the slots E_1 .. E_32 of a u64 count at bound 256, for four waves
    std::vector<std::string> big = {"22", "64"};
    for (int i = 0; i < 64; ++i) big.push_back("256");
    return run_case(big) ? 0 : 1;
}
