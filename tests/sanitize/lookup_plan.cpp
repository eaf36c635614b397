// Host-only account of table-lookup plans (lookup_host.h), under ASan/UBSan: the planner header is
// compiled into this driver and nothing else is linked, no hm_ctx and no GPU.  Built and run by
// tests/test_lookup_host.py (g++ -std=c++17 -fsanitize=address,undefined), as its own process.
//
//   lookup_plan [in_bits out_nbytes a_0 .. a_{in_bits-1} TABLE]
//
// TABLE is the table's bytes in hex (2^in_bits entries of out_nbytes little-endian bytes).
// Without arguments the cases are read from stdin, one per line in the same form.  Every case
// prints one JSON object: "status" (hm_status of the bounds, then of plan_lookup), the
// coefficient masks (hex, bit S of mask j = the monomial S of output bit j), the output bounds
// and, when the plan fits, the wave's LDS layout.  A last line is the plan of a byte index at bound 20 000 per bit, whose two
// accumulators alone exceed a block's LDS.
#include "../../homomorph-rust_amd/csrc/lookup_host.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

static int hexval(char c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

// (what hm_lookup_batch has checked before it plans)
static bool run_case(const std::vector<std::string> &w) {
    if (w.size() < 3) return false;
    const uint32_t k = (uint32_t)std::strtoul(w[0].c_str(), nullptr, 10);
    const uint32_t nbytes = (uint32_t)std::strtoul(w[1].c_str(), nullptr, 10);
    if (k == 0 || k > hm::kLookupMaxIn || (nbytes != 1 && nbytes != 2 && nbytes != 4) ||
        w.size() != 3 + k)
        return false;
    std::vector<uint32_t> ab(k);
    for (uint32_t i = 0; i < k; ++i) ab[i] = (uint32_t)std::strtoul(w[2 + i].c_str(), nullptr, 10);
    const std::string &hex = w[2 + k];
    std::vector<uint8_t> table((size_t)nbytes << k);
    if (hex.size() != 2 * table.size()) return false;
    for (size_t i = 0; i < table.size(); ++i) {
        const int hi = hexval(hex[2 * i]), lo = hexval(hex[2 * i + 1]);
        if (hi < 0 || lo < 0) return false;
        table[i] = (uint8_t)(hi * 16 + lo);
    }
    hm::LookupArgs A{};
    std::vector<uint32_t> ob(8 * nbytes, 0);
    hm::lookup_plan::moebius(k, table.data(), nbytes, A.coef);
    hm_status st = hm::lookup_plan::bounds(k, ab.data(), A.coef, 8 * nbytes, ob.data());
    if (st == HM_OK) st = hm::plan_lookup(k, ab.data(), nbytes, A);
    std::printf("{\"status\": %d, \"in_bits\": %u, \"masks\": [", (int)st, k);
    for (uint32_t j = 0; j < 8 * nbytes; ++j) {
        std::printf("%s\"", j ? ", " : "");
        for (int q = 7; q >= 0; --q) std::printf("%08x", A.coef[j][q]);
        std::printf("\"");
    }
    std::printf("], \"bounds\": [");
    for (uint32_t j = 0; j < 8 * nbytes; ++j) std::printf("%s%u", j ? ", " : "", ob[j]);
    std::printf("]");
    if (st == HM_OK) {
        std::printf(", \"kl\": %u, \"kh\": %u, \"need\": %u, \"lds_per_wave\": %u, \"oN\": %u, "
                    "\"oI\": %u, \"oP\": %u, \"cI\": %u, \"cP\": %u, \"off\": [",
                    A.kl, A.kh, A.need, A.lds_per_wave, A.oN, A.oI, A.oP, A.cI, A.cP);
        for (int s = 0; s < 32; ++s) std::printf("%s%u", s ? ", " : "", A.off[s]);
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
        std::fprintf(stderr, "usage: lookup_plan [in_bits out_nbytes a[in_bits] hex-table]\n");
        return 2;
    }
    // beyond LDS: two accumulators of 8 * 20 000 / 32 words each, for four waves
    std::vector<std::string> big = {"8", "1"};
    for (int i = 0; i < 8; ++i) big.push_back("20000");
    std::string all_ones; // v == 255: the top monomial alone
    for (int v = 0; v < 256; ++v) all_ones += v == 255 ? "01" : "00";
    big.push_back(all_ones);
    return run_case(big) ? 0 : 1;
}
