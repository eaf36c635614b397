// Host-only account of the array read's and write's plans (array_host.h), under ASan/UBSan: the
// planner header is compiled into this driver and nothing else is linked, no hm_ctx and no GPU.
// Built and run by tests/test_array_host.py (g++ -std=c++17 -fsanitize=address,undefined), as its
// own process.
//
//   array_plan [which nbits count a_0 .. a_{nbits-1} (x_0 .. x_{nbits-1}) s_0 .. s_{k-1}]
//
// which is the hm_op code (28 read, 29 write; x only for a write), k = ceil(log2 count).  Without
// arguments the cases are read from stdin, one per line in the same form.  Every case prints one
// JSON object: "status" (hm_status of the bounds, then of the plan), the output bounds, the index
// bits "k", the circuit's degree "m", the products a value takes and, when the plan fits, the
// wave's LDS layout.  A last line is the plan of a read of 256 elements at bound 2048 on every
// bit, which exceeds a wave's share of a block's LDS.
#include "../../homomorph-rust_amd/csrc/array_host.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

static void print_list(const char *name, const uint32_t *v, uint32_t n) {
    std::printf(", \"%s\": [", name);
    for (uint32_t i = 0; i < n; ++i) std::printf("%s%u", i ? ", " : "", v[i]);
    std::printf("]");
}

// (what hm_array_read_batch / hm_array_write_batch have checked before they plan)
static bool run_case(const std::vector<std::string> &w) {
    if (w.size() < 3) return false;
    const hm_op which = (hm_op)std::strtoul(w[0].c_str(), nullptr, 10);
    const uint32_t nbits = (uint32_t)std::strtoul(w[1].c_str(), nullptr, 10);
    const uint32_t count = (uint32_t)std::strtoul(w[2].c_str(), nullptr, 10);
    const uint32_t k = hm::array_plan::index_bits(count);
    const bool write = which == HM_OP_ARRAY_WRITE;
    if (!hm::array_plan::is_array_op(which) || nbits == 0 || nbits > HM_MAX_BITS || !k ||
        w.size() != 3 + (size_t)nbits * (write ? 2 : 1) + k)
        return false;
    std::vector<uint32_t> ab(nbits), xb(nbits), sb(k), need(nbits);
    size_t p = 3;
    for (uint32_t i = 0; i < nbits; ++i) ab[i] = (uint32_t)std::strtoul(w[p++].c_str(), nullptr, 10);
    if (write)
        for (uint32_t i = 0; i < nbits; ++i) xb[i] = (uint32_t)std::strtoul(w[p++].c_str(), nullptr, 10);
    for (uint32_t t = 0; t < k; ++t) sb[t] = (uint32_t)std::strtoul(w[p++].c_str(), nullptr, 10);
    hm::ArrayReadArgs R{};
    hm::ArrayWriteArgs W{};
    hm_status st;
    if (write) {
        st = hm::array_plan::write_bounds(nbits, ab.data(), xb.data(), count, sb.data(), need.data());
        if (st == HM_OK) st = hm::plan_array_write(nbits, ab.data(), xb.data(), count, sb.data(), W);
    } else {
        st = hm::array_plan::read_bounds(nbits, ab.data(), count, sb.data(), need.data());
        if (st == HM_OK) st = hm::plan_array_read(nbits, ab.data(), count, sb.data(), false, R);
    }
    std::printf("{\"status\": %d, \"which\": %d, \"nbits\": %u, \"count\": %u, \"k\": %u, \"m\": %u, "
                "\"products\": %u, \"indicator_products\": %u",
                (int)st, (int)which, nbits, count, k, hm::array_plan::degree_of(k),
                write ? hm::array_plan::write_products(nbits, count)
                      : hm::array_plan::read_products(nbits, count),
                hm::array_plan::indicator_products(count));
    print_list("bounds", need.data(), nbits);
    if (st == HM_OK && write) {
        std::printf(", \"lds_per_wave\": %u, \"oN\": %u, \"oU\": %u, \"oT\": %u, \"oX\": %u, "
                    "\"oO\": %u, \"oV\": %u",
                    W.lds_per_wave, W.oN, W.oU, W.oT, W.oX, W.oO, W.oV);
        print_list("soff", W.soff, hm::kArrayMaxIndex);
        print_list("qoff", W.qoff, hm::kArrayMaxIndex);
        print_list("sb", W.sb, hm::kArrayMaxIndex);
    } else if (st == HM_OK) {
        std::printf(", \"lds_per_wave\": %u, \"shared\": %u, \"oN\": %u, \"oL\": %u, \"oX\": %u, "
                    "\"oP\": %u, \"cP\": %u",
                    R.lds_per_wave, R.shared, R.oN, R.oL, R.oX, R.oP, R.cP);
        print_list("soff", R.soff, hm::kArrayMaxIndex);
        print_list("slot", R.slot, hm::kArrayMaxIndex);
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
        std::fprintf(stderr, "usage: array_plan [which nbits count a[nbits] (x[nbits]) s[k]]\n");
        return 2;
    }
    // beyond LDS: the eight waiting left children of a 256-element read at bound 2048
    std::vector<std::string> big = {"28", "8", "256"};
    for (int i = 0; i < 16; ++i) big.push_back("2048");
    return run_case(big) ? 0 : 1;
}
