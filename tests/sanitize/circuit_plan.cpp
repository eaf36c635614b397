// Host-only account of the plans of the gates, the ripple-borrow chain, min / max and select
// (circuit_host.h), under ASan/UBSan: the planner header is compiled into this driver and nothing
// else is linked, no hm_ctx and no GPU.  Built and run by tests/test_circuit_plans.py
// (g++ -std=c++17 -fsanitize=address,undefined), as its own process.
//
//   circuit_plan < cases        one case per line:   circuit nbits cond a_0 .. a_{nbits-1} [b_0 ..]
//
// circuit is and, or, xor, not (no b), sub, lt, eq, minmax or select; cond is the bound of
// select's condition (read by select alone).  Every case is planned as its hm_*_batch entry does
// (the out-bounds rule, then the layout) and prints one JSON object: "status", the operand rows'
// words ("SA", "SB", "SX"; select: "SC") and every field of the layout.  A first line prints the
// LDS rule at its edge, fits_cu_lds of 10240 and of 10241 words.
#include "../../homomorph-rust_amd/csrc/circuit_host.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace hm;

static void print_slots(const Slots &s) {
    std::printf(", \"SA\": %u, \"SB\": %u, \"SX\": %u", s.SA, s.SB, s.SX);
}

static bool run_case(const std::vector<std::string> &w) {
    if (w.size() < 4) return false;
    const std::string &circuit = w[0];
    const uint32_t nbits = (uint32_t)std::strtoul(w[1].c_str(), nullptr, 10);
    const uint32_t cond = (uint32_t)std::strtoul(w[2].c_str(), nullptr, 10);
    const bool unary = circuit == "not";
    if (nbits == 0 || nbits > HM_MAX_BITS || w.size() != 3 + (unary ? 1 : 2) * (size_t)nbits)
        return false;
    std::vector<uint32_t> a(nbits), b(nbits), need(std::max(nbits, 8u));
    for (uint32_t i = 0; i < nbits; ++i) {
        a[i] = (uint32_t)std::strtoul(w[3 + i].c_str(), nullptr, 10);
        if (!unary) b[i] = (uint32_t)std::strtoul(w[3 + nbits + i].c_str(), nullptr, 10);
    }
    const uint32_t *pb = unary ? nullptr : b.data();
    const Slots s = operand_slots(nbits, a.data(), pb);
    std::printf("{\"circuit\": \"%s\", \"nbits\": %u", circuit.c_str(), nbits);
    hm_status st;
    if (circuit == "and" || circuit == "or" || circuit == "xor" || unary) {
        const hm_op g = circuit == "and" ? HM_OP_AND : circuit == "or" ? HM_OP_OR
                        : circuit == "xor" ? HM_OP_XOR : HM_OP_NOT;
        GateArgs G{};
        st = gate_bounds(g, nbits, a.data(), pb, need.data());
        if (st == HM_OK) {
            st = plan_gate(nbits, a.data(), pb, G);
            print_slots(s);
            std::printf(", \"lds_per_wave\": %u, \"oA\": %u, \"oB\": %u, \"oT\": %u", G.lds_per_wave,
                        G.oA, G.oB, G.oT);
        }
    } else if (circuit == "sub" || circuit == "lt" || circuit == "eq" || circuit == "minmax") {
        // the chain's last bound, as hm_sub_batch, hm_compare_batch and hm_minmax_batch take it
        int64_t chain = 0;
        std::vector<int64_t> wb;
        if (circuit == "sub") {
            st = sub_bounds(nbits, a.data(), b.data(), need.data());
            if (st == HM_OK) borrow_bounds(nbits - 1, a.data(), b.data(), wb), chain = wb[nbits - 1];
        } else if (circuit == "minmax") {
            st = minmax_bounds(nbits, a.data(), b.data(), need.data());
            if (st == HM_OK) borrow_bounds(nbits, a.data(), b.data(), wb), chain = wb[nbits];
        } else {
            st = compare_bounds(circuit == "lt", nbits, a.data(), b.data(), need.data());
            chain = need[0];
        }
        if (st == HM_OK) {
            BorrowLayout Y{};
            st = plan_borrow(nbits, a.data(), b.data(), chain, Y);
            print_slots(s);
            std::printf(", \"chain\": %lld, \"lds_per_wave\": %u, \"oA\": %u, \"oB\": %u, \"oX\": %u, "
                        "\"oP\": %u, \"oG\": %u, \"oW\": %u, \"cw\": %u",
                        (long long)chain, Y.lds_per_wave, Y.oA, Y.oB, Y.oX, Y.oP, Y.oG, Y.oW, Y.cw);
        }
    } else if (circuit == "select") {
        SelectArgs G{};
        st = choice_bounds(nbits, cond, a.data(), b.data(), need.data());
        if (st == HM_OK) {
            st = plan_select(nbits, cond, a.data(), b.data(), G);
            print_slots(s);
            std::printf(", \"SC\": %u, \"lds_per_wave\": %u, \"oC\": %u, \"oA\": %u, \"oB\": %u, "
                        "\"oX\": %u, \"oT\": %u",
                        2 * cap_of(cond), G.lds_per_wave, G.oC, G.oA, G.oB, G.oX, G.oT);
        }
    } else {
        return false;
    }
    std::printf(", \"status\": %d}\n", (int)st);
    return true;
}

int main() {
    std::printf("{\"fits_10240\": %d, \"fits_10241\": %d}\n", (int)fits_cu_lds(10240),
                (int)fits_cu_lds(10241));
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::vector<std::string> w;
        for (std::string t; in >> t;) w.push_back(t);
        if (!w.empty() && !run_case(w)) {
            std::fprintf(stderr, "usage: circuit_plan < cases (circuit nbits cond a[nbits] [b[nbits]])\n");
            return 2;
        }
    }
    return 0;
}
