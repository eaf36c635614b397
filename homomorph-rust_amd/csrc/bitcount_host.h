// bitcount_host.h — the planner of the bit counts (count_ones, count_zeros, leading / trailing
// zeros / ones), host only and header only: the static output bounds, the requirement's degree, the
// number of updates the needed-set rule leaves (engine.h bitcount_needed, shared with the kernel)
// and every plan field of BitCountArgs (the wave's LDS layout).  No HIP, no hm_ctx, no allocation
// beyond std::vector: hm_bitcount_out_bounds and hm_bitcount_batch (capi.cpp) check their
// arguments and plan here; tests/sanitize/bitcount_plan.cpp compiles this header alone into a
// stand-alone driver.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "circuit_host.h"

namespace hm {
namespace bitcount_plan {

inline bool is_bitcount_op(hm_op op) {
    return op >= HM_OP_COUNT_ONES && op <= HM_OP_TRAILING_ONES;
}
inline bool is_run_op(hm_op op) { return op >= HM_OP_LEADING_ZEROS && op <= HM_OP_TRAILING_ONES; }
inline bool counts_zeros(hm_op op) {
    return op == HM_OP_COUNT_ZEROS || op == HM_OP_LEADING_ZEROS || op == HM_OP_TRAILING_ZEROS;
}
inline bool is_leading(hm_op op) { return op == HM_OP_LEADING_ZEROS || op == HM_OP_LEADING_ONES; }

// A wave's slice of LDS: a quarter of what the circuits' general rule (circuit_host.h lds_status)
// admits, 2560 words, so that four blocks stay resident on a CU (four waves a SIMD: the chains here
// are serial and latency bound, and one block a CU would leave three SIMD slots in four idle).
constexpr uint32_t kLdsWords = 160 * 1024 / 4 / (4 * 4);
inline hm_status lds_rule(uint64_t lds_per_wave) {
    return lds_per_wave <= kLdsWords ? lds_status(lds_per_wave) : HM_ERR_UNSUPPORTED;
}

// output bits that are not null by rule: 2^k <= nbits (nbits in 1..HM_MAX_BITS)
inline uint32_t out_bits(uint32_t nbits) { return 32u - (uint32_t)__builtin_clz(nbits); }

// the circuit's degree m in fresh bits (the requirement is 2m + 1): a count's top target
// 2^floor(log2 n), a run's whole prefix n
inline uint32_t degree_of(hm_op which, uint32_t nbits) {
    return is_run_op(which) ? nbits : 1u << (out_bits(nbits) - 1);
}

// slots E_1 .. E_J of a count, and whether its top target is the running product past them
inline uint32_t count_slots(uint32_t nbits) {
    const uint32_t top = 1u << (out_bits(nbits) - 1);
    return top == nbits && nbits >= 2 ? nbits / 2 : top;
}
inline bool count_diag(uint32_t nbits) { return count_slots(nbits) < (1u << (out_bits(nbits) - 1)); }

// Updates E_j <- E_j + u_i E_{j-1} (counts) or t_j = t_{j-1} v_j (runs) a value takes: with_unit
// counts those whose factor is the unit polynomial E_0 or t_0 (j = 1: the kernels copy or XOR
// there), without it only the products the kernels issue at most.
inline uint32_t updates(hm_op which, uint32_t nbits, bool with_unit) {
    if (is_run_op(which)) return with_unit ? nbits : nbits - 1;
    uint32_t c = 0;
    for (uint32_t i = 1; i <= nbits; ++i)
        for (uint32_t j = with_unit ? 1 : 2; j <= i; ++j) c += bitcount_needed(nbits, i, j);
    return c;
}

// Counts: out_bound[k] = the sum of the 2^k largest a_bound.  Runs: the sum of a_bound over the
// first M literals in the run's order (leading: from the top bit down), M the largest multiple
// of 2^k that is <= nbits.  Bits with 2^k > nbits: 0.  sums[j] (j <= nbits) = the bound of E_j,
// the j largest (counts), or of t_j, the first j (runs).  The caller has checked which and nbits.
// HM_ERR_UNSUPPORTED beyond the engine's degree range.
inline hm_status bounds(hm_op which, uint32_t nbits, const uint32_t *a_bound,
                        uint32_t out_bound[kBitCountOut], std::vector<int64_t> *sums = nullptr) {
    std::vector<uint32_t> v(a_bound, a_bound + nbits);
    if (!is_run_op(which)) std::sort(v.begin(), v.end(), std::greater<uint32_t>());
    else if (is_leading(which)) std::reverse(v.begin(), v.end());
    std::vector<int64_t> s(nbits + 1, 0);
    for (uint32_t j = 0; j < nbits; ++j) s[j + 1] = s[j] + v[j];
    for (uint32_t k = 0; k < kBitCountOut; ++k) {
        const uint32_t M = is_run_op(which) ? (nbits >> k) << k : 1u << k;
        const int64_t b = M >= 1 && M <= nbits ? s[M] : 0;
        if (b >= (int64_t)1 << 30) return HM_ERR_UNSUPPORTED;
        out_bound[k] = (uint32_t)b;
    }
    if (sums) sums->swap(s);
    return HM_OK;
}

} // namespace bitcount_plan

// Every plan field of BitCountArgs from the input bounds; the I/O block (the batches and their own
// bounds) is the caller's.  The caller has checked which and nbits.  HM_ERR_UNSUPPORTED: a bound
// beyond the engine's degree range, or a wave's slice is beyond bitcount_plan::lds_rule.
inline hm_status plan_bitcount(hm_op which, uint32_t nbits, const uint32_t *a_bound,
                               BitCountArgs &A) {
    using namespace bitcount_plan;
    uint32_t ob[kBitCountOut];
    std::vector<int64_t> sums;
    if (hm_status st = bounds(which, nbits, a_bound, ob, &sums); st) return st;
    const bool runs = is_run_op(which);
    A.zeros = counts_zeros(which), A.leading = is_leading(which);
    A.K = out_bits(nbits);
    A.J = runs ? 0 : count_slots(nbits), A.diag = !runs && count_diag(nbits);
    memset(A.off, 0, sizeof(A.off));
    uint64_t limbs = 0;
    uint32_t amax = 0;
    for (uint32_t i = 0; i < nbits; ++i) {
        limbs += cap_of(a_bound[i]);
        amax = std::max(amax, a_bound[i]);
    }
    A.a_limbs = (uint32_t)limbs;
    // layout, in words.  The literal's buffer holds whole limbs (load_bit); a product's buffer its
    // factors' words at their degrees (wave_mul writes nu + nv <= bound / 32 + 2 words), and so
    // does a slot or an accumulator, which then holds the bound / 32 + 1 words of its polynomial.
    auto buf = [](int64_t bound) { return even((uint64_t)bound / 32 + 2); };
    uint64_t o = 0;
    A.oN = 0, o = even(runs ? kBitCountOut : A.J + 1);
    A.oU = (uint32_t)o, o += 2 * (uint64_t)cap_of(amax) + 2;
    A.oT = (uint32_t)o, o += runs ? 0 : buf(sums[A.J]);
    const uint64_t cD = runs || A.diag ? buf(sums[nbits]) : 0;
    A.oD = (uint32_t)o, o += 2 * cD;
    A.oE = (uint32_t)o;
    uint64_t cE = 0;
    if (runs) {
        for (uint32_t k = 0; k < A.K; ++k) A.off[k] = (uint32_t)cE, cE += buf(ob[k]);
    } else {
        for (uint32_t j = 1; j <= A.J; ++j) A.off[j] = (uint32_t)cE, cE += buf(sums[j]);
    }
    const uint64_t total = o + cE;
    if (total > 0xFFFFFFFFu) return HM_ERR_UNSUPPORTED;
    A.cD = (uint32_t)cD;
    A.lds_per_wave = (uint32_t)total;
    return lds_rule(A.lds_per_wave);
}

} // namespace hm
