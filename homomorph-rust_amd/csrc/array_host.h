// array_host.h — the planner of the oblivious array read and write by an encrypted index, host
// only and header only: the index bits of a count, the static output bounds, the requirement's
// degree, the products a value takes and every plan field of ArrayReadArgs / ArrayWriteArgs (the
// wave's LDS layout).  No HIP, no hm_ctx, no allocation beyond std::vector:
// hm_array_*_out_bounds and hm_array_*_batch (capi.cpp) check their arguments and plan here;
// tests/sanitize/array_plan.cpp compiles this header alone into a stand-alone driver.
#pragma once
#include <stdint.h>
#include <string.h>

#include "bitcount_host.h"

namespace hm {
namespace array_plan {

inline bool is_array_op(hm_op op) { return op == HM_OP_ARRAY_READ || op == HM_OP_ARRAY_WRITE; }

// k = ceil(log2 count) for a count the entries take (2..kArrayMaxCount), or 0
inline uint32_t index_bits(uint32_t count) {
    if (count < 2 || count > kArrayMaxCount) return 0;
    return 32u - (uint32_t)__builtin_clz(count - 1);
}

// the circuits' degree m in fresh bits (the requirement is 2m + 1 = 2k + 3): an indicator's k
// literals times an element's or the written value's bit
inline uint32_t degree_of(uint32_t k) { return k + 1; }

// A wave's slice of LDS: the bit counts' rule, 2560 words, so that four blocks stay resident on a
// CU (serial, latency-bound chains like theirs)
inline hm_status lds_rule(uint64_t lds_per_wave) { return bitcount_plan::lds_rule(lds_per_wave); }

// S = the sum of the k index bounds; false beyond the engine's degree range
inline bool index_sum(uint32_t k, const uint32_t *s_bound, int64_t &S) {
    S = 0;
    for (uint32_t t = 0; t < k; ++t) S += s_bound[t];
    return S < (int64_t)1 << 30;
}

// read: out_bound[j] = S + arr_bound[j].  The caller has checked nbits and count.
inline hm_status read_bounds(uint32_t nbits, const uint32_t *arr_bound, uint32_t count,
                             const uint32_t *s_bound, uint32_t *out_bound) {
    int64_t S;
    if (!index_sum(index_bits(count), s_bound, S)) return HM_ERR_UNSUPPORTED;
    for (uint32_t j = 0; j < nbits; ++j) {
        const int64_t b = S + arr_bound[j];
        if (b >= (int64_t)1 << 30) return HM_ERR_UNSUPPORTED;
        out_bound[j] = (uint32_t)b;
    }
    return HM_OK;
}

// write: out_bound[j] = S + max(arr_bound[j], x_bound[j]), shared by all elements
inline hm_status write_bounds(uint32_t nbits, const uint32_t *arr_bound, const uint32_t *x_bound,
                              uint32_t count, const uint32_t *s_bound, uint32_t *out_bound) {
    int64_t S;
    if (!index_sum(index_bits(count), s_bound, S)) return HM_ERR_UNSUPPORTED;
    for (uint32_t j = 0; j < nbits; ++j) {
        const int64_t b = S + std::max(arr_bound[j], x_bound[j]);
        if (b >= (int64_t)1 << 30) return HM_ERR_UNSUPPORTED;
        out_bound[j] = (uint32_t)b;
    }
    return HM_OK;
}

// Products a value takes at most (a null factor skips its own).  read: per output bit one per
// tree node above the leaves with an element below it, the sum over t = 1..k of ceil(count / 2^t)
// (count - 1 for a power of two; a node whose right sibling is past the array still multiplies,
// y = L + s_t L).  write: the suffix products of the indicators (level k - 1 is the literal itself)
// and one product per element bit.
inline uint32_t read_products(uint32_t nbits, uint32_t count) {
    uint32_t per_bit = 0;
    for (uint32_t t = 1; t <= index_bits(count); ++t) per_bit += (count + (1u << t) - 1) >> t;
    return nbits * per_bit;
}
inline uint32_t indicator_products(uint32_t count) {
    const uint32_t k = index_bits(count);
    uint32_t c = k - 1; // v = 0: levels k - 2 .. 0
    for (uint32_t v = 1; v < count; ++v) {
        const uint32_t top = (uint32_t)__builtin_ctz(v); // levels top .. 0 are formed again
        c += top + 1 - (top == k - 1);
    }
    return c;
}
inline uint32_t write_products(uint32_t nbits, uint32_t count) {
    return indicator_products(count) + nbits * count;
}

// words of a buffer that holds a polynomial within bound: what wave_mul writes for it (its
// factors' words, nu + nv <= bound / 32 + 2), which covers a loaded bit's whole limbs
inline uint64_t buf(int64_t bound) { return even((uint64_t)bound / 32 + 2); }

} // namespace array_plan

// Every plan field of ArrayReadArgs from the bounds; the I/O block is the caller's.  The caller
// has checked nbits and count.  The layout works one output bit at a time, at the widest element
// bit: it does not depend on the element width.  HM_ERR_UNSUPPORTED: a bound beyond the engine's
// degree range, or a wave's slice beyond array_plan::lds_rule.
inline hm_status plan_array_read(uint32_t nbits, const uint32_t *arr_bound, uint32_t count,
                                 const uint32_t *s_bound, bool shared, ArrayReadArgs &A) {
    using namespace array_plan;
    const uint32_t k = index_bits(count);
    int64_t S;
    if (!index_sum(k, s_bound, S)) return HM_ERR_UNSUPPORTED;
    uint32_t amax = 0;
    for (uint32_t j = 0; j < nbits; ++j) amax = std::max(amax, arr_bound[j]);
    if (S + amax >= (int64_t)1 << 30) return HM_ERR_UNSUPPORTED;
    A.count = count, A.k = k, A.shared = shared;
    memset(A.soff, 0, sizeof(A.soff)), memset(A.slot, 0, sizeof(A.slot));
    uint64_t o = 0;
    A.oN = 0, o = 2 * kArrayMaxIndex;
    for (uint32_t t = 0; t < k; ++t) {
        A.soff[t] = (uint32_t)o;
        o += 2 * (uint64_t)cap_of(s_bound[t]);
    }
    // a level-t node is within amax + s_bound[0] + .. + s_bound[t - 1]; L + R at the last join is
    // a level k - 1 node, the root a level k one
    std::vector<int64_t> lvl(k + 1, amax);
    for (uint32_t t = 0; t < k; ++t) lvl[t + 1] = lvl[t] + s_bound[t];
    A.oL = (uint32_t)o, o += buf(lvl[0]);
    A.oX = (uint32_t)o, o += buf(lvl[k - 1]);
    A.cP = (uint32_t)buf(lvl[k]);
    A.oP = (uint32_t)o, o += 2 * (uint64_t)A.cP;
    for (uint32_t t = 0; t < k; ++t) {
        A.slot[t] = (uint32_t)o;
        o += buf(lvl[t]);
    }
    if (o > 0xFFFFFFFFu) return HM_ERR_UNSUPPORTED;
    A.lds_per_wave = (uint32_t)o;
    return lds_rule(A.lds_per_wave);
}

// Every plan field of ArrayWriteArgs from the bounds; the I/O block and the index batch are the
// caller's.  x's bits are kept in LDS for the whole value, never reloaded per element: a shape
// whose slice that takes beyond the rule is refused.
inline hm_status plan_array_write(uint32_t nbits, const uint32_t *arr_bound,
                                  const uint32_t *x_bound, uint32_t count,
                                  const uint32_t *s_bound, ArrayWriteArgs &A) {
    using namespace array_plan;
    const uint32_t k = index_bits(count);
    int64_t S;
    if (!index_sum(k, s_bound, S)) return HM_ERR_UNSUPPORTED;
    uint32_t amax = 0, xmax = 0, smax = 0;
    uint64_t xwords = 0;
    for (uint32_t j = 0; j < nbits; ++j) {
        amax = std::max(amax, arr_bound[j]), xmax = std::max(xmax, x_bound[j]);
        xwords += 2 * (uint64_t)cap_of(x_bound[j]);
    }
    const uint32_t wide = std::max(amax, xmax);
    if (S + wide >= (int64_t)1 << 30) return HM_ERR_UNSUPPORTED;
    A.count = count, A.k = k;
    memset(A.soff, 0, sizeof(A.soff)), memset(A.qoff, 0, sizeof(A.qoff));
    memset(A.sb, 0, sizeof(A.sb));
    uint64_t o = 0;
    A.oN = 0, o = even(2 * (uint64_t)kArrayMaxIndex + nbits);
    for (uint32_t t = 0; t < k; ++t) {
        A.soff[t] = (uint32_t)o, A.sb[t] = s_bound[t];
        o += 2 * (uint64_t)cap_of(s_bound[t]);
        smax = std::max(smax, s_bound[t]);
    }
    A.oU = (uint32_t)o, o += buf(smax);
    A.oT = (uint32_t)o, o += buf(amax);
    A.oX = (uint32_t)o, o += buf(wide);
    A.oO = (uint32_t)o, o += buf(S + wide);
    int64_t suffix = 0; // Q_t is within s_bound[t] + .. + s_bound[k - 1]
    for (uint32_t t = k; t-- > 0;) {
        suffix += s_bound[t];
        A.qoff[t] = (uint32_t)o;
        o += buf(suffix);
    }
    A.oV = (uint32_t)o, o += xwords;
    if (o > 0xFFFFFFFFu) return HM_ERR_UNSUPPORTED;
    A.lds_per_wave = (uint32_t)o;
    return lds_rule(A.lds_per_wave);
}

} // namespace hm
