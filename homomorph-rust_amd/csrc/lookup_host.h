// lookup_host.h — the table lookup's planner, host only and header only: from the plaintext table
// and the static bounds of the index bits, the coefficient masks of every output bit (the table's
// algebraic normal form), the table-dependent output bounds, and every plan field of LookupArgs
// (which monomials to form, the wave's LDS layout; the word helpers and the LDS rule are
// circuit_host.h's).  No HIP, no hm_ctx, no allocation:
// hm_lookup_batch (capi.cpp) checks its arguments and plans here;
// tests/sanitize/lookup_plan.cpp compiles this header alone into a stand-alone driver.
#pragma once
#include <stdint.h>
#include <string.h>

#include "circuit_host.h"

namespace hm {
namespace lookup_plan {

inline uint32_t top_bit(uint32_t s) { return 31u - (uint32_t)__builtin_clz(s); } // s > 0

// Entry v of a table of 2^k entries of out_nbytes little-endian bytes; bit j of it.
inline uint32_t table_bit(const uint8_t *table, uint32_t out_nbytes, uint32_t v, uint32_t j) {
    return (table[(size_t)v * out_nbytes + j / 8] >> (j % 8)) & 1u;
}

// The algebraic normal form of every output bit: coef[j] bit S = XOR over S' subset of S of bit j
// of T[S'] (the Moebius transform over the k index bits, in place on the truth table).
inline void moebius(uint32_t k, const uint8_t *table, uint32_t out_nbytes,
                    uint32_t coef[kLookupMaxOut][8]) {
    const uint32_t E = 1u << k;
    memset(coef, 0, sizeof(uint32_t) * kLookupMaxOut * 8);
    for (uint32_t j = 0; j < 8 * out_nbytes; ++j) {
        uint8_t f[1u << kLookupMaxIn];
        for (uint32_t v = 0; v < E; ++v) f[v] = (uint8_t)table_bit(table, out_nbytes, v, j);
        for (uint32_t i = 0; i < k; ++i)
            for (uint32_t v = 0; v < E; ++v)
                if ((v >> i) & 1u) f[v] ^= f[v ^ (1u << i)];
        for (uint32_t v = 0; v < E; ++v)
            if (f[v]) coef[j][v >> 5] |= 1u << (v & 31);
    }
}

inline bool has(const uint32_t c[8], uint32_t S) { return (c[S >> 5] >> (S & 31)) & 1u; }

// out_bound[j] = the largest sum of a_bound over a set S of coef[j] (0: no set, or only the empty
// one).  HM_ERR_UNSUPPORTED beyond the engine's degree range.
inline hm_status bounds(uint32_t k, const uint32_t *a_bound, const uint32_t coef[kLookupMaxOut][8],
                        uint32_t nob, uint32_t *out_bound) {
    const uint32_t E = 1u << k;
    int64_t sum[1u << kLookupMaxIn];
    sum[0] = 0;
    for (uint32_t S = 1; S < E; ++S) sum[S] = sum[S & (S - 1)] + a_bound[__builtin_ctz(S)];
    for (uint32_t j = 0; j < nob; ++j) {
        int64_t b = 0;
        for (uint32_t S = 0; S < E; ++S)
            if (has(coef[j], S) && sum[S] > b) b = sum[S];
        if (b >= (int64_t)1 << 30) return HM_ERR_UNSUPPORTED;
        out_bound[j] = (uint32_t)b;
    }
    return HM_OK;
}

// The 2^kl coefficients of output bit j that go with the high monomial t: bit s = coef[j] bit
// t 2^kl + s (2^kl <= 16 divides 32, so they never straddle a word).
inline uint32_t inner_mask(const uint32_t c[8], uint32_t kl, uint32_t t) {
    const uint32_t at = t << kl;
    return (c[at >> 5] >> (at & 31)) & ((1u << (1u << kl)) - 1u);
}

} // namespace lookup_plan

// Every plan field of LookupArgs but the coefficient masks, which the caller has filled
// (lookup_plan::moebius) and bounded (lookup_plan::bounds); the batches, n, status and the output
// bounds are the caller's too.  The caller has checked k in 1..8 and out_nbytes in {1, 2, 4}.
// HM_ERR_UNSUPPORTED: four waves' slices do not fit a CU's LDS.
inline hm_status plan_lookup(uint32_t k, const uint32_t *a_bound, uint32_t out_nbytes,
                             LookupArgs &A) {
    using namespace lookup_plan;
    const uint32_t kl = (k + 1) / 2, kh = k - kl, nob = 8 * out_nbytes;
    A.k = k, A.kl = kl, A.kh = kh, A.nob = nob;
    memset(A.ab, 0, sizeof(A.ab)), memset(A.ob, 0, sizeof(A.ob));
    for (uint32_t i = 0; i < k; ++i) A.ab[i] = a_bound[i];
    // the monomials the output bits use, and the ones those are formed from: M[s] = M[s without
    // its top bit] times that bit
    uint32_t need = 0;
    for (uint32_t j = 0; j < nob; ++j)
        for (uint32_t t = 0; t < (1u << kh); ++t)
            if (const uint32_t m = inner_mask(A.coef[j], kl, t); m) need |= m | (1u << (16 + t));
    for (uint32_t half = 0; half < 2; ++half)
        for (uint32_t s = (1u << (half ? kh : kl)) - 1; s >= 1; --s)
            if ((need >> (16 * half + s)) & 1u) need |= 1u << (16 * half + (s ^ (1u << top_bit(s))));
    A.need = need;
    // layout, in words.  A single bit's slot holds whole limbs (load_bit); a product's slot its
    // factors' words at their bounds (wave_mul writes nu + nv words).
    uint64_t o = 0;
    A.oN = 0, o = 32;
    const uint64_t unit = o;
    o += 2;
    uint64_t cI = 1, cH = 0; // the widest low monomial; the widest high one
    memset(A.off, 0, sizeof(A.off));
    for (uint32_t half = 0; half < 2; ++half) {
        const uint32_t kk = half ? kh : kl, base = half ? kl : 0;
        int64_t sum[16];
        sum[0] = 0;
        A.off[16 * half] = (uint32_t)unit;
        for (uint32_t s = 1; s < (1u << kk); ++s) {
            const uint32_t top = top_bit(s), rest = s ^ (1u << top), b = a_bound[base + top];
            sum[s] = sum[rest] + b;
            const uint64_t cap = rest ? (uint64_t)words_of_bound(sum[rest]) + words_of_bound(b)
                                      : 2 * (uint64_t)cap_of(b);
            if (o + cap > 0xFFFFFFFFu) return HM_ERR_UNSUPPORTED;
            A.off[16 * half + s] = (uint32_t)o;
            o += even(cap);
            uint64_t &widest = half ? cH : cI;
            if (words_of_bound(sum[s]) > widest) widest = words_of_bound(sum[s]);
        }
    }
    const uint64_t cP = even(cI + cH) + 2; // an accumulator: MH[t] I_jt, or an inner sum alone
    const uint64_t oI = o, oP = oI + even(cI) + 2, total = oP + 2 * cP;
    if (total > 0xFFFFFFFFu) return HM_ERR_UNSUPPORTED;
    A.oI = (uint32_t)oI, A.oP = (uint32_t)oP, A.cI = (uint32_t)cI, A.cP = (uint32_t)cP;
    A.lds_per_wave = (uint32_t)total;
    return lds_status(A.lds_per_wave);
}

} // namespace hm
