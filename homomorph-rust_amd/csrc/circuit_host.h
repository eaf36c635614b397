// circuit_host.h — the host-only, header-only home of what the wave-per-value circuits (kernels.hip:
// gates, borrow chain, min / max, select, lookup, shift) plan on the host: the word and rounding
// helpers, the LDS rule, and for the gates, the ripple-borrow chain, min / max and select the
// static degree bounds and the wave's LDS layout.  (The lookup's and the shifter's own planners,
// lookup_host.h and shift_host.h, build on the helpers here.)  No HIP, no hm_ctx, no allocation
// beyond std::vector: the hm_*_out_bounds and hm_*_batch entries (capi.cpp) check their arguments
// and plan here; tests/sanitize/circuit_plan.cpp compiles this header alone into a stand-alone
// driver (tests/test_circuit_plans.py).
//
// A layout is word offsets into a wave's slice of lds_per_wave words.  An operand row holds one
// bit's whole limbs as load_bit writes them, 2 cap_of(bound) words of the operand's widest bit,
// and two spare words; a product buffer holds what wave_mul writes, its factors' words and one.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "engine.h"

namespace hm {

// (cap_of and words_of_bound, the limbs and the words at a degree bound: engine.h)
inline uint64_t even(uint64_t v) { return (v + 1) & ~(uint64_t)1; }

// The LDS rule of the wave-per-value circuits: a block is four waves, and its four slices of
// lds_per_wave words fit a CU's 160 KiB
inline bool fits_cu_lds(uint64_t lds_per_wave) { return lds_per_wave * 4 * 4 <= 160 * 1024; }
inline hm_status lds_status(uint64_t lds_per_wave) {
    return fits_cu_lds(lds_per_wave) ? HM_OK : HM_ERR_UNSUPPORTED;
}

// ------------------------------------------------------------------ static degree bounds
// (deg(xy) = deg x + deg y, deg(x + y) <= max; HM_ERR_UNSUPPORTED beyond the engine's degree range.
// The callers have checked their pointers and widths.)

inline hm_status gate_bounds(hm_op g, uint32_t L, const uint32_t *a, const uint32_t *b,
                             uint32_t *out) {
    for (uint32_t i = 0; i < L; ++i) {
        uint64_t v;
        switch (g) {
        case HM_OP_AND: case HM_OP_OR: v = (uint64_t)a[i] + b[i]; break;
        case HM_OP_XOR: v = std::max(a[i], b[i]); break;
        case HM_OP_NOT: v = a[i]; break;
        default: return HM_ERR_INVALID_ARGUMENT;
        }
        if (v >= (1u << 30)) return HM_ERR_UNSUPPORTED;
        out[i] = (uint32_t)v;
    }
    return HM_OK;
}

// Borrow bounds wb_0 = 0, wb_{i+1} = max(a_i + b_i, max(a_i, b_i) + wb_i) for i < upto; false
// beyond the engine's degree range.  wb[i] for i <= upto.
inline bool borrow_bounds(uint32_t upto, const uint32_t *a, const uint32_t *b,
                          std::vector<int64_t> &wb) {
    wb.assign(upto + 1, 0);
    for (uint32_t i = 0; i < upto; ++i) {
        wb[i + 1] = std::max<int64_t>((int64_t)a[i] + b[i], std::max<int64_t>(a[i], b[i]) + wb[i]);
        if (wb[i + 1] >= (int64_t)1 << 30) return false;
    }
    return true;
}

// Subtraction: out_i = x_i + w_i
inline hm_status sub_bounds(uint32_t L, const uint32_t *a, const uint32_t *b, uint32_t *out) {
    std::vector<int64_t> wb;
    if (!borrow_bounds(L - 1, a, b, wb)) return HM_ERR_UNSUPPORTED;
    for (uint32_t i = 0; i < L; ++i) {
        const int64_t s = std::max<int64_t>(std::max(a[i], b[i]), wb[i]);
        if (s >= (int64_t)1 << 30) return HM_ERR_UNSUPPORTED;
        out[i] = (uint32_t)s;
    }
    return HM_OK;
}

// A comparison's Ciphered<bool>: bit 0 is the last borrow (an ordering) or the equality prefix
// e_L, bits 1..7 are null
inline hm_status compare_bounds(bool ordering, uint32_t L, const uint32_t *a, const uint32_t *b,
                                uint32_t out[8]) {
    int64_t r = 0;
    if (ordering) { // (the recurrence is symmetric: exchanging the operands keeps it)
        std::vector<int64_t> wb;
        if (!borrow_bounds(L, a, b, wb)) return HM_ERR_UNSUPPORTED;
        r = wb[L];
    } else {
        for (uint32_t i = 0; i < L; ++i) r += std::max(a[i], b[i]);
        if (r >= (int64_t)1 << 30) return HM_ERR_UNSUPPORTED;
    }
    out[0] = (uint32_t)r;
    for (int k = 1; k < 8; ++k) out[k] = 0;
    return HM_OK;
}

// select, min and max: the condition's bound (for min / max the last borrow's,
// wb_L) plus the wider operand's, bit by bit
inline hm_status choice_bounds(uint32_t L, int64_t cond, const uint32_t *a, const uint32_t *b,
                               uint32_t *out) {
    for (uint32_t i = 0; i < L; ++i) {
        const int64_t s = cond + std::max(a[i], b[i]);
        if (s >= (int64_t)1 << 30) return HM_ERR_UNSUPPORTED;
        out[i] = (uint32_t)s;
    }
    return HM_OK;
}

inline hm_status minmax_bounds(uint32_t L, const uint32_t *a, const uint32_t *b, uint32_t *out) {
    std::vector<int64_t> wb;
    if (!borrow_bounds(L, a, b, wb)) return HM_ERR_UNSUPPORTED;
    return choice_bounds(L, wb[L], a, b, out);
}

// ------------------------------------------------------------------ LDS layouts
// Words of the operand rows: two per limb of the widest bit of a, of b (null: a unary gate, two
// words) and of either
struct Slots {
    uint32_t SA = 2, SB = 2, SX = 2;
};
inline Slots operand_slots(uint32_t nbits, const uint32_t *a, const uint32_t *b) {
    Slots s;
    for (uint32_t i = 0; i < nbits; ++i) {
        s.SA = std::max(s.SA, 2 * cap_of(a[i]));
        if (b) s.SB = std::max(s.SB, 2 * cap_of(b[i]));
    }
    s.SX = std::max(s.SA, s.SB);
    return s;
}

// gate_kernel: a_i | b_i | the result at oT: a product a_i b_i of up to SA + SB words, with (OR)
// x_i = a_i + b_i behind it
inline hm_status plan_gate(uint32_t nbits, const uint32_t *a, const uint32_t *b, GateArgs &G) {
    const Slots s = operand_slots(nbits, a, b);
    G.oA = 0, G.oB = s.SA + 2, G.oT = G.oB + s.SB + 2;
    G.lds_per_wave = G.oT + 2 * (s.SA + s.SB) + 8;
    return lds_status(G.lds_per_wave);
}

// borrow_kernel and minmax_kernel, chain = the degree bound of the last borrow (or equality
// prefix) formed, for min / max wb_L: a_i | b_i | x_i | p_i | generate term a_i b_i + b_i | two
// borrow buffers of cw words each.  The widest product p_i w_i, like min / max's x_i w_L, spans
// words(p_i) + words(w_i) <= SX + chain / 32 + 1 words.
inline BorrowLayout borrow_layout(const Slots &s, int64_t chain) {
    BorrowLayout y{};
    y.oA = 0, y.oB = s.SA + 2, y.oX = y.oB + s.SB + 2, y.oP = y.oX + s.SX + 2, y.oG = y.oP + s.SX + 2;
    y.oW = y.oG + s.SA + s.SB + 2;
    y.cw = s.SX + (uint32_t)(chain / 32) + 3;
    y.lds_per_wave = y.oW + 2 * y.cw;
    return y;
}
inline hm_status plan_borrow(uint32_t nbits, const uint32_t *a, const uint32_t *b, int64_t chain,
                             BorrowLayout &Y) {
    Y = borrow_layout(operand_slots(nbits, a, b), chain);
    return lds_status(Y.lds_per_wave);
}

// select_kernel: c | a_i | b_i | x_i | the product c x_i + b_i: words(c) + words(x_i) <= SC + SX
inline hm_status plan_select(uint32_t nbits, uint32_t cbound, const uint32_t *a, const uint32_t *b,
                             SelectArgs &G) {
    const Slots s = operand_slots(nbits, a, b);
    const uint32_t SC = 2 * cap_of(cbound);
    G.cbound = cbound;
    G.oC = 0, G.oA = SC + 2, G.oB = G.oA + s.SA + 2, G.oX = G.oB + s.SB + 2, G.oT = G.oX + s.SX + 2;
    G.lds_per_wave = G.oT + SC + s.SX + 2;
    return lds_status(G.lds_per_wave);
}

} // namespace hm
