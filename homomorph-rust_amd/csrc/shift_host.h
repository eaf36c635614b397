// shift_host.h — the planner of the shifts and rotates by an encrypted amount, host only and
// header only: the static output bounds, the stages' source map (engine.h shift_src, shared with
// the kernel) and every plan field of ShiftArgs (the wave's LDS layout).  No HIP, no hm_ctx, no
// allocation: hm_shift_out_bounds and hm_shift_batch (capi.cpp) check their arguments and plan
// here; tests/sanitize/shift_plan.cpp compiles this header alone into a stand-alone driver.
#pragma once
#include <stdint.h>
#include <string.h>

#include "circuit_host.h"

namespace hm {
namespace shift_plan {

inline bool is_shift_op(hm_op op) { return op >= HM_OP_SHL && op <= HM_OP_ROTR; }

// log2 of a width the shifter takes (a power of two in 2..HM_MAX_BITS), or 0
inline uint32_t stages(uint32_t nbits) {
    if (nbits < 2 || nbits > HM_MAX_BITS || (nbits & (nbits - 1))) return 0;
    return 31u - (uint32_t)__builtin_clz(nbits);
}

inline uint32_t mode_of(hm_op which, bool is_signed) {
    switch (which) {
    case HM_OP_SHL: return kShiftShl;
    case HM_OP_SHR: return is_signed ? kShiftSar : kShiftShr;
    case HM_OP_ROTL: return kShiftRotl;
    default: return kShiftRotr;
    }
}

// out_bound[j] = the sum of the L amount bounds plus the widest bit of a that can reach bit j: the
// bits at or below j for a left shift, at or above j for a right shift (either kind), every bit
// for a rotate.  Every stage's intermediate value stays within it, whatever the stage order.
// The caller has checked which and nbits.  HM_ERR_UNSUPPORTED beyond the engine's degree range.
inline hm_status bounds(hm_op which, uint32_t nbits, const uint32_t *a_bound,
                        const uint32_t *s_bound, uint32_t *out_bound) {
    const uint32_t L = stages(nbits);
    int64_t S = 0;
    for (uint32_t t = 0; t < L; ++t) S += s_bound[t];
    uint32_t widest = 0;
    for (uint32_t i = 0; i < nbits; ++i) widest = a_bound[i] > widest ? a_bound[i] : widest;
    uint32_t run = 0;
    for (uint32_t q = 0; q < nbits; ++q) {
        const uint32_t j = which == HM_OP_SHR ? nbits - 1 - q : q; // SHR: from the top bit down
        run = a_bound[j] > run ? a_bound[j] : run;
        const int64_t b = S + (which == HM_OP_SHL || which == HM_OP_SHR ? run : widest);
        if (b >= (int64_t)1 << 30) return HM_ERR_UNSUPPORTED;
        out_bound[j] = (uint32_t)b;
    }
    return HM_OK;
}

} // namespace shift_plan

// Every plan field of ShiftArgs from the input bounds and the output bounds need (shift_plan::
// bounds); the I/O block (the batches and their own bounds) is the caller's.  The caller has
// checked nbits (shift_plan::stages).  HM_ERR_UNSUPPORTED: four waves' slices do not
// fit a CU's LDS.
inline hm_status plan_shift(uint32_t mode, uint32_t nbits, const uint32_t *a_bound,
                            const uint32_t *s_bound, const uint32_t *need, ShiftArgs &A) {
    using namespace shift_plan;
    const uint32_t L = stages(nbits);
    A.mode = mode, A.L = L;
    memset(A.off, 0, sizeof(A.off)), memset(A.soff, 0, sizeof(A.soff));
    // layout, in words.  An input bit's slot holds whole limbs (load_bit); a product's buffer its
    // factors' words at their bounds (wave_mul writes nu + nv <= bound / 32 + 2 words), and so
    // does a slot, which covers the limbs of its input bit (need[i] >= a_bound[i]).
    uint64_t o = 0;
    A.oN = 0, o = even((uint64_t)nbits + 8 + nbits / 2);
    for (uint32_t t = 0; t < L; ++t) {
        A.soff[t] = (uint32_t)o;
        o += 2 * (uint64_t)cap_of(s_bound[t]);
    }
    uint64_t cV = 0, widest = 2;
    uint32_t amax = 0;
    for (uint32_t i = 0; i < nbits; ++i) {
        const uint64_t slot = even((uint64_t)need[i] / 32 + 2);
        A.off[i] = (uint32_t)cV;
        cV += slot;
        widest = slot > widest ? slot : widest;
        amax = a_bound[i] > amax ? a_bound[i] : amax;
    }
    // a rotate's stage t saves the 2^t bits that wrap, at its input's bound: the stages above it
    // have run (the wide steps first), so that is the amount bounds above t plus the widest a
    uint64_t save = 0, above = 0;
    memset(A.sv, 0, sizeof(A.sv));
    for (uint32_t t = L; t-- > 0;) {
        if (mode == kShiftRotl || mode == kShiftRotr) {
            A.sv[t] = (uint32_t)even((above + amax) / 32 + 2);
            const uint64_t area = ((uint64_t)1 << t) * A.sv[t];
            save = area > save ? area : save;
        }
        above += s_bound[t];
    }
    const uint64_t oX = o, oT = oX + widest, oS = oT + widest, oV = oS + save, total = oV + cV;
    if (total > 0xFFFFFFFFu) return HM_ERR_UNSUPPORTED;
    A.oX = (uint32_t)oX, A.oT = (uint32_t)oT, A.oS = (uint32_t)oS, A.oV = (uint32_t)oV;
    A.cV = (uint32_t)cV;
    A.lds_per_wave = (uint32_t)total;
    return lds_status(A.lds_per_wave);
}

} // namespace hm
