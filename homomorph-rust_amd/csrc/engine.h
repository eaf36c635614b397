// engine.h — argument blocks shared by the HIP kernels (kernels.hip) and the C-ABI host code
// (capi.cpp; the adder's plan fields are filled by add_host.h, the multiplier's by
// mul_plan.h and mul_host.cpp).  Plain structs passed to kernels by value.
#pragma once
#include <stdint.h>

#include "../../include/homomorph_gpu.h"

namespace hm {

// Per-bit-position degree bounds of a batch (cap = bound/64 + 1 limbs).  Passed by value; kernels
// derive limb offsets with a running prefix sum.
struct Bounds {
    uint32_t b[HM_MAX_BITS];
};

// Kernel timer (hm_ctx_set_kernel_timing): device wall-clock stamps of one launch, in the slot
// the host gave it (one slot per launch made or captured while timing is on, so every launch of a
// captured K-step graph has its own).  Each wave's lane 0 stamps its start into t0[w] and its end
// into t1[w] (w = the wave's index in the grid, modulo kTimerWaves; relaxed min / max atomics on
// distinct addresses, nothing waits on them); the host takes the slot's earliest start and latest end.
struct KTimer {
    unsigned long long *t0; // null: timing off
    unsigned long long *t1;
};

struct BatchArg {
    uint64_t *limbs;
    uint32_t *degree;
    uint64_t stride;  // limbs per value
    uint32_t dstride; // degree words per value (the batch's nbits; a low-bits view keeps it)
};

// limbs of a ciphertext bit at a degree bound (host and device)
__attribute__((always_inline)) constexpr uint32_t cap_of(uint32_t bound) { return bound / 64 + 1; }
// words of a polynomial at a degree bound (negative: always null; host planning)
constexpr uint32_t words_of_bound(int64_t b) { return b < 0 ? 0u : (uint32_t)(b / 32 + 1); }

// Fused adder, two launches.  add_prep_kernel (several waves per value, lanes over (bit, word))
// validates the inputs and computes every per-bit product ab_i = a_i b_i and P_i = x_i (1 ^ ab_i)
// into a global workspace; add_chain_kernel (one wave per value) runs the sequential carry chain.
// Workspace per value (ws_stride words): [ab slots: nbits*cntAB][P slots: nbits*cntP]
// [deg(ab)+1: nbits][deg(P)+1: nbits].
struct AddArgs {
    BatchArg a, b, out;
    uint64_t n;
    uint32_t nbits;
    uint32_t *ws;
    uint64_t ws_stride;               // words per value
    uint32_t cntA, cntB, cntAB, cntP; // slot sizes in words (cntA = 2*max cap of a, ...)
    uint32_t cntX;                    // words of x_i = a_i ^ b_i (masked at the degrees)
    uint32_t top1;                    // prep: word cntX - 1 of every a_i, b_i, x_i is 0 or 1 (the
                                      // bounds' maximum is a multiple of 32): no product rows for it
    uint32_t wpv;                     // prep: waves per value (bits are dealt round-robin)
    uint32_t vpw;                     // prep: > 1: values per wave instead (whole values, L = 2^lgL)
    uint32_t lgL;                     // prep: log2 nbits when vpw > 1
    uint32_t ucap;                    // prep: > 0: every bit of a and of b has the one bound
                                      // 64 (ucap - 1), ucap limbs (add_prep_uniform_kernel<ucap>:
                                      // cntA = cntB = 2 ucap, cntX = 2 ucap - 1, cntAB = 4 ucap - 3,
                                      // cntP = 6 ucap - 5, one value per wave or less)
    uint32_t prep_lds;                // prep: LDS words per wave
    uint32_t chain_lds;               // chain: LDS words per wave
    uint32_t staged;                  // chain: x, ab, P and degrees staged in LDS, carry in place
    uint32_t cw;                      // chain: carry buffer words
    uint32_t max_prod_words;          // widest carry product along the chain (picks WMAX)
    uint32_t pad;                     // carry buffers zero-padded: unchecked window reads (add_host)
    uint32_t mfma;                    // chain on the matrix cores (adder_mfma.hip): its chunk count
                                      // NC (MfmaCfg), 0 = the VALU chain
    uint32_t mf_cw;                   // MFMA chain: carry bit words (tiles, window overhang)
    int *status;
    Bounds ab, bb, ob;
    KTimer kt; // the carry-chain kernel's launches
};

struct EncArgs {
    const uint64_t *pk;     // tau * pk_cap limbs
    const uint64_t *pk_tab; // nibble table [ceil(tau/4)][limb pair][16][2] (upload_pk), or null
    const uint64_t *pk_tab1; // the same over limbs 0 .. pk_cap - 2 (top1 keys), or null
    uint32_t cus;           // compute units (grid sizing)
    uint32_t tau, pk_cap;
    const uint8_t *data;
    uint32_t nbytes;
    int lognbits;           // log2(8*nbytes) when a power of two, else -1
    uint32_t uniform_cap;   // every output bit has exactly pk_cap limbs: stores go through LDS
    const uint8_t *masks;
    BatchArg out;
    uint64_t n;
    int *status;
    Bounds ob;
    Bounds ooff;            // limb offset of each bit within a value (prefix sums of the caps)
    // every row's top limb (pk_cap - 1) is 0 or 1 (tau <= 128): that limb of a subset sum is
    // parity(mask & topcol), topcol bit i = row i's bit 64 (pk_cap - 1) (cipher.hip enc_bits_t128)
    uint32_t top1;
    uint32_t topcol[4];
    uint64_t *nonce_bump; // non-null: advance this CSPRNG nonce (the masks were just drawn)
    KTimer kt;
};

struct DecArgs {
    BatchArg in;
    uint64_t n;
    uint32_t nbits;
    const uint64_t *z; // z_k = (X^k mod S)(0), bit-packed, zlimbs limbs
    uint32_t zlimbs;
    uint8_t *out;
    int *status;
    Bounds ib;
    Bounds ioff;     // limb offset of each bit within a value (prefix sums of the caps)
    uint32_t maxcap; // widest bit (limbs): picks lane-per-bit or wave-per-value
    uint32_t ucap;   // every bit has exactly ucap <= 8 limbs (fresh ciphertexts), else 0
    KTimer kt;
};

// The wave-per-value circuits (kernels.hip: gates, borrow chain, min / max, select, lookup, shift,
// bit counts) keep their intermediates in LDS, one wavefront per value, in a slice of lds_per_wave
// words whose layout the host plans (circuit_host.h, lookup_host.h, shift_host.h,
// bitcount_host.h, array_host.h).  What their argument
// blocks share, filled by capi.cpp fill_io: the operands, the output and their static bounds.
struct CircuitIO {
    BatchArg a, b, out; // b: the second operand (a shift's amount; a unary gate has none)
    uint64_t n;
    uint32_t nbits;     // bits of a (a comparison's output has 8, the amount its own width)
    int *status;
    Bounds ab, bb, ob;
};

struct GateArgs {
    int op;
    uint32_t lds_per_wave, oA, oB, oT; // circuit_host.h plan_gate
    CircuitIO io;
};

// Ripple-borrow chain (kernels.hip borrow_kernel): subtraction, the four orderings and equality,
// one wavefront per value, everything in LDS.  The host exchanges the operands
// for > and <=, so the kernel knows three chains and a constant:
//   kBorrowSub  out_i = x_i + w_i, w_{i+1} = a_i b_i + b_i + p_i w_i   (x = a + b, p = x + 1)
//   kBorrowLt   the same borrows through bit nbits - 1; the result is w_nbits (+ 1 when flip)
//   kBorrowEq   e_{i+1} = p_i e_i from e_0 = 1; the result is e_nbits (+ 1 when flip)
enum { kBorrowSub = 0, kBorrowLt = 1, kBorrowEq = 2 };
// A wave's LDS slice on that chain, word offsets (circuit_host.h plan_borrow):
// a_i | b_i | x_i | p_i | generate term | two borrow buffers of cw words each at oW
struct BorrowLayout {
    uint32_t lds_per_wave, oA, oB, oX, oP, oG, oW;
    uint32_t cw;
};
struct BorrowArgs {
    int mode;          // kBorrowSub / kBorrowLt / kBorrowEq
    uint32_t flip;     // comparisons: the result plus the unit polynomial (>=, <=, !=)
    uint32_t sgn;      // kBorrowLt on a signed type: bit nbits - 1 generates a_i b_i + a_i
    BorrowLayout lay;
    CircuitIO io;
};

// min / max on the same chain (kernels.hip minmax_kernel), one wavefront per
// value in the same BorrowLayout.  Phase 1 is the kBorrowLt chain: it leaves w_nbits (the
// polynomial a < b returns) in one borrow buffer.  Phase 2 walks the bits again:
//   min  out_i = b_i + w_nbits x_i      max  out_i = a_i + w_nbits x_i      (x = a + b)
// each product formed into the other borrow buffer and stored from there.
struct MinMaxArgs {
    uint32_t is_max;   // phase 2 adds a_i (max) instead of b_i (min)
    uint32_t sgn;      // signed type: bit nbits - 1 generates a_i b_i + a_i
    BorrowLayout lay;  // cw: the widest of p_i w_i and x_i w_nbits
    CircuitIO io;
};

// Oblivious choice (kernels.hip select_kernel): out_i = b_i + c x_i with c bit 0
// of a Ciphered<bool> (its bits 1..7 are not read), one wavefront per value.  c is loaded once per
// value; per bit a_i, b_i and x_i are formed in LDS and one product goes to the buffer at oT.
struct SelectArgs {
    BatchArg cond;     // (8 bits; a, b and out have io.nbits)
    uint32_t cbound;   // degree bound of cond's bit 0
    uint32_t lds_per_wave, oC, oA, oB, oX, oT; // word offsets in a wave's LDS slice (plan_select)
    CircuitIO io;
};

// Table lookup (kernels.hip lookup_kernel): out = T[v] for the k <= 8 low bits v
// of a value and a plaintext table T, as the algebraic normal form of every output bit,
//   out_j = sum over the sets S with coef[j] bit S of prod_{i in S} a_i,
// one wavefront per value.  The index bits are split into a low half (kl = ceil(k / 2) bits) and a
// high half (kh bits); the monomials of either half are formed once per value by doubling
// (M[s | 1 << i] = M[s] a_i), then out_j = sum_t MH[t] I_jt with the inner sums
// I_jt = sum_s coef[j][t 2^kl + s] ML[s] plain XORs: at most 2^kh - 1 products per output bit.
// Everything below is filled by lookup_host.h plan_lookup.  A monomial's index is s for the low
// half and 16 + t for the high half (off, need and the word counts at oN); ML[0] = MH[0] = the unit
// polynomial, one shared word.  The coefficient masks travel by value: every index into them, as
// into off, ab and ob, is wave-uniform (dev_common.h).
constexpr uint32_t kLookupMaxIn = 8;   // index bits
constexpr uint32_t kLookupMaxOut = 32; // output bits
struct LookupArgs {
    BatchArg a, out;
    uint64_t n;
    uint32_t k, kl, kh;  // index bits: all, low half, high half
    uint32_t nob;        // output bits
    uint32_t need;       // monomials some output bit uses (with the ones they are formed from)
    // word offsets in a wave's LDS slice: the monomials' word counts (32 words) | the unit | the
    // monomials | an inner sum of cI words | two accumulators of cP words each
    uint32_t lds_per_wave, oN, oI, oP, cI, cP;
    uint32_t off[32];
    uint32_t coef[kLookupMaxOut][8]; // bit S of coef[j]: the monomial of the index bits in S
    uint32_t ab[kLookupMaxIn], ob[kLookupMaxOut];
    int *status;
};

// Shift or rotate by an encrypted amount (kernels.hip shift_kernel): a barrel
// shifter of L = log2 nbits stages, one per amount bit s_t, step k = 2^t,
//   y_i = x_i + s_t (x_i + x_src(i)),      src = shift_src(mode, nbits, k, i),
// one wavefront per value.  The whole value lives in the wave's LDS slice across the stages, IN
// PLACE, one slot per bit sized by its output bound.  The stages run from the widest step down
// (they commute); a stage walks the bits away from its sources (from the top bit down when
// src < i: SHL, ROTL; from bit 0 up otherwise), so a source is read before its slot is rewritten;
// a rotate first saves the k bits that wrap around (k slots at that stage's input bound: small,
// because the wide steps come first).  Each product is formed in a one-bit buffer and copied to
// its slot; the last stage whose s_t is not null sends its products to the output instead.  A
// null s_t leaves the value where it is.  Everything below but io (the amount is its second
// operand: the low L bits of io.b, at the bounds io.bb) is filled by shift_host.h plan_shift.  The
// bounds and the slot offsets travel by value: every index into them is wave-uniform
// (dev_common.h).
enum { kShiftShl = 0, kShiftShr = 1, kShiftSar = 2, kShiftRotl = 3, kShiftRotr = 4 };
constexpr uint32_t kShiftMaxStages = 7; // log2 HM_MAX_BITS
// The bit a stage of step k mixes into bit i of an nbits-bit value; -1: the null polynomial.
__attribute__((always_inline)) constexpr int32_t shift_src(uint32_t mode, uint32_t nbits, uint32_t k, uint32_t i) {
    switch (mode) {
    case kShiftShl: return i >= k ? (int32_t)(i - k) : -1;
    case kShiftShr: return i + k < nbits ? (int32_t)(i + k) : -1;
    case kShiftSar: return i + k < nbits ? (int32_t)(i + k) : (int32_t)(nbits - 1);
    case kShiftRotl: return (int32_t)((i + nbits - k) & (nbits - 1));
    default: return (int32_t)((i + k) & (nbits - 1)); // kShiftRotr
    }
}
struct ShiftArgs {
    uint32_t mode;      // kShiftShl .. kShiftRotr
    uint32_t L;         // log2 io.nbits (a power of two in 2..128)
    // word offsets in a wave's LDS slice: word counts (nbits of the value's bits, 8 of the amount
    // bits, nbits / 2 of the saved bits) | the amount bits at soff[t] | x_i + x_src | the one-bit
    // product buffer | the saved bits of a rotate's stage t, sv[t] words each, at oS | the value
    // at oV, bit i at off[i], cV words in all
    uint32_t lds_per_wave, oN, oX, oT, oS, oV, cV;
    uint32_t sv[kShiftMaxStages];
    uint32_t soff[kShiftMaxStages];
    uint32_t off[HM_MAX_BITS];
    CircuitIO io;
};
// Bit counts (kernels.hip bitcount_kernel and bitrun_kernel): count_ones /
// count_zeros and the leading / trailing runs of an n-bit value as a Ciphered<u8>, one wavefront
// per value.  Both work on literals u_i = x_i (the "ones" ops) or x_i + 1 (zeros).
//   counts  out_k = e_{2^k}(u_0 .. u_{n-1}), the elementary symmetric polynomial, by the recurrence
//           E_j <- E_j + u_i E_{j-1} (j descending, E_0 = 1), one literal after another.  E_j lives
//           in slot j <= J of the wave's LDS slice; for n a power of two the top target e_n is the
//           running product of all literals, kept past J in two ping-pong buffers (the diagonal).
//           An update runs only while bitcount_needed says some target still reads its result.
//   runs    the literals in the run's order (leading: from the top bit down), t_j = v_1 .. v_j in
//           two ping-pong buffers, out_k = the sum of t_{m 2^k}: one accumulator per output bit.
// Everything below but io (a is its first operand; it has no second) is filled by bitcount_host.h
// plan_bitcount.  The slot offsets travel by value: every index into them, as into io.ab and
// io.ob, is wave-uniform (dev_common.h).
constexpr uint32_t kBitCountMaxSlots = HM_MAX_BITS / 2; // E_1 .. E_64 (n = 65 .. 128)
constexpr uint32_t kBitCountOut = 8;                    // bits of the Ciphered<u8>
// After i literals of n, is E_j (1 <= j <= i) still read by some target T = 2^k <= n?  The
// recurrence reaches E_T^(n) from E_j^(i) only over j <= T with T - j of the n - i literals left.
__attribute__((always_inline)) constexpr bool bitcount_needed(uint32_t n, uint32_t i, uint32_t j) {
    for (uint32_t T = 1; T <= n; T <<= 1)
        if (j <= T && T - j <= n - i) return true;
    return false;
}
struct BitCountArgs {
    uint32_t zeros;    // the literal is x_i + 1
    uint32_t leading;  // runs: the literals from the top bit down
    uint32_t K;        // output bits that are not null by rule: floor(log2 n) + 1
    uint32_t J;        // counts: slots E_1 .. E_J (n / 2 for a power of two n >= 2, else 2^(K-1))
    uint32_t diag;     // counts: the target 2^(K-1) = n is the running product, past slot J
    uint32_t a_limbs;  // limbs of one value of a (a leading run reads its bits from the top down)
    // word offsets in a wave's LDS slice: word counts (kBitCountMaxSlots + 1 of the slots, 8 of the
    // accumulators) | the literal | the product buffer (counts) | two ping-pong buffers of cD words
    // each (the diagonal, the run's prefix) | the slots E_j at off[j] (counts), the accumulators
    // of output bit k at off[k] (runs), from oE
    uint32_t lds_per_wave, oN, oU, oT, oD, cD, oE;
    uint32_t off[kBitCountMaxSlots + 1];
    CircuitIO io;
};
// Oblivious array read and write by an encrypted index (kernels.hip array_read_kernel and
// array_write_kernel), one wavefront per index value.  An array of count
// elements is count consecutive values of an ordinary batch: element v of array e is value
// e count + v (a shared table: value v).  k = ceil(log2 count) index bits s_0 .. s_{k-1} are read.
//   read   out_j = sum_v ind_v T_{v,j} as a multiplexer tree, one output bit at a time: the
//          elements are walked in order, a level-t node (2^t elements) either parks in slot t as
//          a waiting left child or is joined with the parked one, y = L + s_t (L + R), and rises.
//          A right sibling past the array is the null polynomial.
//   write  out_{v,j} = T_{v,j} + ind_v (x_j + T_{v,j}), ind_v = prod_t (s_t or s_t + 1) kept as
//          the suffix products Q_t = prod_{i >= t} lit_i(v) in k slots: stepping v recomputes
//          only the levels at or below its lowest set bit.  x's bits stay in LDS for the value.
// Everything below but io is filled by array_host.h plan_array_read / plan_array_write.  The slot
// offsets and bounds travel by value: every index into them is wave-uniform (dev_common.h).
constexpr uint32_t kArrayMaxIndex = 8;   // index bits
constexpr uint32_t kArrayMaxCount = 256; // elements
struct ArrayReadArgs {
    uint32_t count, k;
    uint32_t shared;    // arr holds one table of count values, read by every index
    // word offsets in a wave's LDS slice: word counts (8 of the index bits, 8 of the slots) | the
    // index bits at soff[t] | an odd element's bit | L + R | two ping-pong product buffers of cP
    // words each | the waiting left children, level t at slot[t]
    uint32_t lds_per_wave, oN, oL, oX, oP, cP;
    uint32_t soff[kArrayMaxIndex];
    uint32_t slot[kArrayMaxIndex];
    CircuitIO io;       // a: the array batch, b: the index (its low k bits), n: index values
};
struct ArrayWriteArgs {
    uint32_t count, k;
    // word offsets in a wave's LDS slice: word counts (8 of the index bits, 8 of the suffix
    // products, nbits of x's bits) | the index bits at soff[t] | the literal | the element's bit |
    // x_j + T_j | the product | the suffix products at qoff[t] | x's bits, whole limbs, at oV
    uint32_t lds_per_wave, oN, oU, oT, oX, oO, oV;
    uint32_t soff[kArrayMaxIndex];
    uint32_t qoff[kArrayMaxIndex];
    uint32_t sb[kArrayMaxIndex]; // the index bits' bounds
    BatchArg idx;                // the index (its low k bits)
    CircuitIO io;                // a: the array batch, b: the value written, n: index values
};
static_assert(sizeof(ShiftArgs) < 4096 && sizeof(LookupArgs) < 4096 && sizeof(SelectArgs) < 4096 &&
                  sizeof(BorrowArgs) < 4096 && sizeof(MinMaxArgs) < 4096 && sizeof(GateArgs) < 4096 &&
                  sizeof(BitCountArgs) < 4096 && sizeof(ArrayReadArgs) < 4096 &&
                  sizeof(ArrayWriteArgs) < 4096,
              "kernarg limit");

// Column-parallel carry-save multiplier (mul_engine.hip, mul_plan.h).  Column i of
// mul_unsigned_internal (common.rs:66-105) XORs its items x_0..x_{n-1} (the partial products
// a_j b_{i-j}, then the previous column's carries) into result_i and pushes the carry
// (x_0 ^ .. ^ x_{t-1}) * x_t before each XOR.  With the prefixes p_t = x_0 ^ .. ^ x_{t-1}
// materialised (a scan), every carry of a column is an independent product p_t * x_t, so a column
// is three launches over the whole batch: partial products, prefix scan (its last prefix is the
// output bit), and the carry products, tiled over the chip.  Polynomials live in a per-value
// arena of u32 words at static offsets (slots, capacity = bound/32 + 1 rounded up to 4 words,
// always zero above the degree); deg1[slot * nv + e] = degree + 1 of value e (0 = null).
struct MulSlot {
    uint32_t off;   // u32-word offset in a value's arena
    uint32_t words; // capacity (multiple of 4)
};
struct MulBase {
    uint32_t *arena;
    uint64_t astride; // arena words per value
    uint32_t *deg1;
    uint64_t nv;      // values in this chunk (deg1 row length)
    const MulSlot *slots;
    uint64_t e0;      // first value of the chunk in the caller's batches
    int *status;
};
struct MulStageArgs {
    MulBase B;
    BatchArg a, b;
    uint32_t K;       // input bits staged: a_j -> slot j, b_j -> slot K + j
    Bounds ab, bb;
};
struct MulPPTask {
    uint32_t a, b, out, flip; // out = a * b (+1 when flip: mul_signed_internal, common.rs:123-126)
};
struct MulPPArgs {
    MulBase B;
    const MulPPTask *tasks;
    uint32_t ntasks;
};
struct MulScanArgs {
    MulBase B;
    const uint32_t *items;  // nitems slot ids, in the reference's XOR order
    const uint32_t *prefix; // nitems - 1 slot ids: p_1 .. p_{n-1}
    uint32_t nitems;
    uint32_t chunks;        // 256-word chunks per value (of the widest prefix)
    uint32_t res;           // degree slot of the result (output bit i)
    BatchArg out;
    uint32_t out_off, out_cap; // output bit i: limb offset within a value, capacity in limbs
};
struct MulProdTask {
    uint32_t u, v, out; // out = u * v; u is the operand with fewer words (the uniform one)
};
struct MulTile {
    uint32_t task, base; // output words [base, base + 64 W) of task
};
// One span of an MFMA schoolbook product, resolved on the host (mul_plan.h build_plan): the
// operands' and the output's arena offsets and slots, so a wave's only dependent loads after this
// one record are the operands' degrees (instead of span -> task -> slots -> degrees).
struct MulSpanRec {
    uint32_t uoff, voff, ooff, nout; // arena offsets; output slot capacity (words)
    uint32_t uslot, vslot, oslot;    // slots (the operands' degrees; the output's, written)
    uint32_t base;                   // first output word of the span
};
struct MulProdArgs {
    MulBase B;
    const MulProdTask *tasks;
    const MulTile *tiles;
    uint32_t ntiles;
};
// Karatsuba products (mul_plan.h "Karatsuba"): the big carries p_t * x_t of the deep columns
// run as a recursion over arena VIEWS (u32-word ranges of a value's arena; words past `valid`
// read as zero).  Level by level: sums of halves (KaSum), leaf products (MulVTask, schoolbook
// tiles), and recombination R = z0 + (z0 + z1 + z2) X^h + z1 X^2h (KaComb).
struct KaSum {
    uint32_t src, valid; // operand view (arena words)
    uint32_t dst;        // dst[0:h) = src[0:h) ^ src[h:2h)
};
struct KaSumArgs {
    MulBase B;
    const KaSum *t;
    uint32_t nt, h;
};
struct MulVTask {
    uint32_t u, nu, v, nv; // operand views (nu, nv valid words; 0 = null)
    uint32_t out, nout;    // out[0:nout) = U * V
    // MFMA leaves of the deepest Karatsuba level read a sum operand lo + hi as two views:
    // U = u[0:nu) ^ u2[0:nu2) (nu2 <= nu; nu2 = 0: no second view), the same for V
    uint32_t u2, nu2, v2, nv2;
};
struct MulVTile {
    uint32_t task, base;
};
struct MulVProdArgs {
    MulBase B;
    const MulVTask *tasks;
    const MulVTile *tiles;
    uint32_t ntiles;
};
// Carry products on the matrix cores (mul_mfma.hip): one wave per (value, task, span of `span`
// output tiles of 32 words; a leaf's whole output, kMfSpan tiles of a schoolbook product), U in
// blocks of kMfUB words.  Tasks are the Karatsuba leaves (MulVTask;
// nspans uniform spans per task) or the column plan's schoolbook products (MulProdTask, with an
// explicit span list {task, first output word}); vmax = the largest V of the launch (words).
constexpr int kMfUB = 256;
constexpr int kMfSpan = 16;
// the narrow class of schoolbook carries: U of at most kMfNarrowWords words, launched apart from
// the wide ones (mul_mfma_kernel<false, true>: 4 waves per SIMD), spans of at most kMfNarrowSpan
// tiles so that 16 waves' LDS slices fit a CU
#ifndef HM_MF_NARROW_WORDS
#define HM_MF_NARROW_WORDS 72
#endif
#ifndef HM_MF_NARROW_SPAN
#define HM_MF_NARROW_SPAN 10
#endif
constexpr uint32_t kMfNarrowWords = HM_MF_NARROW_WORDS;
// ... and within it the tiny class, U of at most kMfTinyWords words (the 17-word partial products
// of fresh d + d' = 512 ciphertexts and carries by them, in slots of 20 words): at most
// kMfTinyWords / 2 + 1 chunks, so its instance (mul_mfma_kernel<false, true, false, 11>) holds
// 11 A fragments, not 17, and fits more waves per SIMD (HM_MFT_WPE)
#ifndef HM_MF_TINY_WORDS
#define HM_MF_TINY_WORDS 20
#endif
constexpr uint32_t kMfTinyWords = HM_MF_TINY_WORDS;
constexpr int kMfTinyChunks = (int)kMfTinyWords / 2 + 1;
constexpr uint32_t kMfNarrowSpan = HM_MF_NARROW_SPAN;
#ifndef HM_MF_WIDE_SPAN
#define HM_MF_WIDE_SPAN 16
#endif
constexpr uint32_t kMfWideSpan = HM_MF_WIDE_SPAN; // tiles per wave of the wide class
// the wide class on the lean windowed instance (mul_mfma_kernel<false, true, true>): configs[4]
// 897.7-901.0 -> 895.4-895.5 ms per 2^20 (spans of 12 tiles: 899-904, 8: 908-909)
#ifndef HM_MF_WIDE_LEAN
#define HM_MF_WIDE_LEAN 1
#endif
constexpr bool kMfWideLean = HM_MF_WIDE_LEAN;
// Karatsuba leaves of at most kMfLeanLeafWords words run on mul_mfma_kernel<true, true> (per-group
// U windows, one tile at a time, 4 waves per SIMD): configs[4]'s 224-word leaves 916-919 -> 911-913
// ms per 2^20; K = 16's 256-word leaves measured 0.5 % slower on it (336-338 -> 338-339 ms), so
// they stay on the 3-wave instance
#ifndef HM_MF_LEAN_LEAF_WORDS
#define HM_MF_LEAN_LEAF_WORDS 224
#endif
constexpr uint32_t kMfLeanLeafWords = HM_MF_LEAN_LEAF_WORDS;
#ifndef HM_MF_LEAN_LEAF_MIN
#define HM_MF_LEAN_LEAF_MIN 193 // leaves narrower than this stay on the 3-wave instance (K = 16: 3,336-3,354 -> 3,389-3,406/s; configs[4]'s 224-word leaves unchanged)
#endif
constexpr uint32_t kMfLeanLeafMin = HM_MF_LEAN_LEAF_MIN;
struct MulMfmaArgs {
    MulBase B;
    const void *tasks;
    const MulTile *spans; // schoolbook products: {task, base}
    const MulSpanRec *recs; // ... the same spans resolved (MulSpanRec), used by the MFMA kernels
    uint32_t nitems;      // work items per value (leaves: tasks x nspans)
    uint32_t nspans;      // leaves: spans per task
    uint32_t span;        // output tiles per span
    uint32_t vmax, wave_words;
    uint32_t umax;        // largest U (words; blocks of at most kMfUB): sizes the U image
    uint32_t lean;        // leaves: the lean instance (per-group U windows, 4 waves per SIMD)
    uint32_t per_wave;    // work items per wave (set by launch_mul_mfma)
};
// A wave's LDS slice of the MFMA product kernels, in words: the kernels (mul_mfma.hip) lay their
// slices out with these functions and the host (mul_plan.h) sizes the launches with them.
constexpr int kMfG = 16;             // chunks per full A group (64 VGPRs of A fragments)
constexpr int kVPad = 2 * kMfG + 32; // V words read beyond V's ends (zero)
// U blocks of at most ub = min(umax, kMfUB) words: the launch's LDS slices are sized for them
// (a launch of narrow schoolbook products reserves no 256-word U image, so more waves fit a CU)
constexpr uint32_t mf_ub(uint32_t umax) { return umax < kMfUB ? umax : kMfUB; }
constexpr uint32_t mf_rs_words(uint32_t umax) { return 4 * (mf_ub(umax) + 2) + 16; }
// V words one (block, span) reaches: 32 span + 32 + 2 NC (NC <= ub/2 + 1), or all of V plus its
// zero pads when that is fewer
constexpr uint32_t mf_vi_words(uint32_t vmax, uint32_t span, uint32_t umax) {
    const uint32_t a = 32 * span + 32 + 2 * (mf_ub(umax) / 2 + 1), b = vmax + 2 * kVPad;
    return 4 * ((a < b ? a : b) + 8);
}
constexpr uint32_t mf_wave_words(uint32_t vmax, uint32_t span, uint32_t umax) {
    return mf_rs_words(umax) + mf_vi_words(vmax, span, umax) + 32 * span;
}
// the U image of the windowed (lean) instances: one group of G chunks' window, RS quads
// Qlo = 2 c0 + 1 .. Qlo + 2G + 1 (mul_mfma.hip mf_win_word)
constexpr uint32_t mf_win_words(int G) { return 4u * (2u * (uint32_t)G + 2u) + 16u; }
// Partial products grouped by their shared factor a_j (mul_mfma.hip mul_ppg_kernel): every
// a_j * b_k of the plan in one launch before the columns, one wave per (value, a_j), a_j's A
// fragments built once for all of its products (a_j within kMfPPGWords words: one chunk group of
// at most kMfPPGWords / 2 + 1 = 17 chunks, as many as the kernel holds A fragments for; 34 words
// would be 18).  Wider operands take the per-column launches (mul_plan.h ppm).
constexpr uint32_t kMfPPGWords = 33;
// b_k words staged per batch of partial products (mul_ppg_kernel: kMfPPGBatch x 64 LDS words)
constexpr uint32_t kMfPPGBatch = 8;
struct MulPPGroup {
    uint32_t u;            // slot of a_j (the shared factor)
    uint32_t first, count; // its products: items [first, first + count)
};
struct MulPPItem {
    uint32_t v, out;       // b_k's slot, the product's slot
};
struct MulPPGArgs {
    MulBase B;
    const MulPPGroup *groups;
    const MulPPItem *items;
    uint32_t ngroups;                 // groups per value
    uint32_t umax, vmax, span;        // largest factor, other factor (words), output tiles
    uint32_t wave_words;
};
// The same partial products on the VALU by product rows (mul_engine.hip mul_ppv_kernel, the adder
// prep's method): one wave per value stages the input slots 0 .. nin - 1 into its LDS, computes
// every a_j * b_k of the plan (tasks, flattened from the groups) with lanes over (product, word of
// a_j) rows -- 16 v_mad_u64_u32 per 32x32 product, rows meeting in LDS by ds_xor -- and writes
// the products and their degrees.  For fresh operands of at most kPPVWords words (d + d' <= 256),
// where a product is only 5 MFMA chunks and the MFMA form is latency-bound (r05: 0.15 busy).
#ifndef HM_PPV_WORDS
#define HM_PPV_WORDS 12
#endif
constexpr uint32_t kPPVWords = HM_PPV_WORDS;
struct MulPPVArgs {
    MulBase B;
    const MulPPTask *tasks; // {u slot (a_j), v slot (b_k), out slot, 0}
    uint32_t ntasks;
    uint32_t nin;        // input slots staged (2 K: a_j, b_j)
    uint32_t inw;        // LDS words per staged input slot (>= every input slot's capacity)
    uint32_t qw;         // rows per product: the widest a_j (words)
    uint32_t outw;       // LDS words per product (>= qw + the widest b_k + 1)
    uint32_t wave_words; // LDS words per wave
};
// Small schoolbook carry products on the VALU by rows (mul_engine.hip mul_rows_kernel): one wave
// per value, a column's products whose operands fit kRowsU x kRowsV words (slot capacities; the
// 17 x 17 and 17 x 33-word carries of the u8 multiply's columns at d + d' = 256, MFMA "tiny" class
// before), each product's operands staged in the wave's LDS, rows (product, word of u) as in
// mul_ppv_kernel.  LDS per task: uw + vw + ow + 2 words.
#ifndef HM_ROWS_U
#define HM_ROWS_U 20
#endif
#ifndef HM_ROWS_V
#define HM_ROWS_V 36
#endif
constexpr uint32_t kRowsU = HM_ROWS_U, kRowsV = HM_ROWS_V;
struct MulRowArgs {
    MulBase B;
    const MulSpanRec *recs; // resolved tasks: u / v / out offsets, out words, slots; base =
                            // u words | v words << 16 (slot capacities)
    uint32_t ntasks;
    uint32_t uw, vw, ow;      // LDS words per task's u, v and product (slot capacities)
    uint32_t qw;              // rows per task: the widest u's words at its degree bound (<= uw)
    uint32_t wave_words;
};
constexpr uint32_t kKaNone = 0xFFFFFFFFu; // a z1 that is null (the high halves were all zero)
struct KaComb {
    uint32_t z0, z1, z2; // child results, 2h words each (z1 may be kKaNone)
    uint32_t r, rcap;    // parent result: r[0:min(4h, rcap))
};
struct KaCombArgs {
    MulBase B;
    const KaComb *t;
    uint32_t nt, h;
};
struct MulDegArgs { // deg1[out] of an exact product from its operands' deg1 (null -> 0)
    MulBase B;
    uint32_t u, v, out;
};

struct MulFinalArgs {
    MulBase B;
    const uint32_t *res; // K degree slots of the output bits
    uint32_t K;
    BatchArg out;
    Bounds ob;
};

struct PolyArgs {
    const uint64_t *a;
    const uint32_t *adeg;
    uint32_t acap;
    const uint64_t *b;
    const uint32_t *bdeg;
    uint32_t bcap;
    uint64_t *out;
    uint32_t *odeg;
    uint32_t ocap;
    uint64_t n;
    int *status;
};

// Device CSPRNG: ChaCha20 (20 rounds, 256-bit key, 64-bit block counter, 64-bit nonce read from
// *nonce and advanced by one per draw).  Block b of the draw fills bytes [64b, 64b + 64).
struct RandArgs {
    uint32_t key[8];
    uint64_t *nonce;
    uint8_t *out;
    uint64_t nbytes;
};

// host-side launchers (kernels.hip)
// bump false: the nonce is left for the caller's next launch to advance (EncArgs::nonce_bump)
int launch_random(const RandArgs &a, void *stream, bool bump = true);
int launch_add(const AddArgs &a, void *stream);
int launch_add_prep(const AddArgs &a, void *stream);
// the same add over values [e0, e0 + n) of a batch: argument block with every pointer advanced
AddArgs add_args_slice(const AddArgs &a, uint64_t e0, uint64_t n);
int launch_add_chain_mfma(const AddArgs &a, void *stream);
int launch_add_chain_valu(const AddArgs &a, void *stream);
int launch_encrypt(const EncArgs &a, void *stream);
int launch_decrypt(const DecArgs &a, void *stream);
int launch_gate(const GateArgs &a, void *stream);
int launch_borrow(const BorrowArgs &a, void *stream);
int launch_minmax(const MinMaxArgs &a, void *stream);
int launch_select(const SelectArgs &a, void *stream);
int launch_lookup(const LookupArgs &a, void *stream);
int launch_shift(const ShiftArgs &a, void *stream);
int launch_bitcount(const BitCountArgs &a, void *stream); // count_ones, count_zeros
int launch_bitrun(const BitCountArgs &a, void *stream);   // leading / trailing zeros / ones
int launch_array_read(const ArrayReadArgs &a, void *stream);
int launch_array_write(const ArrayWriteArgs &a, void *stream);
int launch_mul_stage(const MulStageArgs &a, void *stream);
int launch_mul_pp(const MulPPArgs &a, void *stream);
int launch_mul_scan(const MulScanArgs &a, void *stream);
int launch_mul_prod(const MulProdArgs &a, uint32_t w, void *stream);
int launch_mul_final(const MulFinalArgs &a, void *stream);
int launch_ka_sum(const KaSumArgs &a, void *stream);
int launch_mul_vprod(const MulVProdArgs &a, uint32_t w, void *stream);
int launch_mul_mfma(const MulMfmaArgs &a, bool leaf, void *stream);
int launch_mul_ppg(const MulPPGArgs &a, void *stream);
int launch_mul_ppv(const MulPPVArgs &a, void *stream);
int launch_mul_rows(const MulRowArgs &a, void *stream);
int launch_ka_comb(const KaCombArgs &a, void *stream);
int launch_mul_deg(const MulDegArgs &a, void *stream);
constexpr uint32_t kMulTileW[] = {1, 2, 4, 8, 12}; // per-lane tile widths of the product launches
int launch_poly_add(const PolyArgs &a, void *stream);
int launch_poly_mul(const PolyArgs &a, void *stream);
// The remainder table of poly_rem_kernel (kernels.hip): rows j < deg S of tcols limbs, row j's
// limb t = bits 64 (l0 + t) .. of Z_j (bit k = bit j of X^k mod S); zt = null: deg S is above
// every dividend (the remainder is the dividend)
struct RemTable {
    const uint64_t *zt;
    uint32_t rows, l0, tcols;
};
int launch_poly_rem(const PolyArgs &a, const RemTable &t, void *stream);

constexpr int kAddWavesPerBlock = 4;
constexpr uint64_t kAddPipeMin = 1024; // values per half of a pipelined add (hm_ctx_set_add_pipeline)
constexpr uint32_t kTimedLaunches = 128;  // launches hm_ctx_set_kernel_timing can record
constexpr uint32_t kTimerWaves = 32768;   // stamp pairs per launch (waves beyond share them)
// MFMA carry chain (adder_mfma.hip), one configuration per chunk count NC: P_i within 2 NC - 1
// words (NC = 7: 13 words, d + d' <= 128, configs[0]; NC = 13: 25 words, d + d' <= 256; NC = 25:
// 49 words, d + d' <= 512), nibble ring slots
// (a power of two above a tile's 32 + 2 NC word window plus the 32 words filled ahead), zero carry
// words below C (the deepest window reach), a bit's workspace record in one or two 64-word
// LDS-DMAs, and the SIMD occupancy the A fragments (4 NC VGPRs) leave.
constexpr int kMfmaRingSlots = 128;
template <int NC> struct MfmaCfg {
    static constexpr int kChunks = NC;
    static constexpr int kRevWords = 2 * NC + 2;            // > max np + 1 (jb >= 64)
    static constexpr int kRsWords = 4 * kRevWords + 8 * NC + 8;
    static constexpr int kHalo = NC <= 16 ? 32 : 64;        // >= 2 NC - 1
    static constexpr int kRecWords = NC <= 16 ? 64 : 128;
// NC = 25: 3 waves per SIMD (168 VGPRs; 23 dwords spill, all outside the tile loop): configs[4]
// 910.5-911.9 -> 902.8-905.1 ms per 2^20 against 2 waves per SIMD at 197 VGPRs (round 4)
#ifndef HM_MFMA25_WPE
#define HM_MFMA25_WPE 3
#endif
// NC = 7: its 7 A fragments leave room for more waves per SIMD (a u8 add at d + d' = 128 is a
// short chain: more waves hide its per-bit phases)
#ifndef HM_MFMA7_WPE
#define HM_MFMA7_WPE 4
#endif
    static constexpr int kWavesPerEU = NC <= 8 ? HM_MFMA7_WPE : NC <= 16 ? 4 : HM_MFMA25_WPE;
    static constexpr int kStageWords = 2 * kRecWords * kAddWavesPerBlock; // static LDS per block
    // ring slots mirrored past the end (slot s < kMirror also at kMfmaRingSlots + s), so every
    // lane's window of 2 NC - 1 slots is contiguous wherever it starts
#ifndef HM_MIRROR13
#define HM_MIRROR13 32
#endif
    // (a whole-ring mirror at NC = 13, whose two copies need no per-lane test, measured 0.5 %
    // slower: 0.5764 against 0.5726 ms per step; since then the ring's origin moves with the
    // bit and the mirror test is wave-uniform, adder_mfma.hip "Ring slot")
    static constexpr int kMirror = NC <= 16 ? HM_MIRROR13 : 64;
    static constexpr int kRingWords = 4 * (kMfmaRingSlots + kMirror);
    static_assert(2 * NC - 1 <= kMirror, "ring mirror");
    static_assert(32 + 2 * NC + 32 <= kMfmaRingSlots, "ring window");
};
// Top-tile trimming (adder_mfma.hip "HM_CHAIN_TRIM"): chunk c of a bit's top tile T reads carry
// words from 32 T - np + 2 c up, so only its first L = ceil((nc + np - 32 T) / 2) chunks reach the
// carry's nc words.  The kernel has one tile body per bucket of L and runs the smallest bucket
// >= L; add_host.h counts the MFMAs with the same functions.  Buckets, from the full body down:
// NC, 3 s, 2 s, s with s = (NC - 1) / 3 (NC = 13: 13, 12, 8, 4; NC = 7: 7, 6, 4, 2; NC = 25: 25,
// 24, 16, 8).  Fresh operands of d + d' = 32 (NC - 1) / 3 bits have P_i of NC - 1 chunks' words,
// nc + np grows by 3/4 of a tile a bit, and L takes four values s apart, bit after bit: at the
// headline's measured degrees 3-4, 7-8, 11-12 and 13 (DESIGN.md 4.1 has the histogram).
constexpr int chain_top_live(int NC, int nc, int np, int tiles) {
    const int L = (nc + np - 32 * (tiles - 1) + 1) >> 1;
    return L < 0 ? 0 : L > NC ? NC : L;
}
constexpr int kChainTrimBuckets = 4;
constexpr int chain_trim_lc(int NC, int j) { return j == 0 ? NC : (kChainTrimBuckets - j) * ((NC - 1) / 3); }
constexpr int chain_trim_bucket(int NC, int L) {
    int j = kChainTrimBuckets - 1;
    while (chain_trim_lc(NC, j) < L) --j;
    return chain_trim_lc(NC, j);
}
constexpr size_t kEncTableBytes = 96 * 1024; // largest encryption nibble table staged in LDS
                                              // (tau = 256 at d + dp = 512: 80 KB)

} // namespace hm
