// kernels.hip — gfx950 kernels of the gates and the single-polynomial primitives:
//   gate_kernel     elementwise AND/OR/XOR/NOT (common.rs:5-35)
//   borrow_kernel   subtraction, ==, !=, <, <=, >, >= as one ripple-borrow chain (no reference
//                   circuit: DESIGN.md s4.4a)
//   minmax_kernel   min / max: that chain (borrow_step, shared with borrow_kernel), then its last
//                   borrow times a_i + b_i, in one launch (s4.4b)
//   select_kernel   cond ? a : b on an encrypted bool (s4.4b)
//   lookup_kernel   T[v] for a plaintext table T and an encrypted index of up to 8 bits (s4.4c)
//   shift_kernel    <<, >>, rotates by an encrypted amount: a barrel shifter in LDS (s4.4d)
//   bitcount_kernel, bitrun_kernel   count_ones / count_zeros; leading / trailing runs (s4.4e)
//   array_read_kernel, array_write_kernel   arr[i] and arr[i] = x for an encrypted index (s4.4f)
//   poly_* kernels single-polynomial primitives for unit parity (polynomial.rs:190-365)
// (adder: adder.hip; cipher: cipher.hip; carry-save multiplier: mul_engine.hip)
#include <hip/hip_runtime.h>

#include "dev_common.h"

namespace hm {

// The launch of the wave-per-value circuits (gates, borrow chain, min / max, select, lookup,
// shift, bit counts, array read / write): one wavefront per value, 4 per block, lds_per_wave words of dynamic LDS each.
template <class Args>
static int launch_wave_per_value(void (*kernel)(Args), const Args &g, uint64_t n,
                                 uint32_t lds_per_wave, void *stream) {
    const int wpb = 4;
    const uint64_t blocks = (n + wpb - 1) / wpb;
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(64 * wpb),
                       (size_t)lds_per_wave * 4 * wpb, (hipStream_t)stream, g);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------------------------
// Elementwise gates: one wavefront per value, bit by bit through LDS.
//   AND = a*b, XOR = a+b, OR = a+b+ab, NOT = a+1    (cipher.rs:58-90)
__global__ void __launch_bounds__(256) gate_kernel(GateArgs G) {
    extern __shared__ uint32_t lds[];
    const CircuitIO &IO = G.io;
    const WaveSlice ws = wave_slice(lds, G.lds_per_wave, IO.n);
    if (!ws.live) return;
    const int lane = lane_id();
    uint32_t *Ab = ws.lds + G.oA, *Bb = ws.lds + G.oB, *T = ws.lds + G.oT;
    BitReader ra(IO.a, ws.e, IO.status), rb(IO.b, ws.e, IO.status); // (NOT: rb is not read)
    BitWriter wo(IO.out, ws.e, IO.status);
    for (uint32_t i = 0; i < IO.nbits; ++i) {
        const int na = ra.load(i, IO.ab.b[i], Ab);
        int nb = 0;
        if (G.op == HM_OP_NOT) {
            if (lane == 0) Bb[0] = 1u; // the unit polynomial, CipheredBit::one (cipher.rs:49-51)
            nb = 1;
        } else {
            nb = rb.load(i, IO.bb.b[i], Bb);
        }
        wsync();
        int nt = 0, nout;
        if (G.op == HM_OP_AND) {
            nt = words_of(wave_mul<kQSmall, 8>(Ab, na, Bb, nb, nullptr, 0, T, &nout));
        } else if (G.op == HM_OP_OR) {
            // a + b + ab: first X = a ^ b into T's tail, then T = X ^ a*b
            uint32_t *Xs = T + (na + nb + 2);
            const int nx = words_of(wave_xor(Ab, na, Bb, nb, Xs));
            wsync();
            nt = words_of(wave_mul<kQSmall, 8>(Ab, na, Bb, nb, Xs, nx, T, &nout));
        } else { // XOR, NOT
            nt = words_of(wave_xor(Ab, na, Bb, nb, T));
        }
        wsync();
        wo.store(i, IO.ob.b[i], T, nt);
        wsync();
    }
}

int launch_gate(const GateArgs &g, void *stream) {
    return launch_wave_per_value(gate_kernel, g, g.io.n, g.lds_per_wave, stream);
}

// ---------------------------------------------------------------------------------------------
// Ripple-borrow chain: subtraction, orderings and equality (BorrowArgs).  One
// wavefront per value, bit by bit through LDS like the gates; the borrow lives in two ping-pong
// buffers because wave_mul's Dst may not alias its operands.

// X = A ^ B and P = X ^ 1 (x_i = a_i + b_i, p_i = x_i + 1); their word counts (0 = null).
__device__ __forceinline__ void xor_and_not(const uint32_t *A, int na, const uint32_t *B, int nb,
                                            uint32_t *X, uint32_t *P, int *nx, int *np) {
    const int n = max(max(na, nb), 1);
    int ldx = -1, ldp = -1;
    for (int w = lane_id(); w < n; w += kWave) {
        const uint32_t v = (w < na ? A[w] : 0u) ^ (w < nb ? B[w] : 0u);
        const uint32_t p = v ^ (w == 0 ? 1u : 0u);
        X[w] = v;
        P[w] = p;
        if (v) ldx = w * 32 + 31 - __builtin_clz(v);
        if (p) ldp = w * 32 + 31 - __builtin_clz(p);
    }
    *nx = words_of(wave_max_i32(ldx));
    *np = words_of(wave_max_i32(ldp));
}

// One step of the chain, w_{i+1} = g_i + p_i w_i into Wn (the caller then exchanges W and Wn);
// returns its words.  generate: g_i = a_i b_i + b_i (not a and b), formed in Gt; when top, the
// signed top bit, the operands' roles are exchanged: a_i b_i + a_i.  Otherwise g_i = 0 (the
// equality prefix).  Shared by borrow_kernel and minmax_kernel's phase 1.
__device__ __forceinline__ int borrow_step(const uint32_t *Ab, int na, const uint32_t *Bb, int nb,
                                           const uint32_t *P, int np, const uint32_t *W, int nw,
                                           uint32_t *Gt, uint32_t *Wn, bool generate, bool top) {
    int ng = 0, nout;
    if (generate) {
        ng = words_of(wave_mul<kQSmall, 8>(Ab, na, Bb, nb, top ? Ab : Bb, top ? na : nb, Gt,
                                           &nout));
        wsync();
    }
    nw = words_of(wave_mul<kQSmall, 8>(P, np, W, nw, Gt, ng, Wn, &nout));
    wsync();
    return nw;
}

__global__ void __launch_bounds__(256) borrow_kernel(BorrowArgs G) {
    extern __shared__ uint32_t lds[];
    const CircuitIO &IO = G.io;
    const BorrowLayout &Y = G.lay;
    const WaveSlice ws = wave_slice(lds, Y.lds_per_wave, IO.n);
    if (!ws.live) return;
    const int lane = lane_id();
    uint32_t *L = ws.lds;
    uint32_t *Ab = L + Y.oA, *Bb = L + Y.oB, *X = L + Y.oX, *P = L + Y.oP, *Gt = L + Y.oG;
    uint32_t *W = L + Y.oW, *Wn = W + Y.cw;
    BitReader ra(IO.a, ws.e, IO.status), rb(IO.b, ws.e, IO.status);
    BitWriter wo(IO.out, ws.e, IO.status);
    int nw = 0; // w_0 = 0
    if (G.mode == kBorrowEq) { // e_0 = 1
        if (lane == 0) W[0] = 1u;
        nw = 1;
    }
    for (uint32_t i = 0; i < IO.nbits; ++i) {
        const int na = ra.load(i, IO.ab.b[i], Ab);
        const int nb = rb.load(i, IO.bb.b[i], Bb);
        wsync();
        int nx, np;
        xor_and_not(Ab, na, Bb, nb, X, P, &nx, &np);
        wsync();
        if (G.mode == kBorrowSub) {
            wo.store(i, IO.ob.b[i], X, nx, W, nw);
            if (i + 1 == IO.nbits) break; // the last borrow is not needed
        }
        const bool top = G.sgn && i + 1 == IO.nbits;
        nw = borrow_step(Ab, na, Bb, nb, P, np, W, nw, Gt, Wn, G.mode != kBorrowEq, top);
        uint32_t *t = W;
        W = Wn, Wn = t;
    }
    if (G.mode == kBorrowSub) return;
    // Ciphered<bool>: bit 0 is the result (plus 1 for >=, <=, !=), bits 1..7 are null
    if (lane == 0) X[0] = 1u;
    wsync();
    wo.store(0, IO.ob.b[0], W, nw, X, G.flip ? 1 : 0);
    for (uint32_t k = 1; k < 8; ++k) wo.store(k, IO.ob.b[k], nullptr, 0);
}

int launch_borrow(const BorrowArgs &g, void *stream) {
    return launch_wave_per_value(borrow_kernel, g, g.io.n, g.lay.lds_per_wave, stream);
}

// ---------------------------------------------------------------------------------------------
// min / max (MinMaxArgs): the kBorrowLt chain above, then out_i = b_i + w_n x_i
// (min) or a_i + w_n x_i (max) with w_n kept in LDS.
__global__ void __launch_bounds__(256) minmax_kernel(MinMaxArgs G) {
    extern __shared__ uint32_t lds[];
    const CircuitIO &IO = G.io;
    const BorrowLayout &Y = G.lay;
    const WaveSlice ws = wave_slice(lds, Y.lds_per_wave, IO.n);
    if (!ws.live) return;
    uint32_t *L = ws.lds;
    uint32_t *Ab = L + Y.oA, *Bb = L + Y.oB, *X = L + Y.oX, *P = L + Y.oP, *Gt = L + Y.oG;
    uint32_t *W = L + Y.oW, *Wn = W + Y.cw;
    BitReader ra(IO.a, ws.e, IO.status), rb(IO.b, ws.e, IO.status);
    int nw = 0, nout; // w_0 = 0
    // phase 1: w_{i+1} = a_i b_i + b_i + p_i w_i through the top bit
    for (uint32_t i = 0; i < IO.nbits; ++i) {
        const int na = ra.load(i, IO.ab.b[i], Ab);
        const int nb = rb.load(i, IO.bb.b[i], Bb);
        wsync();
        int nx, np;
        xor_and_not(Ab, na, Bb, nb, X, P, &nx, &np);
        wsync();
        nw = borrow_step(Ab, na, Bb, nb, P, np, W, nw, Gt, Wn, true, G.sgn && i + 1 == IO.nbits);
        uint32_t *t = W;
        W = Wn, Wn = t;
    }
    // phase 2: W holds w_n; the operands from their first bit again; every product goes to Wn and
    // is stored from there
    ra = BitReader(IO.a, ws.e, IO.status), rb = BitReader(IO.b, ws.e, IO.status);
    BitWriter wo(IO.out, ws.e, IO.status);
    for (uint32_t i = 0; i < IO.nbits; ++i) {
        const int na = ra.load(i, IO.ab.b[i], Ab);
        const int nb = rb.load(i, IO.bb.b[i], Bb);
        wsync();
        const int nx = words_of(wave_xor(Ab, na, Bb, nb, X));
        wsync();
        const int nt = words_of(wave_mul<kQSmall, 8>(X, nx, W, nw, G.is_max ? Ab : Bb,
                                                     G.is_max ? na : nb, Wn, &nout));
        wsync();
        wo.store(i, IO.ob.b[i], Wn, nt);
        wsync();
    }
}

int launch_minmax(const MinMaxArgs &g, void *stream) {
    return launch_wave_per_value(minmax_kernel, g, g.io.n, g.lay.lds_per_wave, stream);
}

// Oblivious choice (SelectArgs): out_i = b_i + c x_i, c loaded once per value.
// x_i is the uniform operand of the product (it is short when c comes out of a comparison).
__global__ void __launch_bounds__(256) select_kernel(SelectArgs G) {
    extern __shared__ uint32_t lds[];
    const CircuitIO &IO = G.io;
    const WaveSlice ws = wave_slice(lds, G.lds_per_wave, IO.n);
    if (!ws.live) return;
    uint32_t *L = ws.lds;
    uint32_t *C = L + G.oC, *Ab = L + G.oA, *Bb = L + G.oB, *X = L + G.oX, *T = L + G.oT;
    // bit 0 of the Ciphered<bool> is the first polynomial of the value
    const int nc = BitReader(G.cond, ws.e, IO.status).load(0, G.cbound, C);
    BitReader ra(IO.a, ws.e, IO.status), rb(IO.b, ws.e, IO.status);
    BitWriter wo(IO.out, ws.e, IO.status);
    for (uint32_t i = 0; i < IO.nbits; ++i) {
        const int na = ra.load(i, IO.ab.b[i], Ab);
        const int nb = rb.load(i, IO.bb.b[i], Bb);
        wsync();
        const int nx = words_of(wave_xor(Ab, na, Bb, nb, X));
        wsync();
        int nout;
        const int nt = words_of(wave_mul<kQSmall, 8>(X, nx, C, nc, Bb, nb, T, &nout));
        wsync();
        wo.store(i, IO.ob.b[i], T, nt);
        wsync();
    }
}

int launch_select(const SelectArgs &g, void *stream) {
    return launch_wave_per_value(select_kernel, g, g.io.n, g.lds_per_wave, stream);
}

// ---------------------------------------------------------------------------------------------
// Table lookup (LookupArgs): out_j = sum_t MH[t] I_jt over the monomials of the
// index bits' low and high halves, I_jt = the XOR of the low monomials the table's coefficient
// mask names.  The masks are plaintext, so every skip below is a scalar branch.

// Dst[0..cI) = the XOR of the monomials M[s] (s: the set bits of m) at their word counts N[s];
// returns its words.
__device__ __forceinline__ int lookup_inner_sum(const LookupArgs &G, const uint32_t *L,
                                                const uint32_t *N, uint32_t m, uint32_t *Dst) {
    const int lane = lane_id();
    int ldeg = -1;
    for (uint32_t w0 = 0; w0 < G.cI; w0 += kWave) {
        const uint32_t w = w0 + lane;
        uint32_t v = 0u;
        for (uint32_t mm = m; mm; mm &= mm - 1) {
            const uint32_t s = (uint32_t)__builtin_ctz(mm);
            if (w < rfl(N[s])) v ^= L[G.off[s] + w];
        }
        if (w < G.cI) Dst[w] = v;
        if (v) ldeg = (int)w * 32 + 31 - __builtin_clz(v);
    }
    return words_of(wave_max_i32(ldeg));
}

__global__ void __launch_bounds__(256) lookup_kernel(LookupArgs G) {
    extern __shared__ uint32_t lds[];
    const WaveSlice ws = wave_slice(lds, G.lds_per_wave, G.n);
    if (!ws.live) return;
    const int lane = lane_id();
    uint32_t *L = ws.lds;
    uint32_t *N = L + G.oN, *I = L + G.oI, *P = L + G.oP, *Pn = P + G.cP;
    if (lane == 0) L[G.off[0]] = 1u, N[0] = 1u, N[16] = 1u; // ML[0] = MH[0] = 1
    // every index bit once, into its monomial's slot
    BitReader ra(G.a, ws.e, G.status);
    for (uint32_t i = 0; i < G.k; ++i) {
        const uint32_t id = i < G.kl ? 1u << i : 16u + (1u << (i - G.kl));
        const int na = ra.load(i, G.ab[i], L + G.off[id]);
        if (lane == 0) N[id] = (uint32_t)na;
    }
    wsync();
    // the other monomials by doubling: M[s | 1 << i] = a_i M[s], a_i the uniform operand
    int nout;
    for (uint32_t half = 0; half < 2; ++half) {
        const uint32_t h = 16 * half;
        for (uint32_t i = 1; i < (half ? G.kh : G.kl); ++i) {
            const uint32_t nb = rfl(N[h + (1u << i)]);
            for (uint32_t s = 1; s < (1u << i); ++s) {
                const uint32_t id = h + (1u << i) + s;
                if (!((G.need >> id) & 1u)) continue;
                const int nm = words_of(wave_mul<kQSmall, 8>(L + G.off[h + (1u << i)], (int)nb,
                                                             L + G.off[h + s], (int)rfl(N[h + s]),
                                                             nullptr, 0, L + G.off[id], &nout));
                if (lane == 0) N[id] = (uint32_t)nm;
                wsync();
            }
        }
    }
    BitWriter wo(G.out, ws.e, G.status);
    for (uint32_t j = 0; j < G.nob; ++j) {
        int np = 0; // words of the accumulator P
        for (uint32_t t = 0; t < (1u << G.kh); ++t) {
            const uint32_t at = t << G.kl;
            const uint32_t m = (G.coef[j][at >> 5] >> (at & 31)) & ((1u << (1u << G.kl)) - 1u);
            if (!m) continue;
            if (t == 0) { // MH[0] = 1: the inner sum itself
                np = lookup_inner_sum(G, L, N, m, P);
                wsync();
                continue;
            }
            const int nh = (int)rfl(N[16 + t]);
            if (!nh) continue;
            const int ni = lookup_inner_sum(G, L, N, m, I);
            wsync();
            if (!ni) continue;
            np = words_of(wave_mul<kQSmall, 8>(L + G.off[16 + t], nh, I, ni, P, np, Pn, &nout));
            wsync();
            uint32_t *x = P;
            P = Pn, Pn = x;
        }
        wo.store(j, G.ob[j], P, np);
        wsync();
    }
}

int launch_lookup(const LookupArgs &g, void *stream) {
    return launch_wave_per_value(lookup_kernel, g, g.n, g.lds_per_wave, stream);
}

// ---------------------------------------------------------------------------------------------
// Shift or rotate by an encrypted amount (ShiftArgs): L stages
// y_i = x_i + s_t (x_i + x_src(i)) over a value that stays in LDS, in place.  The stages run from
// the widest step down; a stage walks the bits away from its sources and a rotate saves the bits
// that wrap around first, so every source is read before its slot is rewritten.  Each product is
// formed in T (wave_mul's Dst may not alias U or Add) and copied to its slot; the last stage whose
// s_t is not null stores its products to the output instead and rewrites nothing.  s_t, the short
// operand, is the uniform one.  A null s_t is skipped: its stage is the identity.

// Dst[0..n) = Src[0..n)
__device__ __forceinline__ void wave_copy(const uint32_t *Src, int n, uint32_t *Dst) {
    for (int w = lane_id(); w < n; w += kWave) Dst[w] = Src[w];
}

__global__ void __launch_bounds__(256) shift_kernel(ShiftArgs G) {
    extern __shared__ uint32_t lds[];
    const CircuitIO &IO = G.io;
    const uint32_t nbits = IO.nbits;
    const WaveSlice ws = wave_slice(lds, G.lds_per_wave, IO.n);
    if (!ws.live) return;
    const int lane = lane_id();
    uint32_t *L = ws.lds;
    uint32_t *NB = L + G.oN, *NS = NB + nbits, *NV = NS + 8; // word counts: value, amount, saved
    uint32_t *X = L + G.oX, *T = L + G.oT, *Sv = L + G.oS, *B = L + G.oV;
    // every bit of a into its slot, the low L bits of the amount into theirs
    BitReader ra(IO.a, ws.e, IO.status), rs(IO.b, ws.e, IO.status);
    for (uint32_t i = 0; i < nbits; ++i) {
        const int na = ra.load(i, IO.ab.b[i], B + G.off[i]);
        if (lane == 0) NB[i] = (uint32_t)na;
    }
    int last = -1; // the last stage to run that is not the identity: the lowest such t
    for (uint32_t t = 0; t < G.L; ++t) {
        const int ns = rs.load(t, IO.bb.b[t], L + G.soff[t]);
        if (lane == 0) NS[t] = (uint32_t)ns;
        if (ns && last < 0) last = (int)t;
    }
    wsync();
    BitWriter wo(IO.out, ws.e, IO.status);
    if (last < 0) { // the amount is the null value: out = a
        for (uint32_t i = 0; i < nbits; ++i) wo.store(i, IO.ob.b[i], B + G.off[i], (int)rfl(NB[i]));
        return;
    }
    const bool rot = G.mode == kShiftRotl || G.mode == kShiftRotr;
    const bool down = G.mode == kShiftShl || G.mode == kShiftRotl; // src < i: from the top bit down
    for (int t = (int)G.L - 1; t >= last; --t) {
        const int ns = (int)rfl(NS[t]);
        if (!ns) continue;
        const uint32_t *S = L + G.soff[t];
        const uint32_t k = 1u << t, sv = G.sv[t];
        const bool fin = t == last; // nothing is rewritten: any order, nothing to save
        if (rot && !fin) { // the k bits that wrap: the top ones (ROTL) or the low ones (ROTR)
            for (uint32_t j = 0; j < k; ++j) {
                const uint32_t b = down ? nbits - k + j : j;
                const int nb = (int)rfl(NB[b]);
                wave_copy(B + G.off[b], nb, Sv + j * sv);
                if (lane == 0) NV[j] = (uint32_t)nb;
            }
            wsync();
        }
        for (uint32_t q = 0; q < nbits; ++q) {
            const uint32_t i = down && !fin ? nbits - 1 - q : q;
            uint32_t *xi = B + G.off[i];
            const int ni = (int)rfl(NB[i]);
            const int32_t src = (int32_t)rfl((uint32_t)shift_src(G.mode, nbits, k, i));
            const uint32_t *V = xi; // src null: y_i = x_i + s_t x_i
            int nv = ni;
            if (src >= 0) {
                const uint32_t *xs = B + G.off[src];
                int nsrc = (int)rfl(NB[src]);
                if (rot && !fin && (down ? i < k : i >= nbits - k)) { // src wrapped: saved
                    const uint32_t j = down ? i : (uint32_t)src;
                    xs = Sv + j * sv, nsrc = (int)rfl(NV[j]);
                }
                nv = words_of(wave_xor(xi, ni, xs, nsrc, X));
                wsync();
                V = X;
            }
            int nout;
            const int ny = words_of(wave_mul<kQSmall, 8>(S, ns, V, nv, xi, ni, T, &nout));
            wsync();
            if (fin) { // (i = q: in order)
                wo.store(i, IO.ob.b[i], T, ny);
            } else {
                wave_copy(T, ny, xi);
                if (lane == 0) NB[i] = (uint32_t)ny;
            }
            wsync();
        }
    }
}

int launch_shift(const ShiftArgs &g, void *stream) {
    return launch_wave_per_value(shift_kernel, g, g.io.n, g.lds_per_wave, stream);
}

// ---------------------------------------------------------------------------------------------
// Bit counts (BitCountArgs): count_ones / count_zeros as the elementary symmetric
// polynomials e_{2^k} of the literals, the leading / trailing runs as sums over the literals'
// prefix products.  The literal u_i, the short operand, is the uniform one of every product; a
// null factor skips its product on a scalar branch.

// The literal of the bit just loaded into U (nx words, 0: null, U[0] then undefined): the bit
// itself, or for the zeros ops the bit plus the unit polynomial.  Returns its words.
__device__ __forceinline__ int bitcount_literal(uint32_t *U, int nx, bool zeros) {
    if (!zeros) return nx;
    if (lane_id() == 0) U[0] = (nx ? U[0] : 0u) ^ 1u;
    wsync();
    return nx > 1 ? nx : (rfl(U[0]) ? 1 : 0); // (one word, of any degree 0..31, unless it is now null)
}

// count_ones / count_zeros: E_j <- E_j + u_i E_{j-1} over the slots E_1 .. E_J, j descending so
// that E_{j-1} is read before its own update; each product is formed in T (wave_mul's Dst may not
// alias Add) and copied to its slot.  E_1 <- E_1 + u_i is an XOR in place.  Past slot J (n a power
// of two) only the running product of all literals is still read: it goes on in D / Dn.
__global__ void __launch_bounds__(256) bitcount_kernel(BitCountArgs G) {
    extern __shared__ uint32_t lds[];
    const CircuitIO &IO = G.io;
    const uint32_t n = IO.nbits, J = G.J;
    const WaveSlice ws = wave_slice(lds, G.lds_per_wave, IO.n);
    if (!ws.live) return;
    const int lane = lane_id();
    uint32_t *L = ws.lds;
    uint32_t *NE = L + G.oN, *U = L + G.oU, *T = L + G.oT, *E = L + G.oE; // NE[j]: words of E_j
    uint32_t *D = L + G.oD, *Dn = D + G.cD;
    for (uint32_t j = lane; j <= J; j += kWave) NE[j] = 0u;
    wsync();
    BitReader ra(IO.a, ws.e, IO.status);
    int nd = 0, nout; // words of the running product in D
    for (uint32_t i = 1; i <= n; ++i) {
        const int nu = bitcount_literal(U, ra.load(i - 1, IO.ab.b[i - 1], U), G.zeros);
        wsync();
        if (G.diag && i > J) { // u_1 .. u_i from u_1 .. u_{i-1}: slot J's E_J^(J) at first
            const uint32_t *P = i == J + 1 ? E + G.off[J] : D;
            const int np = i == J + 1 ? (int)rfl(NE[J]) : nd;
            nd = 0;
            if (nu && np) {
                nd = words_of(wave_mul<kQSmall, 8>(U, nu, P, np, nullptr, 0, Dn, &nout));
                wsync();
            }
            uint32_t *x = D;
            D = Dn, Dn = x;
        }
        if (!nu) continue; // a null literal changes no E_j
        for (uint32_t j = min(i, J); j >= 2; --j) {
            if (!bitcount_needed(n, i, j)) continue;
            const int np = (int)rfl(NE[j - 1]);
            if (!np) continue;
            uint32_t *Ej = E + G.off[j];
            const int ne = words_of(wave_mul<kQSmall, 8>(U, nu, E + G.off[j - 1], np, Ej,
                                                         (int)rfl(NE[j]), T, &nout));
            wsync();
            wave_copy(T, ne, Ej);
            if (lane == 0) NE[j] = (uint32_t)ne;
            wsync();
        }
        uint32_t *E1 = E + G.off[1]; // E_1 <- E_1 + u_i E_0 (J >= 1)
        const int ne = words_of(wave_xor(E1, (int)rfl(NE[1]), U, nu, E1));
        if (lane == 0) NE[1] = (uint32_t)ne;
        wsync();
    }
    BitWriter wo(IO.out, ws.e, IO.status);
    for (uint32_t k = 0; k < kBitCountOut; ++k) {
        const uint32_t t = 1u << k;
        if (t <= J) wo.store(k, IO.ob.b[k], E + G.off[t], (int)rfl(NE[t]));
        else if (G.diag && t == n) wo.store(k, IO.ob.b[k], D, nd);
        else wo.store(k, IO.ob.b[k], nullptr, 0);
    }
}

int launch_bitcount(const BitCountArgs &g, void *stream) {
    return launch_wave_per_value(bitcount_kernel, g, g.io.n, g.lds_per_wave, stream);
}

// leading / trailing zeros / ones: the literals in the run's order, v_j = bit n - j (leading) or
// j - 1 (trailing); t_j = t_{j-1} v_j in D / Dn, XORed into the accumulator of every output bit k
// with 2^k | j.  Once t_j is null the chain stays null: the remaining bits are only loaded (their
// degree words are validated like the others).
__global__ void __launch_bounds__(256) bitrun_kernel(BitCountArgs G) {
    extern __shared__ uint32_t lds[];
    const CircuitIO &IO = G.io;
    const uint32_t n = IO.nbits;
    const WaveSlice ws = wave_slice(lds, G.lds_per_wave, IO.n);
    if (!ws.live) return;
    const int lane = lane_id();
    uint32_t *L = ws.lds;
    uint32_t *NA = L + G.oN, *U = L + G.oU, *A = L + G.oE; // NA[k]: words of accumulator k
    uint32_t *D = L + G.oD, *Dn = D + G.cD;
    if (lane < (int)kBitCountOut) NA[lane] = 0u;
    wsync();
    BitReader ra(IO.a, ws.e, IO.status);
    if (G.leading) ra.off = G.a_limbs; // from the top bit down
    int nt = 0, nout; // words of t_j in D
    for (uint32_t j = 1; j <= n; ++j) {
        const uint32_t i = G.leading ? n - j : j - 1;
        const int nx = G.leading ? ra.load_down(i, IO.ab.b[i], U) : ra.load(i, IO.ab.b[i], U);
        if (j > 1 && !nt) continue;
        const int nu = bitcount_literal(U, nx, G.zeros);
        wsync();
        const int np = nt;
        nt = 0;
        if (j == 1) { // t_1 = v_1
            wave_copy(U, nu, Dn);
            nt = nu;
        } else if (nu) {
            nt = words_of(wave_mul<kQSmall, 8>(U, nu, D, np, nullptr, 0, Dn, &nout));
        }
        wsync();
        uint32_t *x = D;
        D = Dn, Dn = x;
        if (!nt) continue;
        for (uint32_t k = 0; k < G.K && !(j & ((1u << k) - 1u)); ++k) {
            uint32_t *Ak = A + G.off[k];
            const int na = words_of(wave_xor(Ak, (int)rfl(NA[k]), D, nt, Ak));
            if (lane == 0) NA[k] = (uint32_t)na;
        }
        wsync();
    }
    BitWriter wo(IO.out, ws.e, IO.status);
    for (uint32_t k = 0; k < kBitCountOut; ++k) {
        if (k < G.K) wo.store(k, IO.ob.b[k], A + G.off[k], (int)rfl(NA[k]));
        else wo.store(k, IO.ob.b[k], nullptr, 0);
    }
}

int launch_bitrun(const BitCountArgs &g, void *stream) {
    return launch_wave_per_value(bitrun_kernel, g, g.io.n, g.lds_per_wave, stream);
}

// ---------------------------------------------------------------------------------------------
// Oblivious array read and write by an encrypted index (ArrayReadArgs / ArrayWriteArgs, DESIGN.md
// s4.4f).  One wavefront per index value; element v of its array is value e count + v of the array
// batch (64-bit arithmetic), or value v of a shared table.  The short operand of every product is
// the uniform one; a null factor skips its product on a scalar branch.

// read: one output bit at a time, the elements in order through a stack of one waiting left child
// per tree level.  A level-t node (an even element's bit is loaded straight into slot 0) parks in
// slot t when bit t of v is 0, or is joined with the one parked there, y = L + s_t (L + R): L + R
// into X, the product into the ping-pong buffer the node is not in.  Under the last element a
// node with nothing parked beside it has the null polynomial for its right sibling, y = L + s_t L,
// and goes on rising: the walk ends at the root, level k.  A skipped product leaves the node
// where its L is (a slot; it is copied only when it parks).
__global__ void __launch_bounds__(256) array_read_kernel(ArrayReadArgs G) {
    extern __shared__ uint32_t lds[];
    const CircuitIO &IO = G.io;
    const uint32_t k = G.k, count = G.count;
    const WaveSlice ws = wave_slice(lds, G.lds_per_wave, IO.n);
    if (!ws.live) return;
    const int lane = lane_id();
    uint32_t *L = ws.lds;
    uint32_t *NS = L + G.oN, *NK = NS + kArrayMaxIndex; // word counts: index bits, slots
    uint32_t *Ld = L + G.oL, *X = L + G.oX, *P0 = L + G.oP, *P1 = P0 + G.cP;
    BitReader rs(IO.b, ws.e, IO.status);
    for (uint32_t t = 0; t < k; ++t) {
        const int ns = rs.load(t, IO.bb.b[t], L + G.soff[t]);
        if (lane == 0) NS[t] = (uint32_t)ns;
    }
    wsync();
    const uint64_t first = G.shared ? 0ull : ws.e * count;
    BitWriter wo(IO.out, ws.e, IO.status);
    uint32_t aoff = 0; // limbs of an element before bit j
    for (uint32_t j = 0; j < IO.nbits; ++j) {
        const uint32_t bj = IO.ab.b[j];
        for (uint32_t v = 0; v < count; ++v) {
            BitReader ra(IO.a, first + v, IO.status);
            ra.off = aoff;
            uint32_t *node = v & 1u ? Ld : L + G.slot[0];
            int nn = ra.load(j, bj, node);
            wsync();
            uint32_t t = 0;
            for (; t < k; ++t) {
                uint32_t *Sl = L + G.slot[t];
                const uint32_t *V, *Add; // the product's long factor, and what it is added to
                int nv, nadd;
                if ((v >> t) & 1u) { // joins the left child parked at this level
                    nadd = (int)rfl(NK[t]);
                    nv = words_of(wave_xor(Sl, nadd, node, nn, X));
                    wsync();
                    V = X, Add = Sl;
                } else if (v + 1 == count) { // the right sibling is past the array: null
                    V = Add = node, nv = nadd = nn;
                } else { // waits for its right sibling
                    if (node != Sl) wave_copy(node, nn, Sl);
                    if (lane == 0) NK[t] = (uint32_t)nn;
                    wsync();
                    break;
                }
                const int ns = (int)rfl(NS[t]);
                if (ns && nv) {
                    uint32_t *Dst = node == P0 ? P1 : P0;
                    int nout;
                    nn = words_of(wave_mul<kQSmall, 8>(L + G.soff[t], ns, V, nv, Add, nadd, Dst,
                                                       &nout));
                    wsync();
                    node = Dst;
                } else {
                    node = const_cast<uint32_t *>(Add), nn = nadd;
                }
            }
            if (t == k) { // (the last element only) the root
                wo.store(j, IO.ob.b[j], node, nn);
                wsync();
            }
        }
        aoff += cap_of(bj);
    }
}

int launch_array_read(const ArrayReadArgs &g, void *stream) {
    return launch_wave_per_value(array_read_kernel, g, g.io.n, g.lds_per_wave, stream);
}

// write: the suffix products Q_t = prod_{i >= t} lit_i(v) in k slots, Q_0 the indicator of v.
// From v - 1 to v the bits up to v's lowest set bit change: those levels are formed again from the
// top one down (level k - 1 is the literal itself), the literal s_t + 1 of a 0 bit as
// bitcount_literal forms it from a copy of s_t.  Then out_j = T_j + Q_0 (x_j + T_j) for every bit
// of element v, x's bits held in LDS since the start; a null Q_0 or x_j + T_j stores T_j itself.
__global__ void __launch_bounds__(256) array_write_kernel(ArrayWriteArgs G) {
    extern __shared__ uint32_t lds[];
    const CircuitIO &IO = G.io;
    const uint32_t k = G.k, count = G.count;
    const WaveSlice ws = wave_slice(lds, G.lds_per_wave, IO.n);
    if (!ws.live) return;
    const int lane = lane_id();
    uint32_t *L = ws.lds;
    // word counts: index bits, suffix products, x's bits
    uint32_t *NS = L + G.oN, *NQ = NS + kArrayMaxIndex, *NX = NQ + kArrayMaxIndex;
    uint32_t *U = L + G.oU, *T = L + G.oT, *X = L + G.oX, *O = L + G.oO, *XV = L + G.oV;
    BitReader rs(G.idx, ws.e, IO.status), rx(IO.b, ws.e, IO.status);
    for (uint32_t t = 0; t < k; ++t) {
        const int ns = rs.load(t, G.sb[t], L + G.soff[t]);
        if (lane == 0) NS[t] = (uint32_t)ns;
    }
    uint32_t xo = 0;
    for (uint32_t j = 0; j < IO.nbits; ++j) {
        const int nx = rx.load(j, IO.bb.b[j], XV + xo);
        if (lane == 0) NX[j] = (uint32_t)nx;
        xo += 2 * cap_of(IO.bb.b[j]);
    }
    wsync();
    for (uint32_t v = 0; v < count; ++v) {
        for (int t = v ? __builtin_ctz(v) : (int)k - 1; t >= 0; --t) {
            const int ns = (int)rfl(NS[t]);
            wave_copy(L + G.soff[t], ns, U);
            wsync();
            const int nu = bitcount_literal(U, ns, !((v >> t) & 1u));
            wsync();
            uint32_t *Q = L + G.qoff[t];
            int nq = 0, nout;
            if (t == (int)k - 1) {
                wave_copy(U, nu, Q);
                nq = nu;
            } else {
                const int np = (int)rfl(NQ[t + 1]);
                if (nu && np)
                    nq = words_of(wave_mul<kQSmall, 8>(U, nu, L + G.qoff[t + 1], np, nullptr, 0, Q,
                                                       &nout));
            }
            if (lane == 0) NQ[t] = (uint32_t)nq;
            wsync();
        }
        const uint32_t *Q0 = L + G.qoff[0];
        const int nind = (int)rfl(NQ[0]);
        const uint64_t el = ws.e * count + v;
        BitReader ra(IO.a, el, IO.status);
        BitWriter wo(IO.out, el, IO.status);
        xo = 0;
        for (uint32_t j = 0; j < IO.nbits; ++j) {
            const int nt = ra.load(j, IO.ab.b[j], T);
            wsync();
            int nx = 0, nout;
            if (nind) {
                nx = words_of(wave_xor(XV + xo, (int)rfl(NX[j]), T, nt, X));
                wsync();
            }
            if (nx) {
                const int no = words_of(wave_mul<kQSmall, 8>(X, nx, Q0, nind, T, nt, O, &nout));
                wsync();
                wo.store(j, IO.ob.b[j], O, no);
            } else {
                wo.store(j, IO.ob.b[j], T, nt);
            }
            wsync();
            xo += 2 * cap_of(IO.bb.b[j]);
        }
    }
}

int launch_array_write(const ArrayWriteArgs &g, void *stream) {
    return launch_wave_per_value(array_write_kernel, g, g.io.n, g.lds_per_wave, stream);
}

// ---------------------------------------------------------------------------------------------
// Single-polynomial primitives (unit parity for polynomial.rs).  Inputs must satisfy the layout
// invariant (bits above the degree are zero); word views of the u64 limbs are used directly.
__device__ __forceinline__ int poly_words(const uint64_t *limbs, uint32_t deg) {
    if (deg == 0 && (rfl((uint32_t)limbs[0]) & 1u) == 0) return 0;
    return nwords((int)deg);
}

__device__ __forceinline__ void zero_tail_and_degree(uint64_t *out, uint32_t ocap, int deg, uint32_t *odeg,
                                     int written_words) {
    uint32_t *w = (uint32_t *)out;
    for (int k = written_words + lane_id(); k < (int)(2 * ocap); k += kWave) w[k] = 0u;
    if (lane_id() == 0) *odeg = (uint32_t)max(deg, 0);
}

__global__ void __launch_bounds__(256) poly_add_kernel(PolyArgs P) {
    const uint64_t e = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (e >= P.n) return;
    const uint64_t *a = P.a + e * P.acap, *b = P.b + e * P.bcap;
    uint64_t *o = P.out + e * P.ocap;
    const int na = poly_words(a, rfl(P.adeg[e])), nb = poly_words(b, rfl(P.bdeg[e]));
    const int deg = wave_xor((const uint32_t *)a, na, (const uint32_t *)b, nb, (uint32_t *)o);
    zero_tail_and_degree(o, P.ocap, deg, P.odeg + e, max(na, nb));
}

__global__ void __launch_bounds__(256) poly_mul_kernel(PolyArgs P) {
    const uint64_t e = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (e >= P.n) return;
    const uint64_t *a = P.a + e * P.acap, *b = P.b + e * P.bcap;
    uint64_t *o = P.out + e * P.ocap;
    const int na = poly_words(a, rfl(P.adeg[e])), nb = poly_words(b, rfl(P.bdeg[e]));
    int nout;
    int deg;
    if (na <= nb)
        deg = wave_mul<kQBig, 8>((const uint32_t *)a, na, (const uint32_t *)b, nb, nullptr, 0,
                              (uint32_t *)o, &nout);
    else
        deg = wave_mul<kQBig, 8>((const uint32_t *)b, nb, (const uint32_t *)a, na, nullptr, 0,
                              (uint32_t *)o, &nout);
    wsync();
    zero_tail_and_degree(o, P.ocap, deg, P.odeg + e, nout);
}

// Remainder by one divisor S (polynomial.rs:316-365) as a table remainder:
// C mod S = XOR over the set bits k of C of (X^k mod S), so remainder bit j is the parity of
// C AND Z_j, where bit k of the row Z_j is bit j of X^k mod S.  The same linear functional as the
// decrypt table (row j = 0), for every bit of the remainder; identical to the long division's
// remainder, which is unique.  For k < deg S, X^k mod S = X^k: those columns are the identity, so
// the host table (zt, built in hm_poly_rem_batch) holds rows j < deg S over the limbs from
// l0 = deg S / 64 on only (tcols = acap - l0 limbs per row), and remainder word w < l0 starts as
// C's limb w.  zt = null: the divisor is above every dividend's degree, the remainder is C.
// One wave per polynomial: lanes hold C's first 512 limbs in registers (limbs past them are
// re-read from memory for every row, so any dividend size is accepted, as polynomial.rs:316-365
// accepts it), one ballot per remainder bit gives its parity.
constexpr int kRemLimbsPerLane = 8; // limbs held in registers: 512 (32768 coefficients)

__global__ void __launch_bounds__(256) poly_rem_kernel(PolyArgs P, RemTable T) {
    const uint64_t e = (uint64_t)blockIdx.x * (blockDim.x >> 6) + rfl(threadIdx.x >> 6);
    if (e >= P.n) return;
    const int lane = lane_id();
    const uint64_t *a = P.a + e * P.acap;
    uint64_t *r = P.out + e * P.ocap;
    const uint32_t adeg = rfl(P.adeg[e]);
    const int na = poly_words(a, adeg) ? (int)(adeg / 64 + 1) : 0;
    if (!T.zt) { // deg S above every dividend: C mod S = C
        for (int k = lane; k < (int)P.ocap; k += kWave) r[k] = k < na ? a[k] : 0ull;
        if (lane == 0) P.odeg[e] = na ? adeg : 0u;
        return;
    }
    const int l0 = (int)T.l0;
    uint64_t c[kRemLimbsPerLane];
#pragma unroll
    for (int t = 0; t < kRemLimbsPerLane; ++t) {
        const int k = lane + kWave * t;
        c[t] = k >= l0 && k < na ? a[k] : 0ull;
    }
    // remainder bits, 64 at a time: lane j%64 keeps word j/64's bit j%64; degree < deg S
    const int rl = min((int)(T.rows + 63) / 64, (int)P.ocap);
    int top = -1;
    for (int w = 0; w < rl; ++w) {
        uint64_t word = w < l0 && w < na ? a[w] : 0ull; // the identity columns (wave-uniform)
        for (int jb = 0; jb < 64 && 64 * w + jb < (int)T.rows; ++jb) {
            const uint64_t *z = T.zt + (size_t)(64 * w + jb) * T.tcols - l0; // z[k], k >= l0
            uint32_t par = 0u;
#pragma unroll
            for (int t = 0; t < kRemLimbsPerLane; ++t) {
                const int k = lane + kWave * t;
                if (k >= l0 && k < na) par ^= (uint32_t)__popcll(c[t] & z[k]);
            }
            for (int k = max(kWave * kRemLimbsPerLane, l0) + lane; k < na; k += kWave)
                par ^= (uint32_t)__popcll(a[k] & z[k]);
            const uint64_t m = __ballot(par & 1u);
            word ^= (uint64_t)(__popcll(m) & 1) << jb;
        }
        if (lane == 0) r[w] = word; // word is wave-uniform
        if (word) top = 64 * w + 63 - __builtin_clzll(word);
    }
    for (int k = rl + lane; k < (int)P.ocap; k += kWave) r[k] = 0ull;
    if (lane == 0) P.odeg[e] = (uint32_t)max(top, 0);
}

int launch_poly_add(const PolyArgs &P, void *stream) {
    if (!P.n) return 0;
    hipLaunchKernelGGL(poly_add_kernel, dim3((unsigned)((P.n + 3) / 4)), dim3(256), 0,
                       (hipStream_t)stream, P);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int launch_poly_mul(const PolyArgs &P, void *stream) {
    if (!P.n) return 0;
    hipLaunchKernelGGL(poly_mul_kernel, dim3((unsigned)((P.n + 3) / 4)), dim3(256), 0,
                       (hipStream_t)stream, P);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int launch_poly_rem(const PolyArgs &P, const RemTable &T, void *stream) {
    if (!P.n) return 0;
    hipLaunchKernelGGL(poly_rem_kernel, dim3((unsigned)((P.n + 3) / 4)), dim3(256), 0,
                       (hipStream_t)stream, P, T);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace hm
