// capi.cpp — host side of the C ABI declared in include/homomorph_gpu.h.
//
// Owns the per-device context (keys, derived decrypt table, workspace, stream), validates every
// call the way the reference's safe wrappers do (Context::validate_operation, src/context.rs:
// 310-323; Parameters::new asserts, :87-94) and launches the kernels.  The static degree bounds
// and the plans come from host-only headers: the adder's from add_host.h (plan_add), the
// wave-per-value circuits' from circuit_host.h (plan_gate, plan_borrow, plan_select),
// lookup_host.h (plan_lookup), shift_host.h (plan_shift), bitcount_host.h (plan_bitcount) and
// array_host.h (plan_array_read, plan_array_write); the multiplier's from mul_plan.h
// (mul_result_bounds, mul_cost_model; its plans are built, cached and run by mul_host.cpp).
// Never throws across the ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <new>
#include <vector>

#include <sys/random.h>

#include "add_host.h"
#include "array_host.h"
#include "bitcount_host.h"
#include "circuit_host.h"
#include "ctx.h"
#include "lookup_host.h"
#include "mul_plan.h"
#include "shift_host.h"

using namespace hm;

namespace {

uint64_t splitmix64(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

size_t degree_of(const uint64_t *c, size_t n) {
    for (size_t k = n; k-- > 0;)
        if (c[k]) return 64 * k + 63 - (size_t)__builtin_clzll(c[k]);
    return 0;
}

// getrandom(2) into buf (the reference's getrandom::fill, src/polynomial.rs:87, cipher.rs:95)
bool os_random(void *buf, size_t n) {
    uint8_t *p = (uint8_t *)buf;
    while (n) {
        const ssize_t r = getrandom(p, n, 0);
        if (r < 0) return false;
        p += r, n -= (size_t)r;
    }
    return true;
}

// Polynomial::random(degree) (src/polynomial.rs:73-96): limbs from getrandom, or from the
// context's SplitMix64 stream once hm_ctx_seed_rng fixed it (test contract); top bit forced,
// bits above it cleared (:89-90).
bool random_poly(hm_ctx *c, size_t degree, std::vector<uint64_t> &v) {
    v.assign(degree / 64 + 1, 0);
    if (c->seeded) {
        for (auto &w : v) w = splitmix64(c->rng);
    } else if (!os_random(v.data(), v.size() * 8)) {
        return false;
    }
    v.back() &= (1ull << (degree % 64)) - 1;
    v.back() |= 1ull << (degree % 64);
    return true;
}

void wipe(void *p, size_t n) {
    volatile uint8_t *q = (volatile uint8_t *)p;
    for (size_t i = 0; i < n; ++i) q[i] = 0;
}

// Host carry-less product for key generation only (setup path, runs once per key).
std::vector<uint64_t> clmul_host(const std::vector<uint64_t> &a, const std::vector<uint64_t> &b) {
    std::vector<uint64_t> r(a.size() + b.size(), 0);
    for (size_t i = 0; i < a.size(); ++i) {
        for (size_t j = 0; j < b.size(); ++j) {
            uint64_t lo = 0, hi = 0, x = a[i], y = b[j];
            while (x) {
                unsigned k = (unsigned)__builtin_ctzll(x);
                lo ^= y << k;
                if (k) hi ^= y >> (64 - k);
                x &= x - 1;
            }
            r[i + j] ^= lo;
            r[i + j + 1] ^= hi;
        }
    }
    return r;
}

// 64x64 bit-matrix transpose in place: bit j of m[u] moves to bit u of m[j] (block swaps of
// halving size; the remainder table's columns are built as rows of X^k mod S)
void transpose64(uint64_t m[64]) {
    uint64_t mask = 0x00000000FFFFFFFFull;
    for (unsigned s = 32; s; s >>= 1, mask ^= mask << s)
        for (unsigned u = 0; u < 64; u = ((u | s) + 1) & ~s) {
            const uint64_t x = ((m[u] >> s) ^ m[u | s]) & mask;
            m[u] ^= x << s;
            m[u | s] ^= x;
        }
}

uint16_t min_d_over_delta(hm_op op) { // src/impls/numbers.rs:27-50
    switch (op) {
    case HM_OP_AND: case HM_OP_OR: return 2;
    case HM_OP_XOR: case HM_OP_NOT: return 1;
    case HM_OP_ADD: return 21;
    case HM_OP_MUL: case HM_OP_MUL_SIGNED: return 64;
    case HM_OP_SELECT: return 5; // 2m + 1 for c x_i of fresh bits, m = 2
    default: break; // HM_OP_SUB .. HM_OP_GE, HM_OP_MIN, HM_OP_MAX, HM_OP_LOOKUP, the shifts and
                    // the bit counts depend on the width: borrow_min_d_over_delta
    }
    return 0xFFFF;
}

bool is_borrow_op(hm_op op) { return op >= HM_OP_SUB && op <= HM_OP_GE; }
bool is_compare_op(hm_op op) { return op >= HM_OP_EQ && op <= HM_OP_GE; }
bool is_ordering_op(hm_op op) { return op >= HM_OP_LT && op <= HM_OP_GE; }
bool is_minmax_op(hm_op op) { return op == HM_OP_MIN || op == HM_OP_MAX; }
using shift_plan::is_shift_op;
using bitcount_plan::is_bitcount_op;
using array_plan::is_array_op;
bool needs_width(hm_op op) {
    return is_borrow_op(op) || is_minmax_op(op) || op == HM_OP_LOOKUP || is_shift_op(op) ||
           is_bitcount_op(op) || is_array_op(op);
}

// 2m + 1 with m the borrow circuit's degree in fresh input bits: nbits + 1 for the orderings
// (the borrow out of the top bit), nbits for subtraction and equality, nbits + 2 for min / max
// (that borrow times x_i).  A table lookup is multilinear in its nbits index bits: m = nbits.
// A shift or rotate of an nbits-bit value is log2 nbits selects deep: m = log2 nbits + 1 (the
// caller has checked the width, shift_plan::stages).  A bit count's m is bitcount_plan::degree_of:
// the top symmetric polynomial 2^floor(log2 nbits) of a count, the whole prefix nbits of a run.
// An array read or write by nbits index bits multiplies an indicator of nbits literals by one
// more bit: m = nbits + 1 (array_plan::degree_of).
// A fresh bit's noise has degree delta + 1 <= 2 delta, so d >= (2m + 1) delta gives
// m (delta + 1) < d.
uint16_t borrow_min_d_over_delta(hm_op op, uint32_t nbits) {
    if (is_shift_op(op)) return (uint16_t)(2 * shift_plan::stages(nbits) + 3);
    if (is_bitcount_op(op)) return (uint16_t)(2 * bitcount_plan::degree_of(op, nbits) + 1);
    if (is_array_op(op)) return (uint16_t)(2 * array_plan::degree_of(nbits) + 1);
    const uint32_t m = nbits + (is_ordering_op(op) ? 1u : is_minmax_op(op) ? 2u : 0u);
    return (uint16_t)(2 * m + 1);
}

// the bound of an output must cover the computed bound, bit by bit
bool covers(const hm_batch *out, const std::vector<uint32_t> &need) {
    for (uint32_t i = 0; i < out->nbits; ++i)
        if (out->bound[i] < need[i]) return false;
    return true;
}

// The operand check of the batch entries: check_batch on each operand in the order given (a null
// one is its HM_ERR_INVALID_ARGUMENT, a bound beyond 2^30 its HM_ERR_UNSUPPORTED), then each has
// the width asked of it (0: the operation's width, the first such operand's) and as many values
// as the first.  Which status a call with several faults returns depends on the order of the
// operands, on whether the entry tests every pointer first, and on where validate_operation sits
// relative to this check: each entry keeps its own.
struct Operand {
    const hm_batch *x;
    uint32_t nbits;
};
hm_status check_operands(std::initializer_list<Operand> ops) {
    for (const Operand &o : ops)
        if (hm_status st = check_batch(o.x); st) return st;
    uint32_t width = 0;
    for (const Operand &o : ops)
        if (!o.nbits && !width) width = o.x->nbits;
    for (const Operand &o : ops)
        if (o.x->nbits != (o.nbits ? o.nbits : width) || o.x->n != ops.begin()->x->n)
            return HM_ERR_INVALID_ARGUMENT;
    return HM_OK;
}

// The operands, counts, bounds and status word of a wave-per-value circuit (b null: a unary gate)
void fill_io(CircuitIO &io, hm_ctx *c, const hm_batch *a, const hm_batch *b, const hm_batch *out) {
    io.a = batch_arg(a), io.out = batch_arg(out);
    io.n = a->n, io.nbits = a->nbits;
    io.status = c->d_status;
    fill_bounds(io.ab, a), fill_bounds(io.ob, out);
    if (b) io.b = batch_arg(b), fill_bounds(io.bb, b);
}

// Launches a planned wave-per-value circuit over checked batches
template <class Args>
hm_status run_circuit(hm_ctx *c, const Args &G, int (*launch)(const Args &, void *)) {
    DeviceGuard g(c->device);
    return launch(G, c->stream) ? hip_fail(c, hipGetLastError()) : HM_OK;
}

// Uploads the public key rows, and (when it fits an LDS budget) the encryption nibble table:
// for every group g of four rows, the 16 XOR combinations T[g][n] = XOR_{k: bit k of n} T_{4g+k}
// (rows past tau are zero).  Built once per key, so encryption blocks only copy it into LDS.
// Layout [g][limb pair p][n][2 limbs] (a missing last limb is zero): the 16 entries' copies of
// one limb pair are 16 B apart, so a wave's per-lane lookups (any n per lane) of one pair are a
// conflict-free ds_read_b128 -- 16 distinct addresses cover the 64 LDS banks exactly once.
hm_status upload_pk(hm_ctx *c) {
    DeviceGuard g(c->device);
    HM_HIP(c, hipStreamSynchronize(c->stream));
    retire(c, c->d_pk, 0, false), c->d_pk = nullptr;
    retire(c, c->d_pk_tab, 0, false), c->d_pk_tab = nullptr;
    retire(c, c->d_pk_tab1, 0, false), c->d_pk_tab1 = nullptr;
    HM_HIP(c, hipMalloc(&c->d_pk, c->pk.size() * 8));
    HM_HIP(c, hipMemcpy(c->d_pk, c->pk.data(), c->pk.size() * 8, hipMemcpyHostToDevice));
    const uint32_t G = (c->pk_tau + 3) / 4, PC = c->pk_cap, NP = (PC + 1) / 2;
    const size_t words = (size_t)G * NP * 16 * 2;
    if (words * 8 <= kEncTableBytes) {
        std::vector<uint64_t> tab(words, 0);
        for (uint32_t grp = 0; grp < G; ++grp)
            for (uint32_t n = 0; n < 16; ++n)
                for (uint32_t k = 0; k < 4; ++k)
                    if (((n >> k) & 1u) && 4 * grp + k < c->pk_tau)
                        for (uint32_t l = 0; l < PC; ++l)
                            tab[(((size_t)grp * NP + l / 2) * 16 + n) * 2 + l % 2] ^=
                                c->pk[(size_t)(4 * grp + k) * PC + l];
        HM_HIP(c, hipMalloc(&c->d_pk_tab, words * 8));
        HM_HIP(c, hipMemcpy(c->d_pk_tab, tab.data(), words * 8, hipMemcpyHostToDevice));
        if (c->pk_top1) {
            // the same table without the one-bit top limb (EncArgs::top1): pairs of limbs
            // 0 .. PC-2 only, NP1 = (PC - 1 + 1) / 2 pairs per group -- a third smaller at PC = 5
            const uint32_t NP1 = PC / 2;
            std::vector<uint64_t> tab1((size_t)G * NP1 * 32, 0);
            for (uint32_t grp = 0; grp < G; ++grp)
                for (uint32_t p = 0; p < NP1; ++p)
                    for (uint32_t k = 0; k < 32; ++k)
                        if (2 * p + k % 2 < PC - 1)
                            tab1[((size_t)grp * NP1 + p) * 32 + k] = tab[((size_t)grp * NP + p) * 32 + k];
            HM_HIP(c, hipMalloc(&c->d_pk_tab1, tab1.size() * 8));
            HM_HIP(c, hipMemcpy(c->d_pk_tab1, tab1.data(), tab1.size() * 8, hipMemcpyHostToDevice));
        }
    }
    return HM_OK;
}

void drop_secret(hm_ctx *c) {
    // SecretKey's Drop zeroizes (src/context.rs:197-206): zero host copy and device tables
    if (!c->sk.empty()) {
        volatile uint64_t *p = c->sk.data();
        for (size_t i = 0; i < c->sk.size(); ++i) p[i] = 0;
    }
    c->sk.clear();
    if (c->d_z) {
        (void)hipStreamSynchronize(c->stream);
        retire(c, c->d_z, (size_t)c->z_limbs * 8, true);
        c->d_z = nullptr;
        c->z_limbs = 0;
    }
    c->has_sk = false;
}

// z_k = (X^k mod S)(0) for k < 64*limbs: the decrypt functional (DESIGN.md "Decryption").
hm_status ensure_ztable(hm_ctx *c, uint32_t max_bound) {
    const uint32_t need = max_bound / 64 + 1;
    if (c->d_z && c->z_limbs >= need) return HM_OK;
    const size_t ds = degree_of(c->sk.data(), c->sk.size());
    bool nonzero = false;
    for (auto w : c->sk) nonzero |= (w != 0);
    if (!nonzero) return HM_ERR_DIVIDE_BY_ZERO;
    if (ds == 0) return HM_ERR_DIVISOR_IS_ONE;
    const size_t sl = ds / 64 + 1;
    std::vector<uint64_t> r(sl, 0), z(need, 0);
    r[0] = 1; // X^0
    for (size_t k = 0; k < (size_t)need * 64; ++k) {
        if (r[0] & 1) z[k / 64] |= 1ull << (k % 64);
        // r = X*r mod S  (r has degree < ds)
        uint64_t carry = 0;
        for (size_t w = 0; w < sl; ++w) {
            uint64_t nc = r[w] >> 63;
            r[w] = (r[w] << 1) | carry;
            carry = nc;
        }
        if ((r[ds / 64] >> (ds % 64)) & 1)
            for (size_t w = 0; w < sl; ++w) r[w] ^= c->sk[w];
    }
    DeviceGuard g(c->device);
    size_t have = (size_t)c->z_limbs * 8;
    HM_HIP(c, grow(c, c->d_z, have, (size_t)need * 8, true));
    HM_HIP(c, hipMemcpy(c->d_z, z.data(), (size_t)need * 8, hipMemcpyHostToDevice));
    wipe(z.data(), z.size() * 8);
    wipe(r.data(), r.size() * 8);
    c->z_limbs = need;
    return HM_OK;
}

// n bytes of the context's ChaCha20 keystream into device memory: the kernel reads the nonce
// from device memory and a second launch advances it, so every draw -- also every replay of a
// captured graph that contains one -- uses a fresh keystream (DESIGN.md "Randomness").
hm_status draw_random(hm_ctx *c, uint8_t *dst, size_t n, bool bump = true) {
    if (!n) return HM_OK;
    RandArgs R{};
    std::memcpy(R.key, c->chacha_key, sizeof(R.key));
    R.nonce = c->d_nonce, R.out = dst, R.nbytes = n;
    const int r = launch_random(R, c->stream, bump);
    wipe(R.key, sizeof(R.key));
    return r ? hip_fail(c, hipGetLastError()) : HM_OK;
}

} // namespace

// The context's auxiliary stream and its fork / mid / join events (the add pipeline, the
// multiplier's second Karatsuba lane), created on first use into locals and stored only when all
// of them exist.
hm_status hm::ensure_aux_stream(hm_ctx *c) {
    if (c->aux_stream) return HM_OK;
    hipStream_t s = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&ev[k], hipEventDisableTiming);
    if (e != hipSuccess) {
        for (hipEvent_t x : ev)
            if (x) (void)hipEventDestroy(x);
        if (s) (void)hipStreamDestroy(s);
        return hip_fail(c, e);
    }
    c->aux_stream = s, c->ev_fork = ev[0], c->ev_mid = ev[1], c->ev_join = ev[2];
    return HM_OK;
}

// The status an hm_* entry returns for the exception its function-try-block caught (HM_ABI_CATCH,
// ctx.h): host containers throw std::bad_alloc; nothing is allowed to unwind into a C, Rust or
// ctypes caller.
hm_status hm::exception_status() noexcept {
    try {
        throw;
    } catch (const std::bad_alloc &) {
        return HM_ERR_OUT_OF_MEMORY;
    } catch (...) {
        return HM_ERR_INTERNAL;
    }
}

// =============================================================================================
extern "C" {

const char *hm_status_string(int s) { // int: any value a foreign caller passes is defined
    switch (s) {
    case HM_OK: return "ok";
    case HM_ERR_INVALID_PARAMETERS: return "invalid parameters (d < min_d_over_delta * delta)";
    case HM_ERR_SECRET_KEY_UNSET: return "secret key unset";
    case HM_ERR_PUBLIC_KEY_UNSET: return "public key unset";
    case HM_ERR_DIVIDE_BY_ZERO: return "attempt to divide by zero";
    case HM_ERR_DIVISOR_IS_ONE: return "divisor is the constant 1";
    case HM_ERR_CAPACITY: return "output exceeds its capacity";
    case HM_ERR_UNSUPPORTED: return "unsupported size";
    case HM_ERR_HIP: return "HIP runtime error";
    case HM_ERR_INVALID_ARGUMENT: return "invalid argument";
    case HM_ERR_INVALID_CIPHERED_LENGTH: return "ciphered length is not a multiple of 8";
    case HM_ERR_BAD_INPUT: return "input degree does not match its limbs";
    case HM_ERR_RANDOMNESS: return "the OS random source failed";
    case HM_ERR_OUT_OF_MEMORY: return "host memory allocation failed";
    case HM_ERR_INTERNAL: return "internal error (C++ exception caught at the ABI)";
    }
    return "unknown status";
}

uint32_t hm_abi_version(void) { return HM_ABI_VERSION; }

hm_status hm_ctx_create(uint16_t d, uint16_t dp, uint16_t delta, uint16_t tau, int device,
                        hm_ctx **out) try {
    if (!out) return HM_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (d == 0 || dp == 0 || delta == 0 || tau == 0 || delta >= d) return HM_ERR_INVALID_PARAMETERS;
    hm_ctx *c = new (std::nothrow) hm_ctx();
    if (!c) return HM_ERR_OUT_OF_MEMORY;
    c->d = d, c->dp = dp, c->delta = delta, c->tau = tau, c->device = device;
    uint64_t nonce0 = 0;
    if (!os_random(c->chacha_key, sizeof(c->chacha_key)) || !os_random(&nonce0, sizeof(nonce0))) {
        delete c;
        return HM_ERR_RANDOMNESS; // CipherError::Randomness (src/cipher.rs:18-24)
    }
    DeviceGuard g(device);
    hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&c->d_status, sizeof(int));
    if (e == hipSuccess) e = hipMemset(c->d_status, 0, sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&c->d_nonce, sizeof(uint64_t));
    if (e == hipSuccess) e = hipMemcpy(c->d_nonce, &nonce0, sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (c->d_status) (void)hipFree(c->d_status);
        if (c->d_nonce) (void)hipFree(c->d_nonce);
        if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
        wipe(c->chacha_key, sizeof(c->chacha_key));
        delete c;
        return HM_ERR_HIP;
    }
    c->stream = c->own_stream;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess)
        cus = 256;
    c->cus = (uint32_t)std::max(cus, 1);
    // fp4 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4) is a gfx950 instruction: AUTO strategies use
    // the matrix cores only there, and an explicit MFMA request elsewhere is HM_ERR_UNSUPPORTED
    hipDeviceProp_t prop{};
    c->fp4_mfma = hipGetDeviceProperties(&prop, device) == hipSuccess &&
                  std::strncmp(prop.gcnArchName, "gfx950", 6) == 0;
    // test hook: HM_TEST_NO_FP4_MFMA=1 makes this context behave as on a device without the fp4
    // MFMA, so the VALU fallbacks and the explicit-MFMA error path run on the gfx950 test box
    if (const char *v = std::getenv("HM_TEST_NO_FP4_MFMA"); v && v[0] == '1') c->fp4_mfma = false;
    *out = c;
    return HM_OK;
} HM_ABI_CATCH

void hm_ctx_destroy(hm_ctx *c) try {
    if (!c) return;
    DeviceGuard g(c->device);
    (void)hipStreamSynchronize(c->stream);
    drop_secret(c);
    if (c->d_masks) (void)hipMemset(c->d_masks, 0, c->masks_bytes);
    mul_plans_release(c);
    for (void *p : {(void *)c->d_pk, (void *)c->d_pk_tab, (void *)c->d_pk_tab1, (void *)c->d_s,
                    (void *)c->d_ws_add, (void *)c->d_status, (void *)c->d_nonce,
                    (void *)c->d_masks, (void *)c->d_mws, (void *)c->d_kt})
        if (p) (void)hipFree(p);
    for (auto &r : c->retired) (void)hipFree(r.p);
    for (hipEvent_t e : {c->ev_fork, c->ev_mid, c->ev_join})
        if (e) (void)hipEventDestroy(e);
    if (c->aux_stream) (void)hipStreamDestroy(c->aux_stream);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    wipe(c->chacha_key, sizeof(c->chacha_key));
    wipe(&c->rng, sizeof(c->rng));
    delete c;
} catch (...) {
}

uint64_t hm_ctx_generation(const hm_ctx *c) { return c ? c->generation : 0; }

hm_status hm_ctx_trim(hm_ctx *c) try {
    if (!c) return HM_ERR_INVALID_ARGUMENT;
    DeviceGuard g(c->device);
    HM_HIP(c, hipStreamSynchronize(c->stream));
    for (auto &r : c->retired) (void)hipFree(r.p);
    c->retired.clear();
    return HM_OK;
} HM_ABI_CATCH

hm_status hm_ctx_set_stream(hm_ctx *c, void *s) try {
    if (!c) return HM_ERR_INVALID_ARGUMENT;
    c->stream = (hipStream_t)s; // NULL = the device's default (null) stream, as in HIP
    return HM_OK;
} HM_ABI_CATCH

void *hm_ctx_stream(const hm_ctx *c) { return c ? (void *)c->stream : nullptr; }

hm_status hm_ctx_parameters(const hm_ctx *c, uint16_t *d, uint16_t *dp, uint16_t *delta,
                            uint16_t *tau) try {
    if (!c) return HM_ERR_INVALID_ARGUMENT;
    if (d) *d = c->d;
    if (dp) *dp = c->dp;
    if (delta) *delta = c->delta;
    if (tau) *tau = c->tau;
    return HM_OK;
} HM_ABI_CATCH

hm_status hm_ctx_set_secret_key(hm_ctx *c, const uint64_t *limbs, size_t n) try {
    if (!c || !limbs || n == 0) return HM_ERR_INVALID_ARGUMENT; // from_bytes asserts non-empty
    drop_secret(c);
    c->sk.assign(limbs, limbs + n);
    c->has_sk = true;
    c->has_pk = false; // set_secret_key clears the public key (src/context.rs:568-571)
    return HM_OK;
} HM_ABI_CATCH

hm_status hm_ctx_set_public_key(hm_ctx *c, const uint64_t *limbs, uint32_t tau, uint32_t lpp) try {
    if (!c || !limbs || tau == 0 || lpp == 0) return HM_ERR_INVALID_ARGUMENT;
    c->pk.assign(limbs, limbs + (size_t)tau * lpp);
    c->pk_tau = tau, c->pk_cap = lpp;
    c->pk_maxdeg = 0;
    for (uint32_t i = 0; i < tau; ++i)
        c->pk_maxdeg = std::max<uint32_t>(c->pk_maxdeg, (uint32_t)degree_of(&c->pk[(size_t)i * lpp], lpp));
    c->pk_top1 = tau <= 128 && lpp > 1;
    std::memset(c->pk_topcol, 0, sizeof(c->pk_topcol));
    for (uint32_t i = 0; i < tau && c->pk_top1; ++i) {
        const uint64_t top = c->pk[(size_t)i * lpp + lpp - 1];
        if (top > 1) c->pk_top1 = false;
        else c->pk_topcol[i / 32] |= (uint32_t)top << (i % 32);
    }
    hm_status st = upload_pk(c);
    if (st == HM_OK) c->has_pk = true;
    return st;
} HM_ABI_CATCH

hm_status hm_ctx_seed_rng(hm_ctx *c, uint64_t seed) try {
    if (!c) return HM_ERR_INVALID_ARGUMENT;
    // test contract: keys from SplitMix64(seed), masks from ChaCha20 keyed by SplitMix64(seed ^ K)
    c->seeded = true;
    c->rng = seed;
    uint64_t ks = seed ^ 0x6D61736B73636861ull; // "masksCha"
    for (int i = 0; i < 4; ++i) {
        const uint64_t w = splitmix64(ks);
        c->chacha_key[2 * i] = (uint32_t)w, c->chacha_key[2 * i + 1] = (uint32_t)(w >> 32);
    }
    const uint64_t nonce0 = splitmix64(ks);
    DeviceGuard g(c->device);
    HM_HIP(c, hipMemcpyAsync(c->d_nonce, &nonce0, sizeof(nonce0), hipMemcpyHostToDevice, c->stream));
    HM_HIP(c, hipStreamSynchronize(c->stream));
    return HM_OK;
} HM_ABI_CATCH

hm_status hm_ctx_generate_secret_key(hm_ctx *c) try { // src/context.rs:421-424
    if (!c) return HM_ERR_INVALID_ARGUMENT;
    std::vector<uint64_t> s;
    if (!random_poly(c, c->d, s)) return HM_ERR_RANDOMNESS;
    hm_status st = hm_ctx_set_secret_key(c, s.data(), s.size());
    wipe(s.data(), s.size() * 8);
    return st;
} HM_ABI_CATCH

hm_status hm_ctx_generate_public_key(hm_ctx *c) try { // src/context.rs:249-261, :444-454
    if (!c) return HM_ERR_INVALID_ARGUMENT;
    if (!c->has_sk) return HM_ERR_SECRET_KEY_UNSET;
    // T_i = S*Q_i + X*R_i.  deg S is d for generated keys but any degree for a key set with
    // set_secret_key (the reference's own example, SecretKey::from_bytes(&[5, 14, 8]) at d = 6,
    // has degree 19): rows are as wide as the widest T_i needs.
    std::vector<std::vector<uint64_t>> rows(c->tau);
    size_t cap = 1;
    for (uint32_t i = 0; i < c->tau; ++i) {
        std::vector<uint64_t> q, r;
        if (!random_poly(c, c->dp, q) || !random_poly(c, c->delta, r)) return HM_ERR_RANDOMNESS;
        std::vector<uint64_t> t = clmul_host(c->sk, q);
        t.resize(std::max(t.size(), r.size() + 1), 0);
        for (size_t w = 0; w < r.size(); ++w) { // + X * R
            t[w] ^= r[w] << 1;
            t[w + 1] ^= r[w] >> 63;
        }
        wipe(q.data(), q.size() * 8);
        wipe(r.data(), r.size() * 8);
        cap = std::max(cap, (size_t)degree_of(t.data(), t.size()) / 64 + 1);
        rows[i] = std::move(t);
    }
    std::vector<uint64_t> all((size_t)c->tau * cap, 0);
    for (uint32_t i = 0; i < c->tau; ++i)
        for (size_t w = 0; w < cap && w < rows[i].size(); ++w) all[(size_t)i * cap + w] = rows[i][w];
    return hm_ctx_set_public_key(c, all.data(), c->tau, (uint32_t)cap);
} HM_ABI_CATCH

hm_status hm_ctx_get_secret_key(const hm_ctx *c, uint64_t *limbs, size_t cap, size_t *n) try {
    if (!c) return HM_ERR_INVALID_ARGUMENT;
    if (!c->has_sk) return HM_ERR_SECRET_KEY_UNSET;
    if (n) *n = c->sk.size();
    if (limbs) {
        if (cap < c->sk.size()) return HM_ERR_CAPACITY;
        std::memcpy(limbs, c->sk.data(), c->sk.size() * 8);
    }
    return HM_OK;
} HM_ABI_CATCH

hm_status hm_ctx_get_public_key(const hm_ctx *c, uint64_t *limbs, size_t cap, uint32_t *tau,
                                uint32_t *lpp) try {
    if (!c) return HM_ERR_INVALID_ARGUMENT;
    if (!c->has_pk) return HM_ERR_PUBLIC_KEY_UNSET;
    if (tau) *tau = c->pk_tau;
    if (lpp) *lpp = c->pk_cap;
    if (limbs) {
        if (cap < c->pk.size()) return HM_ERR_CAPACITY;
        std::memcpy(limbs, c->pk.data(), c->pk.size() * 8);
    }
    return HM_OK;
} HM_ABI_CATCH

hm_status hm_ctx_set_kernel_timing(hm_ctx *c, int enable) try {
    if (!c || enable < HM_TIME_OFF || enable > HM_TIME_DECRYPT) return HM_ERR_INVALID_ARGUMENT;
    DeviceGuard g(c->device);
    HM_HIP(c, hipStreamSynchronize(c->stream));
    const size_t half = (size_t)kTimedLaunches * kTimerWaves * sizeof(unsigned long long);
    if (enable && !c->d_kt) {
        void *p = nullptr;
        HM_HIP(c, hipMalloc(&p, 2 * half));
        c->d_kt = (unsigned long long *)p;
    }
    if (c->d_kt) { // reset: starts at the maximum (atomic min), ends at 0 (atomic max)
        HM_HIP(c, hipMemset(c->d_kt, 0xFF, half));
        HM_HIP(c, hipMemset((char *)c->d_kt + half, 0, half));
    }
    c->time_kernel = (uint32_t)enable;
    c->kt_next = 0;
    return HM_OK;
} HM_ABI_CATCH

hm_status hm_ctx_clear_kernel_timing(hm_ctx *c) try {
    if (!c) return HM_ERR_INVALID_ARGUMENT;
    if (!c->d_kt) return HM_OK;
    DeviceGuard g(c->device);
    HM_HIP(c, hipStreamSynchronize(c->stream));
    const size_t half = (size_t)kTimedLaunches * kTimerWaves * sizeof(unsigned long long);
    HM_HIP(c, hipMemsetAsync(c->d_kt, 0xFF, half, c->stream));
    HM_HIP(c, hipMemsetAsync((char *)c->d_kt + half, 0, half, c->stream));
    HM_HIP(c, hipStreamSynchronize(c->stream));
    return HM_OK;
} HM_ABI_CATCH

hm_status hm_ctx_kernel_timing(hm_ctx *c, double *total_ms, uint32_t *launches) try {
    if (!c || !total_ms || !launches) return HM_ERR_INVALID_ARGUMENT;
    *total_ms = 0.0, *launches = 0;
    if (!c->d_kt || !c->kt_next) return HM_OK;
    DeviceGuard g(c->device);
    HM_HIP(c, hipStreamSynchronize(c->stream));
    const size_t n = (size_t)c->kt_next * kTimerWaves;
    std::vector<unsigned long long> t0(n), t1(n);
    HM_HIP(c, hipMemcpy(t0.data(), c->d_kt, n * 8, hipMemcpyDeviceToHost));
    HM_HIP(c, hipMemcpy(t1.data(), c->d_kt + (size_t)kTimedLaunches * kTimerWaves, n * 8,
                        hipMemcpyDeviceToHost));
    int rate_khz = 0; // the wall clock's frequency (100 MHz on gfx9)
    HM_HIP(c, hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, c->device));
    if (rate_khz <= 0) return HM_ERR_UNSUPPORTED;
    double ticks = 0.0;
    uint32_t k = 0;
    for (uint32_t s = 0; s < c->kt_next; ++s) {
        unsigned long long lo = ~0ull, hi = 0ull;
        for (size_t w = (size_t)s * kTimerWaves; w < (size_t)(s + 1) * kTimerWaves; ++w)
            lo = std::min(lo, t0[w]), hi = std::max(hi, t1[w]);
        if (lo == ~0ull || hi < lo) continue; // (a slot whose launch has not run)
        ticks += (double)(hi - lo);
        ++k;
    }
    *total_ms = ticks / rate_khz;
    *launches = k;
    return HM_OK;
} HM_ABI_CATCH

hm_status hm_ctx_set_add_options(hm_ctx *c, uint32_t chain) try {
    if (!c || chain > HM_ADD_CHAIN_VALU) return HM_ERR_INVALID_ARGUMENT;
    c->add_chain = chain;
    return HM_OK;
} HM_ABI_CATCH

hm_status hm_ctx_set_mul_options(hm_ctx *c, uint32_t ka_min, uint32_t ka_leaf) try {
    if (!c || (ka_min && (ka_leaf < 32 || ka_leaf > 512))) return HM_ERR_INVALID_ARGUMENT;
    c->ka_min = ka_min;
    c->ka_leaf = ka_leaf & ~31u;
    return HM_OK;
} HM_ABI_CATCH

hm_status hm_ctx_set_mul_scratch(hm_ctx *c, uint64_t words) try {
    if (!c || words == 0 || words > (1ull << 27) + (1ull << 26)) return HM_ERR_INVALID_ARGUMENT;
    c->ka_scratch = words;
    return HM_OK;
} HM_ABI_CATCH

hm_status hm_ctx_set_mul_chunk(hm_ctx *c, uint64_t max_values) try {
    if (!c) return HM_ERR_INVALID_ARGUMENT;
    c->mul_chunk = max_values;
    return HM_OK;
} HM_ABI_CATCH

hm_status hm_ctx_set_add_pipeline(hm_ctx *c, int enable) try {
    if (!c) return HM_ERR_INVALID_ARGUMENT;
    c->add_pipe = enable != 0;
    return HM_OK;
} HM_ABI_CATCH

hm_status hm_ctx_set_mul_products(hm_ctx *c, uint32_t products) try {
    if (!c || products > HM_MUL_PRODUCTS_VALU) return HM_ERR_INVALID_ARGUMENT;
    if (products == HM_MUL_PRODUCTS_MFMA && !c->fp4_mfma) return HM_ERR_UNSUPPORTED;
    c->mul_products = products;
    return HM_OK;
} HM_ABI_CATCH

hm_status hm_validate_operation(const hm_ctx *c, hm_op op, uint16_t *req) try {
    if (!c || needs_width(op)) return HM_ERR_INVALID_ARGUMENT; // those need a width (_bits)
    const uint16_t m = min_d_over_delta(op);
    if (req) *req = m;
    if ((uint32_t)c->d < (uint32_t)m * (uint32_t)c->delta) return HM_ERR_INVALID_PARAMETERS;
    return HM_OK;
} HM_ABI_CATCH

hm_status hm_validate_operation_bits(const hm_ctx *c, hm_op op, uint32_t nbits, uint16_t *req) try {
    if (!needs_width(op)) return hm_validate_operation(c, op, req);
    if (!c || nbits == 0 || nbits > HM_MAX_BITS) return HM_ERR_INVALID_ARGUMENT;
    if (is_shift_op(op) && !shift_plan::stages(nbits)) return HM_ERR_INVALID_ARGUMENT;
    if (is_array_op(op) && nbits > kArrayMaxIndex) return HM_ERR_INVALID_ARGUMENT; // index bits
    const uint16_t m = borrow_min_d_over_delta(op, nbits);
    if (req) *req = m;
    if ((uint32_t)c->d < (uint32_t)m * (uint32_t)c->delta) return HM_ERR_INVALID_PARAMETERS;
    return HM_OK;
} HM_ABI_CATCH

// A fresh ciphertext bit is a subset sum of public-key rows (plus the plaintext bit), so its
// degree is at most max(d + dp, deg T_i): d + dp for generated keys, more for a loaded key.
uint32_t hm_fresh_bound(const hm_ctx *c) {
    if (!c) return 0;
    const uint32_t b = (uint32_t)c->d + c->dp;
    return c->has_pk ? std::max(b, c->pk_maxdeg) : b;
}

uint32_t hm_ctx_mask_bytes(const hm_ctx *c) { return (c && c->has_pk) ? (c->pk_tau + 7) / 8 : 0; }

uint64_t hm_batch_stride(uint32_t nbits, const uint32_t *bound) {
    uint64_t s = 0;
    for (uint32_t i = 0; i < nbits; ++i) s += cap_of(bound[i]);
    return s;
}

// Degree bounds of common.rs:37-56 (deg(xy) = deg x + deg y, deg(x+y) <= max).
hm_status hm_add_out_bounds(uint32_t L, const uint32_t *a, const uint32_t *b, uint32_t *out) try {
    if (!a || !b || !out || L == 0 || L > HM_MAX_BITS) return HM_ERR_INVALID_ARGUMENT;
    int64_t c = -1; // null carry
    for (uint32_t i = 0; i < L; ++i) {
        const int64_t x = std::max<int64_t>(a[i], b[i]);
        const int64_t s = std::max(x, c);
        if (s >= (int64_t)1 << 30) return HM_ERR_UNSUPPORTED;
        out[i] = (uint32_t)s;
        if (i + 1 < L) {
            const int64_t ab = (int64_t)a[i] + b[i];
            const int64_t p = x + ab;
            c = (c < 0) ? ab : std::max(ab, p + c);
        }
    }
    return HM_OK;
} HM_ABI_CATCH

// Degree bounds of the ripple-borrow circuits.
hm_status hm_sub_out_bounds(uint32_t L, const uint32_t *a, const uint32_t *b, uint32_t *out) try {
    if (!a || !b || !out || L == 0 || L > HM_MAX_BITS) return HM_ERR_INVALID_ARGUMENT;
    return sub_bounds(L, a, b, out);
} HM_ABI_CATCH

hm_status hm_compare_out_bounds(hm_op cmp, uint32_t L, const uint32_t *a, const uint32_t *b,
                                uint32_t out[8]) try {
    if (!a || !b || !out || L == 0 || L > HM_MAX_BITS || !is_compare_op(cmp))
        return HM_ERR_INVALID_ARGUMENT;
    return compare_bounds(is_ordering_op(cmp), L, a, b, out);
} HM_ABI_CATCH

// Degree bounds of select, min and max.
hm_status hm_select_out_bounds(uint32_t L, uint32_t cond_bound0, const uint32_t *a,
                               const uint32_t *b, uint32_t *out) try {
    if (!a || !b || !out || L == 0 || L > HM_MAX_BITS) return HM_ERR_INVALID_ARGUMENT;
    return choice_bounds(L, cond_bound0, a, b, out);
} HM_ABI_CATCH

// Degree bounds of a table lookup: per output bit the widest monomial of its
// algebraic normal form.
hm_status hm_lookup_out_bounds(uint32_t in_bits, const uint32_t *a, const uint8_t *table,
                               uint32_t out_nbytes, uint32_t *out) try {
    if (!a || !table || !out || in_bits == 0 || in_bits > kLookupMaxIn ||
        (out_nbytes != 1 && out_nbytes != 2 && out_nbytes != 4))
        return HM_ERR_INVALID_ARGUMENT;
    uint32_t coef[kLookupMaxOut][8];
    lookup_plan::moebius(in_bits, table, out_nbytes, coef);
    return lookup_plan::bounds(in_bits, a, coef, 8 * out_nbytes, out);
} HM_ABI_CATCH

// Degree bounds of a shift or rotate by an encrypted amount.
hm_status hm_shift_out_bounds(hm_op which, uint32_t nbits, const uint32_t *a, const uint32_t *s,
                              uint32_t *out) try {
    if (!a || !s || !out || !is_shift_op(which) || !shift_plan::stages(nbits))
        return HM_ERR_INVALID_ARGUMENT;
    return shift_plan::bounds(which, nbits, a, s, out);
} HM_ABI_CATCH

// Degree bounds of a bit count.
hm_status hm_bitcount_out_bounds(hm_op which, uint32_t nbits, const uint32_t *a,
                                 uint32_t out[8]) try {
    if (!a || !out || !is_bitcount_op(which) || nbits == 0 || nbits > HM_MAX_BITS)
        return HM_ERR_INVALID_ARGUMENT;
    return bitcount_plan::bounds(which, nbits, a, out);
} HM_ABI_CATCH

// Degree bounds of an array read or write by an encrypted index.
hm_status hm_array_read_out_bounds(uint32_t nbits, const uint32_t *arr, uint32_t count,
                                   const uint32_t *s, uint32_t *out) try {
    if (!arr || !s || !out || nbits == 0 || nbits > HM_MAX_BITS || !array_plan::index_bits(count))
        return HM_ERR_INVALID_ARGUMENT;
    return array_plan::read_bounds(nbits, arr, count, s, out);
} HM_ABI_CATCH

hm_status hm_array_write_out_bounds(uint32_t nbits, const uint32_t *arr, const uint32_t *x,
                                    uint32_t count, const uint32_t *s, uint32_t *out) try {
    if (!arr || !x || !s || !out || nbits == 0 || nbits > HM_MAX_BITS ||
        !array_plan::index_bits(count))
        return HM_ERR_INVALID_ARGUMENT;
    return array_plan::write_bounds(nbits, arr, x, count, s, out);
} HM_ABI_CATCH

hm_status hm_minmax_out_bounds(uint32_t L, const uint32_t *a, const uint32_t *b,
                               uint32_t *out) try {
    if (!a || !b || !out || L == 0 || L > HM_MAX_BITS) return HM_ERR_INVALID_ARGUMENT;
    return minmax_bounds(L, a, b, out);
} HM_ABI_CATCH

hm_status hm_mul_out_bounds(uint32_t L, const uint32_t *a, const uint32_t *b, int is_signed,
                            uint32_t *out) try {
    if (!a || !b || !out || L == 0 || L > HM_MAX_BITS) return HM_ERR_INVALID_ARGUMENT;
    std::vector<int64_t> res;
    if (!mul_result_bounds(L, L, a, b, is_signed != 0, res)) return HM_ERR_UNSUPPORTED;
    for (uint32_t i = 0; i < L; ++i) out[i] = (uint32_t)std::max<int64_t>(res[i], 0);
    return HM_OK;
} HM_ABI_CATCH

hm_status hm_mul_cost(uint32_t L, uint32_t k, const uint32_t *a, const uint32_t *b, int is_signed,
                      double *word_pairs, double *out_bytes, double *max_degree) try {
    if (!a || !b || L == 0 || L > HM_MAX_BITS || k == 0 || k > L) return HM_ERR_INVALID_ARGUMENT;
    (void)is_signed; // the signed corners (+1 in column L-1) change no bound
    double w, o, m;
    mul_cost_model(L, k, a, b, w, o, m);
    if (word_pairs) *word_pairs = w;
    if (out_bytes) *out_bytes = o;
    if (max_degree) *max_degree = m;
    return HM_OK;
} HM_ABI_CATCH

hm_status hm_mul_plan_work(hm_ctx *c, uint32_t L, uint32_t k, const uint32_t *a, const uint32_t *b,
                          int is_signed, double *word_pairs) try {
    if (!c || !a || !b || !word_pairs || L == 0 || L > HM_MAX_BITS || k == 0 || k > L)
        return HM_ERR_INVALID_ARGUMENT;
    return mul_plan_work(c, L, k, a, b, is_signed != 0 && k == L, *word_pairs);
} HM_ABI_CATCH

hm_status hm_gate_out_bounds(hm_op g, uint32_t L, const uint32_t *a, const uint32_t *b,
                             uint32_t *out) try {
    if (!a || !out || L == 0 || L > HM_MAX_BITS) return HM_ERR_INVALID_ARGUMENT;
    if (g != HM_OP_NOT && !b) return HM_ERR_INVALID_ARGUMENT;
    return gate_bounds(g, L, a, b, out);
} HM_ABI_CATCH

// ------------------------------------------------------------------ cipher
hm_status hm_encrypt_batch(hm_ctx *c, const uint8_t *data, uint32_t nbytes, const uint8_t *masks,
                           hm_batch *out) try {
    if (!c || !out) return HM_ERR_INVALID_ARGUMENT;
    if (!c->has_pk) return HM_ERR_PUBLIC_KEY_UNSET;
    if (hm_status st = check_batch(out); st) return st;
    if (nbytes == 0 || out->nbits != 8 * nbytes) return HM_ERR_INVALID_ARGUMENT;
    if (out->n && !data) return HM_ERR_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < out->nbits; ++i)
        if (out->bound[i] < c->pk_maxdeg) return HM_ERR_INVALID_ARGUMENT;
    if (out->n == 0) return HM_OK;
    // launch_encrypt instantiates pk_cap <= 17 limbs; reject the rest BEFORE a mask draw (the
    // encryption kernel advances the CSPRNG nonce: a draw without it would repeat its keystream)
    if (c->pk_cap == 0 || c->pk_cap > 17) return HM_ERR_UNSUPPORTED;
    DeviceGuard g(c->device);
    EncArgs E{};
    E.pk = c->d_pk, E.tau = c->pk_tau, E.pk_cap = c->pk_cap;
    E.pk_tab = c->d_pk_tab;
    E.pk_tab1 = c->d_pk_tab1;
    E.cus = c->cus;
    E.lognbits = -1;
    for (int s = 0; s < 8; ++s)
        if ((8u * nbytes) == (1u << s)) E.lognbits = s;
    E.data = data, E.nbytes = nbytes;
    E.out = batch_arg(out);
    E.n = out->n;
    E.status = c->d_status;
    fill_bounds(E.ob, out);
    E.uniform_cap = 1;
    for (uint32_t i = 0, o = 0; i < out->nbits; ++i) {
        E.ooff.b[i] = o, o += cap_of(out->bound[i]);
        E.uniform_cap &= cap_of(out->bound[i]) == c->pk_cap;
    }
#ifndef HM_ENC_NO_TOP1
    E.top1 = c->pk_top1 && c->d_pk_tab1 ? 1u : 0u;
#endif
    std::memcpy(E.topcol, c->pk_topcol, sizeof(E.topcol));
    if (!masks) {
        // CipheredBit::part draws ceil(tau/8) random bytes per bit (cipher.rs:92-97): here the
        // device ChaCha20 stream, drawn into the context's mask buffer right before the launch;
        // the encryption kernel advances the nonce (no bump launch of its own)
        const size_t mb = (size_t)out->n * out->nbits * ((c->pk_tau + 7) / 8);
        const size_t need = (mb + 63) & ~(size_t)63;
        if (need > c->masks_bytes && c->d_masks) (void)hipMemset(c->d_masks, 0, c->masks_bytes);
        HM_HIP(c, grow(c, c->d_masks, c->masks_bytes, need));
        if (hm_status st = draw_random(c, c->d_masks, mb, false); st) return st;
        masks = c->d_masks;
        E.nonce_bump = c->d_nonce;
    }
    E.masks = masks;
    E.kt = c->ktimer(HM_TIME_ENCRYPT);
    int r = launch_encrypt(E, c->stream);
    if (r == HM_ERR_UNSUPPORTED) return HM_ERR_UNSUPPORTED;
    return r ? hip_fail(c, hipGetLastError()) : HM_OK;
} HM_ABI_CATCH

hm_status hm_random_bytes(hm_ctx *c, uint8_t *dst, size_t nbytes) try {
    if (!c || (nbytes && !dst)) return HM_ERR_INVALID_ARGUMENT;
    DeviceGuard g(c->device);
    return draw_random(c, dst, nbytes);
} HM_ABI_CATCH

hm_status hm_decrypt_batch(hm_ctx *c, const hm_batch *in, uint8_t *out) try {
    if (!c || !in) return HM_ERR_INVALID_ARGUMENT;
    if (!c->has_sk) return HM_ERR_SECRET_KEY_UNSET;
    if (in->nbits % 8) return HM_ERR_INVALID_CIPHERED_LENGTH; // cipher.rs:218-220
    if (hm_status st = check_batch(in); st) return st;
    if (in->n == 0) return HM_OK;
    if (!out) return HM_ERR_INVALID_ARGUMENT;
    uint32_t mb = 0;
    for (uint32_t i = 0; i < in->nbits; ++i) mb = std::max(mb, in->bound[i]);
    if (hm_status st = ensure_ztable(c, mb); st) return st;
    DecArgs D{};
    D.in = batch_arg(in);
    D.n = in->n, D.nbits = in->nbits;
    D.z = c->d_z, D.zlimbs = c->z_limbs;
    D.out = out;
    D.status = c->d_status;
    fill_bounds(D.ib, in);
    for (uint32_t i = 0, o = 0; i < in->nbits; ++i) {
        D.ioff.b[i] = o;
        o += cap_of(in->bound[i]);
        D.maxcap = std::max(D.maxcap, cap_of(in->bound[i]));
    }
    D.ucap = cap_of(in->bound[0]) <= 8 ? cap_of(in->bound[0]) : 0;
    for (uint32_t i = 1; i < in->nbits; ++i)
        if (cap_of(in->bound[i]) != D.ucap) D.ucap = 0;
    D.kt = c->ktimer(HM_TIME_DECRYPT);
    DeviceGuard g(c->device);
    return launch_decrypt(D, c->stream) ? hip_fail(c, hipGetLastError()) : HM_OK;
} HM_ABI_CATCH

// ------------------------------------------------------------------ operations
hm_status hm_add_batch(hm_ctx *c, const hm_batch *a, const hm_batch *b, hm_batch *out) try {
    if (!c || !a || !b || !out) return HM_ERR_INVALID_ARGUMENT;
    if (hm_status st = hm_validate_operation(c, HM_OP_ADD, nullptr); st) return st;
    if (hm_status st = check_operands({{a, 0}, {b, 0}, {out, 0}}); st) return st;
    const uint32_t L = a->nbits;
    std::vector<uint32_t> need(L);
    if (hm_status st = hm_add_out_bounds(L, a->bound, b->bound, need.data()); st) return st;
    if (!covers(out, need)) return HM_ERR_INVALID_ARGUMENT;
    if (a->n == 0) return HM_OK;
    // workspace slots, the prep's shape and the chain's LDS plan, from the static bounds
    AddArgs A{};
    const AddShape shape{L, a->bound, b->bound, a->n, c->add_chain, c->fp4_mfma};
    if (hm_status st = plan_add(shape, A); st) return st;
    const size_t bytes = (size_t)A.ws_stride * 4 * a->n;
    DeviceGuard g(c->device);
    HM_HIP(c, grow(c, c->d_ws_add, c->ws_add_bytes, bytes));
    A.ws = c->d_ws_add;
    A.a = batch_arg(a), A.b = batch_arg(b), A.out = batch_arg(out);
    A.n = a->n, A.nbits = L, A.status = c->d_status;
    fill_bounds(A.ab, a), fill_bounds(A.bb, b), fill_bounds(A.ob, out);
    A.kt = c->ktimer(HM_TIME_ADD_CHAIN);
    // Two-stage pipeline (not while timing the chain): the batch in two halves, the second
    // half's prep on the auxiliary stream right after the first half's, so it runs beside the
    // first half's chain (the chain is matrix-core and latency bound, the prep VALU bound); the
    // halves use disjoint workspace and outputs.  Fork / join by events, so a graph captured on
    // the context stream holds both branches.
    if (c->add_pipe && !A.kt.t0 && A.mfma && a->n >= 2 * kAddPipeMin) {
        if (hm_status st = ensure_aux_stream(c); st) return st;
        const uint64_t h = (a->n / 2 + kAddWavesPerBlock - 1) / kAddWavesPerBlock * kAddWavesPerBlock;
        const AddArgs A1 = add_args_slice(A, 0, h), A2 = add_args_slice(A, h, a->n - h);
        HM_HIP(c, hipEventRecord(c->ev_fork, c->stream));
        HM_HIP(c, hipStreamWaitEvent(c->aux_stream, c->ev_fork, 0));
        if (launch_add_prep(A1, c->stream)) return hip_fail(c, hipGetLastError());
        HM_HIP(c, hipEventRecord(c->ev_mid, c->stream));
        if (launch_add_chain_mfma(A1, c->stream)) return hip_fail(c, hipGetLastError());
        HM_HIP(c, hipStreamWaitEvent(c->aux_stream, c->ev_mid, 0));
        if (launch_add_prep(A2, c->aux_stream)) return hip_fail(c, hipGetLastError());
        if (launch_add_chain_mfma(A2, c->aux_stream)) return hip_fail(c, hipGetLastError());
        HM_HIP(c, hipEventRecord(c->ev_join, c->aux_stream));
        HM_HIP(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
        return HM_OK;
    }
    return launch_add(A, c->stream) ? hip_fail(c, hipGetLastError()) : HM_OK;
} HM_ABI_CATCH

hm_status hm_mul_batch(hm_ctx *c, const hm_batch *a, const hm_batch *b, int is_signed,
                       hm_batch *out) try {
    if (!c || !a || !b || !out) return HM_ERR_INVALID_ARGUMENT;
    if (hm_status st = hm_validate_operation(c, is_signed ? HM_OP_MUL_SIGNED : HM_OP_MUL, nullptr); st)
        return st;
    if (hm_status st = check_operands({{a, 0}, {b, 0}, {out, 0}}); st) return st;
    return mul_columns(c, a, b, a->nbits, is_signed != 0, out);
} HM_ABI_CATCH

hm_status hm_mul_low_batch(hm_ctx *c, const hm_batch *a, const hm_batch *b, uint32_t k,
                           hm_batch *out) try {
    if (!c || !a || !b || !out) return HM_ERR_INVALID_ARGUMENT;
    if (hm_status st = hm_validate_operation(c, HM_OP_MUL, nullptr); st) return st;
    if (hm_status st = check_operands({{a, 0}, {b, 0}, {out, k}}); st) return st;
    if (k == 0 || k > a->nbits) return HM_ERR_INVALID_ARGUMENT; // (k = 0 asked out for a's width)
    return mul_columns(c, a, b, k, false, out);
} HM_ABI_CATCH

hm_status hm_gate_batch(hm_ctx *c, hm_op gate, const hm_batch *a, const hm_batch *b,
                        hm_batch *out) try {
    if (!c || !a || !out) return HM_ERR_INVALID_ARGUMENT;
    if (gate > HM_OP_NOT) return HM_ERR_INVALID_ARGUMENT;
    if (hm_status st = hm_validate_operation(c, gate, nullptr); st) return st;
    if (gate == HM_OP_NOT) b = nullptr; // (a unary gate's b is not looked at)
    // (out before b: the order this entry checks them in)
    if (hm_status st = gate == HM_OP_NOT ? check_operands({{a, 0}, {out, 0}})
                                         : check_operands({{a, 0}, {out, 0}, {b, 0}});
        st)
        return st;
    const uint32_t L = a->nbits;
    std::vector<uint32_t> need(L);
    if (hm_status st = hm_gate_out_bounds(gate, L, a->bound, b ? b->bound : nullptr, need.data()); st)
        return st;
    if (!covers(out, need)) return HM_ERR_INVALID_ARGUMENT;
    if (a->n == 0) return HM_OK;
    GateArgs G{};
    G.op = gate;
    if (hm_status st = plan_gate(L, a->bound, b ? b->bound : nullptr, G); st) return st;
    fill_io(G.io, c, a, b, out);
    return run_circuit(c, G, launch_gate);
} HM_ABI_CATCH

// The ripple-borrow kernel over checked batches (a, b: L bits; out covers its bounds).  chain: the
// degree bound of the last borrow (or equality prefix) the kernel forms.
static hm_status borrow_run(hm_ctx *c, int mode, bool flip, bool sgn, const hm_batch *a,
                            const hm_batch *b, hm_batch *out, int64_t chain) {
    BorrowArgs G{};
    G.mode = mode, G.flip = flip, G.sgn = sgn;
    if (hm_status st = plan_borrow(a->nbits, a->bound, b->bound, chain, G.lay); st) return st;
    fill_io(G.io, c, a, b, out);
    return run_circuit(c, G, launch_borrow);
}

hm_status hm_sub_batch(hm_ctx *c, const hm_batch *a, const hm_batch *b, hm_batch *out) try {
    if (!c || !a || !b || !out) return HM_ERR_INVALID_ARGUMENT;
    if (hm_status st = check_operands({{a, 0}, {b, 0}, {out, 0}}); st) return st;
    const uint32_t L = a->nbits;
    if (hm_status st = hm_validate_operation_bits(c, HM_OP_SUB, L, nullptr); st) return st;
    std::vector<uint32_t> need(L);
    if (hm_status st = hm_sub_out_bounds(L, a->bound, b->bound, need.data()); st) return st;
    if (!covers(out, need)) return HM_ERR_INVALID_ARGUMENT;
    if (a->n == 0) return HM_OK;
    std::vector<int64_t> wb;
    borrow_bounds(L - 1, a->bound, b->bound, wb);
    return borrow_run(c, kBorrowSub, false, false, a, b, out, wb[L - 1]);
} HM_ABI_CATCH

hm_status hm_compare_batch(hm_ctx *c, hm_op cmp, const hm_batch *a, const hm_batch *b,
                           int is_signed, hm_batch *out) try {
    if (!c || !a || !b || !out || !is_compare_op(cmp)) return HM_ERR_INVALID_ARGUMENT;
    if (hm_status st = check_operands({{a, 0}, {b, 0}, {out, 8}}); st) return st;
    const uint32_t L = a->nbits;
    if (hm_status st = hm_validate_operation_bits(c, cmp, L, nullptr); st) return st;
    std::vector<uint32_t> need(8);
    if (hm_status st = hm_compare_out_bounds(cmp, L, a->bound, b->bound, need.data()); st)
        return st;
    if (!covers(out, need)) return HM_ERR_INVALID_ARGUMENT;
    if (a->n == 0) return HM_OK;
    if (cmp == HM_OP_GT || cmp == HM_OP_LE) std::swap(a, b); // a > b is b < a
    const bool flip = cmp == HM_OP_NE || cmp == HM_OP_GE || cmp == HM_OP_LE;
    const bool ord = is_ordering_op(cmp);
    return borrow_run(c, ord ? kBorrowLt : kBorrowEq, flip, ord && is_signed != 0, a, b, out,
                      need[0]);
} HM_ABI_CATCH

// out's limbs or degree words share device memory with in's
static bool overlaps(const hm_batch *out, const hm_batch *in) {
    auto cross = [](const void *p, uint64_t pn, const void *q, uint64_t qn) {
        const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
        return pn && qn && a < b + qn && b < a + pn;
    };
    return cross(out->limbs, 8 * out->n * hm_batch_stride(out->nbits, out->bound), in->limbs,
                 8 * in->n * hm_batch_stride(in->nbits, in->bound)) ||
           cross(out->degree, 4 * out->n * out->nbits, in->degree, 4 * in->n * in->nbits);
}

hm_status hm_minmax_batch(hm_ctx *c, hm_op which, const hm_batch *a, const hm_batch *b,
                          int is_signed, hm_batch *out) try {
    if (!c || !a || !b || !out || !is_minmax_op(which)) return HM_ERR_INVALID_ARGUMENT;
    if (hm_status st = check_operands({{a, 0}, {b, 0}, {out, 0}}); st) return st;
    const uint32_t L = a->nbits;
    if (hm_status st = hm_validate_operation_bits(c, which, L, nullptr); st) return st;
    std::vector<uint32_t> need(L);
    if (hm_status st = hm_minmax_out_bounds(L, a->bound, b->bound, need.data()); st) return st;
    if (!covers(out, need) || overlaps(out, a) || overlaps(out, b)) return HM_ERR_INVALID_ARGUMENT;
    if (a->n == 0) return HM_OK;
    std::vector<int64_t> wb;
    borrow_bounds(L, a->bound, b->bound, wb);
    MinMaxArgs G{};
    G.is_max = which == HM_OP_MAX, G.sgn = is_signed != 0;
    // borrow_run's layout with chain = wb_L (the phase-2 product x_i w_L, circuit_host.h)
    if (hm_status st = plan_borrow(L, a->bound, b->bound, wb[L], G.lay); st) return st;
    fill_io(G.io, c, a, b, out);
    return run_circuit(c, G, launch_minmax);
} HM_ABI_CATCH

hm_status hm_select_batch(hm_ctx *c, const hm_batch *cond, const hm_batch *a, const hm_batch *b,
                          hm_batch *out) try {
    if (!c || !cond || !a || !b || !out) return HM_ERR_INVALID_ARGUMENT;
    if (hm_status st = check_operands({{cond, 8}, {a, 0}, {b, 0}, {out, 0}}); st) return st;
    if (hm_status st = hm_validate_operation(c, HM_OP_SELECT, nullptr); st) return st;
    const uint32_t L = a->nbits;
    std::vector<uint32_t> need(L);
    if (hm_status st = hm_select_out_bounds(L, cond->bound[0], a->bound, b->bound, need.data()); st)
        return st;
    if (!covers(out, need) || overlaps(out, cond) || overlaps(out, a) || overlaps(out, b))
        return HM_ERR_INVALID_ARGUMENT;
    if (a->n == 0) return HM_OK;
    SelectArgs G{};
    if (hm_status st = plan_select(L, cond->bound[0], a->bound, b->bound, G); st) return st;
    G.cond = batch_arg(cond);
    fill_io(G.io, c, a, b, out);
    return run_circuit(c, G, launch_select);
} HM_ABI_CATCH

hm_status hm_lookup_batch(hm_ctx *c, const hm_batch *a, uint32_t in_bits, const uint8_t *table,
                          uint32_t out_nbytes, hm_batch *out) try {
    if (!c || !a || !table || !out) return HM_ERR_INVALID_ARGUMENT;
    // (a of any width; out_nbytes = 0 asks out for a's width and is refused below)
    if (hm_status st = check_operands({{a, 0}, {out, 8 * out_nbytes}}); st) return st;
    if (in_bits == 0 || in_bits > kLookupMaxIn || in_bits > a->nbits ||
        (out_nbytes != 1 && out_nbytes != 2 && out_nbytes != 4))
        return HM_ERR_INVALID_ARGUMENT;
    if (hm_status st = hm_validate_operation_bits(c, HM_OP_LOOKUP, in_bits, nullptr); st) return st;
    LookupArgs G{};
    lookup_plan::moebius(in_bits, table, out_nbytes, G.coef);
    std::vector<uint32_t> need(out->nbits);
    if (hm_status st = lookup_plan::bounds(in_bits, a->bound, G.coef, out->nbits, need.data()); st)
        return st;
    if (!covers(out, need) || overlaps(out, a)) return HM_ERR_INVALID_ARGUMENT;
    if (a->n == 0) return HM_OK;
    if (hm_status st = plan_lookup(in_bits, a->bound, out_nbytes, G); st) return st;
    G.a = batch_arg(a), G.out = batch_arg(out);
    G.n = a->n, G.status = c->d_status;
    for (uint32_t j = 0; j < out->nbits; ++j) G.ob[j] = out->bound[j];
    return run_circuit(c, G, launch_lookup);
} HM_ABI_CATCH

hm_status hm_shift_batch(hm_ctx *c, hm_op which, const hm_batch *a, const hm_batch *amount,
                         int is_signed, hm_batch *out) try {
    if (!c || !a || !amount || !out || !is_shift_op(which)) return HM_ERR_INVALID_ARGUMENT;
    // (the amount at its own width, of which the low L bits are read)
    if (hm_status st = check_operands({{a, 0}, {amount, amount->nbits}, {out, 0}}); st) return st;
    const uint32_t L = shift_plan::stages(a->nbits);
    if (!L || amount->nbits < L) return HM_ERR_INVALID_ARGUMENT;
    if (hm_status st = hm_validate_operation_bits(c, which, a->nbits, nullptr); st) return st;
    std::vector<uint32_t> need(a->nbits);
    if (hm_status st = shift_plan::bounds(which, a->nbits, a->bound, amount->bound, need.data()); st)
        return st;
    if (!covers(out, need) || overlaps(out, a) || overlaps(out, amount))
        return HM_ERR_INVALID_ARGUMENT;
    if (a->n == 0) return HM_OK;
    ShiftArgs G{};
    if (hm_status st = plan_shift(shift_plan::mode_of(which, is_signed != 0), a->nbits, a->bound,
                                  amount->bound, need.data(), G);
        st)
        return st;
    fill_io(G.io, c, a, amount, out);
    return run_circuit(c, G, launch_shift);
} HM_ABI_CATCH

hm_status hm_bitcount_batch(hm_ctx *c, hm_op which, const hm_batch *a, hm_batch *out) try {
    if (!c || !a || !out || !is_bitcount_op(which)) return HM_ERR_INVALID_ARGUMENT;
    if (hm_status st = check_operands({{a, 0}, {out, kBitCountOut}}); st) return st;
    if (hm_status st = hm_validate_operation_bits(c, which, a->nbits, nullptr); st) return st;
    std::vector<uint32_t> need(kBitCountOut);
    if (hm_status st = bitcount_plan::bounds(which, a->nbits, a->bound, need.data()); st) return st;
    if (!covers(out, need) || overlaps(out, a)) return HM_ERR_INVALID_ARGUMENT;
    if (a->n == 0) return HM_OK;
    BitCountArgs G{};
    if (hm_status st = plan_bitcount(which, a->nbits, a->bound, G); st) return st;
    fill_io(G.io, c, a, nullptr, out);
    return run_circuit(c, G, bitcount_plan::is_run_op(which) ? launch_bitrun : launch_bitcount);
} HM_ABI_CATCH

// What the two array entries check of their batches (check_operands assumes one n and one width):
// each batch on its own, the index's k bits, the elements' width on out (and value), and the value
// counts: n indices, count n elements (or, a shared table, count).
static hm_status check_array(const hm_batch *arr, uint32_t count, const hm_batch *index,
                             const hm_batch *value, const hm_batch *out, uint32_t *k) {
    for (const hm_batch *x : {arr, index, out})
        if (hm_status st = check_batch(x); st) return st;
    if (value)
        if (hm_status st = check_batch(value); st) return st;
    *k = array_plan::index_bits(count);
    if (!*k || index->nbits < *k || out->nbits != arr->nbits) return HM_ERR_INVALID_ARGUMENT;
    const uint64_t n = index->n;
    if (value) { // write: no shared form
        if (value->nbits != arr->nbits || value->n != n || arr->n != count * n || out->n != arr->n)
            return HM_ERR_INVALID_ARGUMENT;
    } else if (out->n != n || (arr->n != count * n && arr->n != count)) {
        return HM_ERR_INVALID_ARGUMENT;
    }
    return HM_OK;
}

hm_status hm_array_read_batch(hm_ctx *c, const hm_batch *arr, uint32_t count,
                              const hm_batch *index, hm_batch *out) try {
    if (!c || !arr || !index || !out) return HM_ERR_INVALID_ARGUMENT;
    uint32_t k;
    if (hm_status st = check_array(arr, count, index, nullptr, out, &k); st) return st;
    if (hm_status st = hm_validate_operation_bits(c, HM_OP_ARRAY_READ, k, nullptr); st) return st;
    std::vector<uint32_t> need(arr->nbits);
    if (hm_status st = array_plan::read_bounds(arr->nbits, arr->bound, count, index->bound,
                                               need.data());
        st)
        return st;
    if (!covers(out, need) || overlaps(out, arr) || overlaps(out, index))
        return HM_ERR_INVALID_ARGUMENT;
    if (index->n == 0) return HM_OK;
    ArrayReadArgs G{};
    const bool shared = arr->n != count * index->n; // (n = 1: the two forms are one)
    if (hm_status st = plan_array_read(arr->nbits, arr->bound, count, index->bound, shared, G); st)
        return st;
    fill_io(G.io, c, arr, index, out);
    G.io.n = index->n;
    return run_circuit(c, G, launch_array_read);
} HM_ABI_CATCH

hm_status hm_array_write_batch(hm_ctx *c, const hm_batch *arr, uint32_t count,
                               const hm_batch *index, const hm_batch *value, hm_batch *out) try {
    if (!c || !arr || !index || !value || !out) return HM_ERR_INVALID_ARGUMENT;
    uint32_t k;
    if (hm_status st = check_array(arr, count, index, value, out, &k); st) return st;
    if (hm_status st = hm_validate_operation_bits(c, HM_OP_ARRAY_WRITE, k, nullptr); st) return st;
    std::vector<uint32_t> need(arr->nbits);
    if (hm_status st = array_plan::write_bounds(arr->nbits, arr->bound, value->bound, count,
                                                index->bound, need.data());
        st)
        return st;
    if (!covers(out, need) || overlaps(out, arr) || overlaps(out, index) || overlaps(out, value))
        return HM_ERR_INVALID_ARGUMENT;
    if (index->n == 0) return HM_OK;
    ArrayWriteArgs G{};
    if (hm_status st = plan_array_write(arr->nbits, arr->bound, value->bound, count, index->bound,
                                        G);
        st)
        return st;
    fill_io(G.io, c, arr, value, out);
    G.io.n = index->n;
    G.idx = batch_arg(index);
    return run_circuit(c, G, launch_array_write);
} HM_ABI_CATCH

// ------------------------------------------------------------------ polynomial primitives
static PolyArgs poly_args(hm_ctx *c, const hm_polys *a, const hm_polys *b, hm_polys *out) {
    PolyArgs P{};
    P.a = a->limbs, P.adeg = a->degree, P.acap = a->cap;
    if (b) P.b = b->limbs, P.bdeg = b->degree, P.bcap = b->cap;
    P.out = out->limbs, P.odeg = out->degree, P.ocap = out->cap;
    P.n = a->n;
    P.status = c->d_status;
    return P;
}

hm_status hm_poly_add_batch(hm_ctx *c, const hm_polys *a, const hm_polys *b, hm_polys *out) try {
    if (!c || !a || !b || !out || a->n != b->n || a->n != out->n) return HM_ERR_INVALID_ARGUMENT;
    if (!a->cap || !b->cap || out->cap < std::max(a->cap, b->cap)) return HM_ERR_INVALID_ARGUMENT;
    DeviceGuard g(c->device);
    return launch_poly_add(poly_args(c, a, b, out), c->stream) ? hip_fail(c, hipGetLastError()) : HM_OK;
} HM_ABI_CATCH

hm_status hm_poly_mul_batch(hm_ctx *c, const hm_polys *a, const hm_polys *b, hm_polys *out) try {
    if (!c || !a || !b || !out || a->n != b->n || a->n != out->n) return HM_ERR_INVALID_ARGUMENT;
    if (!a->cap || !b->cap || out->cap < a->cap + b->cap) return HM_ERR_INVALID_ARGUMENT;
    DeviceGuard g(c->device);
    return launch_poly_mul(poly_args(c, a, b, out), c->stream) ? hip_fail(c, hipGetLastError()) : HM_OK;
} HM_ABI_CATCH

hm_status hm_poly_rem_batch(hm_ctx *c, const hm_polys *a, const uint64_t *s, size_t sn,
                            hm_polys *out) try {
    if (!c || !a || !out || !s || sn == 0 || a->n != out->n) return HM_ERR_INVALID_ARGUMENT;
    if (!a->cap || out->cap < a->cap) return HM_ERR_INVALID_ARGUMENT;
    bool nz = false;
    for (size_t i = 0; i < sn; ++i) nz |= s[i] != 0;
    if (!nz) return HM_ERR_DIVIDE_BY_ZERO;           // polynomial.rs:319-322
    const size_t ds = degree_of(s, sn);
    if (ds == 0) return HM_ERR_DIVISOR_IS_ONE;       // the reference never terminates
    DeviceGuard g(c->device);
    const size_t acap = a->cap, kmax = 64 * acap;
    RemTable T{nullptr, 0, 0, 0};
    if (ds < kmax) {
        // Remainder table (poly_rem_kernel): row j < deg S, bit k = bit j of X^k mod S.  Columns
        // k < deg S are the identity (X^k mod S = X^k), so rows hold only the limbs from
        // l0 = deg S / 64 on; size and build time are bounded by the dividend's capacity whatever
        // the divisor's degree (a divisor above every dividend needs no table: zt = null).
        const size_t l0 = ds / 64, tcols = acap - l0, sl = ds / 64 + 1;
        if ((double)ds * tcols * 8 > 1.0 * (1ull << 30)) return HM_ERR_UNSUPPORTED; // host memory
        const bool cached = c->d_s && c->rem_acap == acap && c->rem_gen == c->generation &&
                            c->rem_key.size() == sl && std::equal(s, s + sl, c->rem_key.begin());
        if (cached) {
            T = RemTable{c->d_s, (uint32_t)ds, (uint32_t)l0, (uint32_t)tcols};
            const int rc = launch_poly_rem(poly_args(c, a, nullptr, out), T, c->stream);
            return rc ? hip_fail(c, hipGetLastError()) : HM_OK;
        }
        // the cache is invalid from here until the new table is complete (a failed rebuild must
        // not leave the old key matching a half-overwritten d_s)
        c->rem_key.clear();
        std::vector<uint64_t> zt(ds * tcols, 0);
        // X^k mod S for the 64 k of column limb l0 + t: unit bits below deg S, then r = X * r mod
        // S; each block of 64 vectors is transposed word by word into the rows
        std::vector<uint64_t> r(sl, 0), blk(64 * sl);
        bool iter = false;
        for (size_t t = 0; t < tcols; ++t) {
            for (size_t u = 0; u < 64; ++u) {
                const size_t k = 64 * (l0 + t) + u;
                uint64_t *v = &blk[u * sl];
                if (k < ds) {
                    std::fill(v, v + sl, 0ull);
                    v[k / 64] = 1ull << (k % 64);
                    continue;
                }
                if (!iter) { // X^ds mod S = S - X^ds
                    std::copy(s, s + sl, r.begin());
                    r[ds / 64] &= ~(1ull << (ds % 64));
                    iter = true;
                } else {
                    uint64_t carry = 0;
                    for (size_t w = 0; w < sl; ++w) {
                        const uint64_t nc = r[w] >> 63;
                        r[w] = (r[w] << 1) | carry;
                        carry = nc;
                    }
                    if ((r[ds / 64] >> (ds % 64)) & 1)
                        for (size_t w = 0; w < sl; ++w) r[w] ^= s[w];
                }
                std::copy(r.begin(), r.end(), v);
            }
            uint64_t m[64];
            for (size_t w = 0; w < sl; ++w) {
                for (size_t u = 0; u < 64; ++u) m[u] = blk[u * sl + w];
                transpose64(m); // m[jb] bit u = bit jb of word w of X^(64(l0+t)+u) mod S
                for (size_t jb = 0; jb < 64 && 64 * w + jb < ds; ++jb) zt[(64 * w + jb) * tcols + t] = m[jb];
            }
        }
        size_t have = c->d_s_limbs * 8;
        HM_HIP(c, grow(c, c->d_s, have, zt.size() * 8));
        c->d_s_limbs = have / 8;
        // d_s is rewritten in place for another divisor: a graph captured with the old table
        // (the cached path has no sync, so it is capturable) must refuse to replay
        ++c->generation;
        HM_HIP(c, hipMemcpyAsync(c->d_s, zt.data(), zt.size() * 8, hipMemcpyHostToDevice, c->stream));
        HM_HIP(c, hipStreamSynchronize(c->stream)); // host buffer is released after return
        T = RemTable{c->d_s, (uint32_t)ds, (uint32_t)l0, (uint32_t)tcols};
        c->rem_key.assign(s, s + sl), c->rem_acap = acap, c->rem_gen = c->generation;
    }
    const int rc = launch_poly_rem(poly_args(c, a, nullptr, out), T, c->stream);
    return rc ? hip_fail(c, hipGetLastError()) : HM_OK;
} HM_ABI_CATCH

hm_status hm_ctx_synchronize(hm_ctx *c) try {
    if (!c) return HM_ERR_INVALID_ARGUMENT;
    DeviceGuard g(c->device);
    HM_HIP(c, hipStreamSynchronize(c->stream));
    int st = 0;
    HM_HIP(c, hipMemcpy(&st, c->d_status, sizeof(int), hipMemcpyDeviceToHost));
    if (st) HM_HIP(c, hipMemset(c->d_status, 0, sizeof(int)));
    if (c->last_hip != hipSuccess) {
        c->last_hip = hipSuccess;
        return HM_ERR_HIP;
    }
    return (hm_status)st;
} HM_ABI_CATCH

int32_t hm_ctx_last_hip_error(const hm_ctx *c) { return c ? (int32_t)c->last_hip : 0; }

} // extern "C"
