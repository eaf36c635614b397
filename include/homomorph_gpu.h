/*
 * homomorph_gpu.h — C ABI of the MI355X (gfx950) GF(2)[X] homomorphic engine.
 *
 * This is the drop-in boundary for mathisbot/homomorph-rust's data-parallel hot path.  Each entry
 * point names the reference item it replaces (file:line, paths relative to the reference crate).
 * The reference has no batch API; every batch entry applies the reference's per-value operation
 * independently to n values (one `Ciphered<T>` = nbits ciphertext bits per value).
 *
 * Conventions
 *  - Plain C: pointers + sizes, no C++ types, no exceptions cross this boundary.  Every function
 *    returns hm_status; HM_OK == 0.
 *  - Device buffers are caller-owned device pointers (hipMalloc'd or a torch tensor's data_ptr);
 *    the library never frees caller memory.  Launches are asynchronous on the context's stream;
 *    no entry below synchronises unless its comment says so.
 *  - Polynomial layout (GF(2)[X], src/polynomial.rs:23-26): coefficient of X^k is bit k%64 of
 *    little-endian u64 limb k/64 (the code's layout, polynomial.rs:142-150, :168-173 — the doc
 *    comment at :16-21 describing reversed bits does not match the code).  Limbs above the degree
 *    are zero.  Degrees are exact; the null polynomial has degree 0 (polynomial.rs:126-137).
 *  - Batch layout (hm_batch): value e, bit i occupies cap[i] = bound[i]/64 + 1 limbs at limb offset
 *    e*stride + off[i] (off = exclusive prefix sum of cap, stride = sum(cap)); its exact degree is
 *    degree[e*nbits + i].  bound[i] is a static degree bound for bit position i (a fresh ciphertext
 *    has bound d+dp); outputs are sized with hm_*_out_bounds.  Bit i is bit i of the bincode fixint
 *    little-endian image of the value (src/cipher.rs:6-13, :175-191).
 *  - Thread-safety: calls on one context are serialised by the caller; contexts on different
 *    devices are independent (the reference's Context is a plain value, src/context.rs:300-306).
 */
#ifndef HOMOMORPH_GPU_H
#define HOMOMORPH_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HM_ABI_VERSION 12 /* 4: kernel timing by device stamps (HM_TIME_*), hm_ctx_last_hip_error;
                            5: hm_ctx_clear_kernel_timing, hm_ctx_set_mul_scratch;
                            6: HM_OP_SUB .. HM_OP_GE, hm_sub_batch, hm_compare_batch, their bounds,
                               hm_validate_operation_bits;
                            7: HM_OP_SELECT, HM_OP_MIN, HM_OP_MAX, hm_select_batch,
                               hm_minmax_batch, their bounds;
                            8: HM_OP_LOOKUP, hm_lookup_batch, hm_lookup_out_bounds;
                            9: HM_OP_SHL .. HM_OP_ROTR, hm_shift_batch, hm_shift_out_bounds;
                            10: HM_OP_COUNT_ONES .. HM_OP_TRAILING_ONES, hm_bitcount_batch,
                               hm_bitcount_out_bounds;
                            11: HM_OP_ARRAY_READ, HM_OP_ARRAY_WRITE, hm_array_read_batch,
                               hm_array_write_batch, their bounds;
                            12: hm_ctx_set_mul_chunk */
#define HM_MAX_BITS 128 /* u128 is the widest type with impls (src/impls/numbers/uint.rs:58) */

typedef enum hm_status {
    HM_OK = 0,
    /* OperationError::InvalidParameters (src/operations.rs:11-18) */
    HM_ERR_INVALID_PARAMETERS = 1,
    /* ContextCryptoError::SecretKeyUnset / PublicKeyUnset (src/context.rs:41-46) */
    HM_ERR_SECRET_KEY_UNSET = 2,
    HM_ERR_PUBLIC_KEY_UNSET = 3,
    /* Polynomial::rem panics "attempt to divide by zero" (src/polynomial.rs:319-322) */
    HM_ERR_DIVIDE_BY_ZERO = 4,
    /* Polynomial::rem by the constant 1 never terminates in the reference (:330-343) */
    HM_ERR_DIVISOR_IS_ONE = 5,
    /* an output would exceed the capacity its bound gives (device-side check) */
    HM_ERR_CAPACITY = 6,
    /* sizes beyond what this build's kernels handle */
    HM_ERR_UNSUPPORTED = 7,
    HM_ERR_HIP = 8,
    HM_ERR_INVALID_ARGUMENT = 9,
    /* CipherError::InvalidCipheredLength (src/cipher.rs:18-24, :218-220) */
    HM_ERR_INVALID_CIPHERED_LENGTH = 10,
    /* an input polynomial's degree word disagrees with its limbs (device-side check) */
    HM_ERR_BAD_INPUT = 11,
    /* CipherError::Randomness (src/cipher.rs:18-24): the OS random source failed */
    HM_ERR_RANDOMNESS = 12,
    /* a host-side allocation failed (std::bad_alloc inside the library, caught at the entry) */
    HM_ERR_OUT_OF_MEMORY = 13,
    /* any other C++ exception raised inside the library, caught at the entry */
    HM_ERR_INTERNAL = 14,
} hm_status;

/* Operation marker types and their OperationRequirement::MIN_D_OVER_DELTA
 * (src/impls/numbers.rs:9-50). */
typedef enum hm_op {
    HM_OP_AND = 0,            /* HomomorphicAndGate,        min d/delta 2  */
    HM_OP_OR = 1,             /* HomomorphicOrGate,         min d/delta 2  */
    HM_OP_XOR = 2,            /* HomomorphicXorGate,        min d/delta 1  */
    HM_OP_NOT = 3,            /* HomomorphicNotGate,        min d/delta 1  */
    HM_OP_ADD = 4,            /* HomomorphicAddition,       min d/delta 21 */
    HM_OP_MUL = 5,            /* HomomorphicMultiplication, min d/delta 64 (unsigned types) */
    HM_OP_MUL_SIGNED = 6,     /* HomomorphicMultiplication on i8..i128 (common.rs:115-163) */
    /* The engine's own operations (the reference defines no circuit for them): one ripple-borrow
     * chain w_{i+1} = a_i b_i + b_i + (a_i + b_i + 1) w_i, w_0 = 0.  Their requirement depends on
     * the width n of the type: min d/delta = 2m + 1 with m the circuit's degree in fresh input
     * bits, m = n for SUB / EQ / NE and m = n + 1 for the orderings (hm_validate_operation_bits). */
    HM_OP_SUB = 7,            /* HomomorphicSubtraction: a - b (wrapping), signed or unsigned */
    HM_OP_EQ = 8,             /* HomomorphicEqual            a == b */
    HM_OP_NE = 9,             /* HomomorphicNotEqual         a != b */
    HM_OP_LT = 10,            /* HomomorphicLessThan         a <  b */
    HM_OP_LE = 11,            /* HomomorphicLessEqual        a <= b */
    HM_OP_GT = 12,            /* HomomorphicGreaterThan      a >  b */
    HM_OP_GE = 13,            /* HomomorphicGreaterEqual     a >= b */
    /* Consumers of a comparison's Ciphered<bool>, on the same rule 2m + 1.
     * SELECT: out_i = b_i + c (a_i + b_i), m = 2, min d/delta 5 at any width.  As the reference's
     * gate requirements do, that number covers FRESH operands, the condition included.  A
     * condition that came out of a comparison carries that comparison's depth: for c = (a < b)
     * on fresh n-bit values the whole circuit is HM_OP_MIN's, and the caller checks that
     * requirement (hm_validate_operation_bits(HM_OP_MIN, n)).
     * MIN / MAX: the borrow out of the top bit times a_i + b_i, m = n + 2, min d/delta 2n + 5
     * (u8 21, u16 37, u32 69, u64 133): width dependent, like HM_OP_SUB .. HM_OP_GE. */
    HM_OP_SELECT = 14,        /* HomomorphicSelect           cond ? a : b,  min d/delta 5 */
    HM_OP_MIN = 15,           /* HomomorphicMin              min(a, b) */
    HM_OP_MAX = 16,           /* HomomorphicMax              max(a, b) */
    /* Any function of the n <= 8 low bits of a value, given as a plaintext table (hm_lookup_batch):
     * a multilinear polynomial of degree at most n in those bits, so m = n and min d/delta 2n + 1
     * (a byte 17, a bool 3): width dependent (hm_validate_operation_bits), for fresh index bits. */
    HM_OP_LOOKUP = 17,        /* HomomorphicLookup           table[a] */
    /* Shifts and rotates of an n-bit value, n a power of two in 2..128, by an ENCRYPTED amount
     * (hm_shift_batch): a barrel shifter of log2 n stages, each a select between the value and its
     * copy moved by 2^t on amount bit t, so m = log2 n + 1 and min d/delta 2 log2 n + 3 (u8 9,
     * u16 11, u32 13, u64 15, u128 17): width dependent (hm_validate_operation_bits), for fresh
     * operands.  (A shift by a plaintext amount only renumbers ciphertext bits: no kernel.) */
    HM_OP_SHL = 18,           /* HomomorphicShiftLeft        a << (s mod n) */
    HM_OP_SHR = 19,           /* HomomorphicShiftRight       a >> (s mod n), logical or arithmetic */
    HM_OP_ROTL = 20,          /* HomomorphicRotateLeft       a.rotate_left(s mod n) */
    HM_OP_ROTR = 21,          /* HomomorphicRotateRight      a.rotate_right(s mod n) */
    /* Bit counts of an n-bit value, n in 1..128, as a Ciphered<u8> (hm_bitcount_batch), on the
     * literals u_i = x_i (the "ones" ops) or x_i + 1 (the "zeros" ops).  A count's bit k is the
     * elementary symmetric polynomial e_{2^k} of the literals, so m = 2^floor(log2 n); a run's
     * bit k is a sum of prefix products of up to n literals, so m = n.  min d/delta = 2m + 1: for
     * u8, u16, u32, u64 both kinds need 17, 33, 65, 129; at n = 24 a count needs 33 and a run 49.
     * Width dependent (hm_validate_operation_bits), for fresh operands. */
    HM_OP_COUNT_ONES = 22,     /* HomomorphicCountOnes        a.count_ones() */
    HM_OP_COUNT_ZEROS = 23,    /* HomomorphicCountZeros       a.count_zeros() */
    HM_OP_LEADING_ZEROS = 24,  /* HomomorphicLeadingZeros     a.leading_zeros() */
    HM_OP_LEADING_ONES = 25,   /* HomomorphicLeadingOnes      a.leading_ones() */
    HM_OP_TRAILING_ZEROS = 26, /* HomomorphicTrailingZeros    a.trailing_zeros() */
    HM_OP_TRAILING_ONES = 27,  /* HomomorphicTrailingOnes     a.trailing_ones() */
    /* Oblivious array read and write by an ENCRYPTED index (hm_array_read_batch,
     * hm_array_write_batch) over an array of count elements, count in 2..256, k = ceil(log2 count)
     * index bits.  Both multiply an indicator of k literals by one element or value bit, so
     * m = k + 1 and min d/delta 2k + 3 (count 2: 5, 4: 7, 16: 11, 256: 19).  Width dependent
     * (hm_validate_operation_bits), and the width is k, the number of index bits, in 1..8, as for
     * HM_OP_LOOKUP; for fresh operands. */
    HM_OP_ARRAY_READ = 28,     /* HomomorphicArrayRead        arr[i] */
    HM_OP_ARRAY_WRITE = 29,    /* HomomorphicArrayWrite       arr[i] = x */
} hm_op;

typedef struct hm_ctx hm_ctx;

/* A batch of n values of nbits ciphertext bits each, in device memory (layout above). */
typedef struct hm_batch {
    uint64_t *limbs;        /* device, n*stride limbs */
    uint32_t *degree;       /* device, n*nbits exact degrees */
    const uint32_t *bound;  /* HOST, nbits per-bit-position degree bounds */
    uint32_t nbits;         /* 1..HM_MAX_BITS */
    uint64_t n;             /* number of values */
} hm_batch;

/* A batch of n independent polynomials, each with cap limbs, in device memory. */
typedef struct hm_polys {
    uint64_t *limbs;        /* device, n*cap limbs */
    uint32_t *degree;       /* device, n exact degrees */
    uint32_t cap;           /* limbs per polynomial */
    uint64_t n;
} hm_polys;

/* ---------------- library / context ---------------- */
/* Text of a status code; any int is accepted ("unknown status" outside hm_status). */
const char *hm_status_string(int s);
uint32_t hm_abi_version(void);

/* Context::new(Parameters::new(d, dp, delta, tau)) — src/context.rs:345-351 with the asserts of
 * Parameters::new (:87-94: all > 0, delta < d) reported as HM_ERR_INVALID_PARAMETERS.
 * device: HIP device ordinal; the context creates its own non-blocking stream. */
hm_status hm_ctx_create(uint16_t d, uint16_t dp, uint16_t delta, uint16_t tau, int device,
                        hm_ctx **out);
/* Drop: device copies of the secret key (and tables derived from it) are zeroed before release,
 * mirroring SecretKey's Drop (src/context.rs:197-206). */
void hm_ctx_destroy(hm_ctx *ctx);
/* Device buffers the kernels read (workspaces, key tables, decrypt tables, mask buffers) are
 * never freed while the context lives, because a HIP graph captured over the engine's launches
 * holds their raw pointers.  When one must be replaced (it grows, or a new key replaces its
 * contents) the old one is retired -- zeroed first if it holds secret-derived data -- and the
 * context generation advances.  A captured graph is valid only while the generation it was
 * captured at is current; hm_ctx_trim frees the retired buffers (no graph may use them after). */
uint64_t hm_ctx_generation(const hm_ctx *ctx);
hm_status hm_ctx_trim(hm_ctx *ctx);
/* Launch on a caller stream (hipStream_t passed as void*; NULL = the default null stream, as in
 * HIP) instead of the context's own non-blocking stream.  Use it to order the engine's launches
 * with the caller's copies, e.g. torch.cuda.current_stream().cuda_stream. */
hm_status hm_ctx_set_stream(hm_ctx *ctx, void *hip_stream);
void *hm_ctx_stream(const hm_ctx *ctx);
/* Parameters getters (src/context.rs:96-118). */
hm_status hm_ctx_parameters(const hm_ctx *ctx, uint16_t *d, uint16_t *dp, uint16_t *delta,
                            uint16_t *tau);

/* Context::set_secret_key(SecretKey::from_bytes) — src/context.rs:568-571 + :153-155.  limbs: host
 * little-endian u64 limbs of S (the bytes of SecretKey::to_bytes).  Clears the public key, as the
 * reference does. */
hm_status hm_ctx_set_secret_key(hm_ctx *ctx, const uint64_t *limbs, size_t nlimbs);
/* Context::set_public_key(PublicKey::from_bytes) — src/context.rs:593-595 + :239-245.  limbs: host,
 * tau polynomials of limbs_per_poly limbs each (row-major). */
hm_status hm_ctx_set_public_key(hm_ctx *ctx, const uint64_t *limbs, uint32_t tau,
                                uint32_t limbs_per_poly);
/* Context::generate_secret_key / generate_public_key — src/context.rs:421-454 (keygen shape
 * S = random(d), T_i = S*Q_i + X*R_i, :160-162 and :249-261).  As in the reference, every key
 * polynomial is drawn from getrandom(2) (src/polynomial.rs:73-96) and encryption masks from a
 * CSPRNG (a device ChaCha20 stream keyed with 32 getrandom bytes at context creation).
 * hm_ctx_seed_rng is a TEST hook: it switches key generation to a SplitMix64 stream and the mask
 * stream to a ChaCha20 key derived from the seed, so parity tests can reproduce both sides.
 * generate_secret_key clears the public key (:421-424); generate_public_key needs the secret key
 * (HM_ERR_SECRET_KEY_UNSET otherwise, :444-454).  Public-key rows are as wide as the widest
 * T_i (deg S + dp for a loaded secret key of any degree). */
hm_status hm_ctx_seed_rng(hm_ctx *ctx, uint64_t seed);
hm_status hm_ctx_generate_secret_key(hm_ctx *ctx);
hm_status hm_ctx_generate_public_key(hm_ctx *ctx);
/* Key export (SecretKey::to_bytes :192-194 / PublicKey::to_bytes :291-297) into host buffers. */
hm_status hm_ctx_get_secret_key(const hm_ctx *ctx, uint64_t *limbs, size_t cap, size_t *nlimbs);
hm_status hm_ctx_get_public_key(const hm_ctx *ctx, uint64_t *limbs, size_t cap, uint32_t *tau,
                                uint32_t *limbs_per_poly);

/* Multiplier strategy (no effect on results: every product is exact).  A carry product of the
 * carry-save circuit whose shorter operand has at least karatsuba_min_words 32-bit words runs as
 * a Karatsuba recursion down to leaves of at most karatsuba_leaf_words
 * words (rounded to a multiple of 32, at most 512); smaller products run as schoolbook tiles.
 * karatsuba_min_words = 0 disables it.  Defaults: 256 and 256 (measured best for the u32 multiply
 * prefixes at d = d' = 128 once the leaves run on the matrix cores; 192 and 192 at d = d' = 256). */
hm_status hm_ctx_set_mul_options(hm_ctx *ctx, uint32_t karatsuba_min_words,
                                 uint32_t karatsuba_leaf_words);
/* Karatsuba scratch (no effect on results).  A Karatsuba product's recursion runs breadth-first
 * (all its leaves in one launch, then the recombinations bottom-up), so every node's buffers are
 * alive at once and the scratch grows as n^1.585.  A product whose recursion needs more than
 * words_per_value 32-bit words of scratch per value is planned one subtree at a time instead: the
 * root's operand sums and child products first, then each child's own recursion (recursively,
 * reusing the scratch above the root's), then the root's recombination.  Default 2e8 words (every
 * product up to the u32 multiply's K = 20 prefix runs whole; K = 21..24 need the split).  At most
 * 2^27 + 2^26 words (the plan's views hold 28-bit offsets); at least 1. */
hm_status hm_ctx_set_mul_scratch(hm_ctx *ctx, uint64_t words_per_value);
/* Chunk limit of the multiplier (no effect on results).  hm_ctx_set_mul_chunk is a TEST hook, like
 * hm_ctx_seed_rng.  A multiply runs its n values in chunks that share one workspace: by default a
 * chunk holds as many values as fit half of the free device memory (at least 2^28 bytes), so on an
 * otherwise empty device every batch is one chunk, and how many chunks a batch takes depends on
 * what else runs on the card.  max_values > 0 caps the chunk, chunk = min(n, budget / per_value,
 * max_values), so that tests run the chunk loop at sizes of their choosing; 0 (the default) is no
 * cap.  Cached plans do not depend on it.  The workspace is sized for the chunk (it never shrinks
 * while the context lives, and is replaced as every other workspace is: hm_ctx_generation). */
hm_status hm_ctx_set_mul_chunk(hm_ctx *ctx, uint64_t max_values);

/* Where the multiplier's products run (no effect on results: every product is exact): as {0,1}
 * Toeplitz GEMMs on the fp4 matrix cores (MFMA, reduced mod 2) or as VALU products.  The choice
 * covers every product kind of the carry-save plan: the Karatsuba leaf products, the schoolbook
 * carry products p_t * x_t, and the partial products a_j * b_k of fresh operands (products whose
 * shorter operand is below 4 words, and the signed circuit's flipped partial products, stay on
 * the VALU either way).  AUTO = MFMA on a device with the gfx950 fp4 MFMA, VALU elsewhere;
 * MFMA on a device without it is HM_ERR_UNSUPPORTED. */
#define HM_MUL_PRODUCTS_AUTO 0u
#define HM_MUL_PRODUCTS_MFMA 1u
#define HM_MUL_PRODUCTS_VALU 2u
hm_status hm_ctx_set_mul_products(hm_ctx *ctx, uint32_t products);

/* Adder strategy (no effect on results: both chains are exact).  The carry chain
 * carry' = ab_i ^ P_i * carry (src/impls/numbers/common.rs:37-56) runs its products either on the
 * matrix cores (a {0,1} Toeplitz product on fp4 MFMA, reduced mod 2; needs P_i within 49 words,
 * i.e. d + dp <= 512 for u32) or as scalar-decided VALU XORs.  AUTO picks the MFMA chain when it
 * applies (and the device has the gfx950 fp4 MFMA); MFMA on a plan or device it cannot run
 * returns HM_ERR_UNSUPPORTED at hm_add_batch. */
#define HM_ADD_CHAIN_AUTO 0u
#define HM_ADD_CHAIN_MFMA 1u
#define HM_ADD_CHAIN_VALU 2u
hm_status hm_ctx_set_add_options(hm_ctx *ctx, uint32_t chain);

/* Adder pipelining (no effect on results; off by default: measured no faster on configs[1],
 * DESIGN.md s4.1).  When enabled, an MFMA-chain add of at least 2048 values runs as two halves,
 * the second half's carry-independent prep on an auxiliary stream beside the first half's carry
 * chain, joined back into the context stream by events (a graph captured on the context stream
 * holds both branches).  Not used while kernel timing is on. */
hm_status hm_ctx_set_add_pipeline(hm_ctx *ctx, int enable);

/* Kernel timing (measurement only; no effect on results).  hm_ctx_set_kernel_timing(ctx, k)
 * times kernel k from now on (HM_TIME_OFF stops; setting resets the record and synchronizes the
 * stream): every launch of it made -- or captured into a graph -- while timing is on takes its
 * own record slot (up to 128), in which the kernel's waves stamp the device wall clock at their
 * start and end (a minimum over starts, a maximum over ends).  A captured launch keeps its slot
 * across replays and nothing clears it in between: the stamps are valid for ONE replay of the
 * graph (R replays make each slot span from the first replay's start to the last one's end).  So
 * enable, capture a K-step graph, replay it once, read: K launches (as the bench times it).
 * hm_ctx_clear_kernel_timing synchronizes the stream and clears the stamps of every slot while
 * keeping the slots (and the kernel timed): a graph captured earlier can then be replayed again
 * and read for that one replay.
 * hm_ctx_kernel_timing synchronizes the stream and returns the summed duration (earliest wave
 * start to latest wave end, per slot) of the launches recorded and their number.
 * HM_TIME_ADD_CHAIN = 1 (hm_add_batch's carry chain, the dominant kernel of the add),
 * HM_TIME_ENCRYPT: hm_encrypt_batch's encryption kernel (not the mask draw), HM_TIME_DECRYPT:
 * hm_decrypt_batch's kernel. */
enum { HM_TIME_OFF = 0, HM_TIME_ADD_CHAIN = 1, HM_TIME_ENCRYPT = 2, HM_TIME_DECRYPT = 3 };
hm_status hm_ctx_set_kernel_timing(hm_ctx *ctx, int kernel);
hm_status hm_ctx_clear_kernel_timing(hm_ctx *ctx);
hm_status hm_ctx_kernel_timing(hm_ctx *ctx, double *total_ms, uint32_t *launches);

/* Context::validate_operation (src/context.rs:310-323): HM_OK or HM_ERR_INVALID_PARAMETERS with
 * the OperationError payload written to *required_min_d_over_delta (may be NULL). */
hm_status hm_validate_operation(const hm_ctx *ctx, hm_op op, uint16_t *required_min_d_over_delta);
/* The same for an operation on nbits-bit values.  HM_OP_AND .. HM_OP_MUL_SIGNED: exactly
 * hm_validate_operation (nbits is not looked at).  HM_OP_SUB .. HM_OP_GE: the requirement
 * 2m + 1 above (u32: 65 for SUB / EQ / NE, 67 for the orderings), which gives m (delta + 1) < d,
 * so results on fresh inputs decrypt exactly; nbits outside 1..HM_MAX_BITS is
 * HM_ERR_INVALID_ARGUMENT.  HM_OP_MIN / HM_OP_MAX likewise: 2 nbits + 5 (u32: 69).
 * HM_OP_LOOKUP: 2 nbits + 1 with nbits the index bits (hm_lookup_batch itself takes 1..8).
 * HM_OP_SHL .. HM_OP_ROTR: 2 log2(nbits) + 3 with nbits the width of the shifted type (u32: 13);
 * a width that is not a power of two in 2..HM_MAX_BITS is HM_ERR_INVALID_ARGUMENT.
 * HM_OP_COUNT_ONES, HM_OP_COUNT_ZEROS: 2 * 2^floor(log2 nbits) + 1; HM_OP_LEADING_ZEROS ..
 * HM_OP_TRAILING_ONES: 2 nbits + 1 (u32: 65 for both kinds; nbits = 24: 33 and 49).
 * HM_OP_SELECT has no width: both entries return 5.  hm_validate_operation itself has no width:
 * it returns HM_ERR_INVALID_ARGUMENT for HM_OP_SUB .. HM_OP_GE, HM_OP_MIN, HM_OP_MAX,
 * HM_OP_LOOKUP, HM_OP_SHL .. HM_OP_ROTR and HM_OP_COUNT_ONES .. HM_OP_TRAILING_ONES. */
hm_status hm_validate_operation_bits(const hm_ctx *ctx, hm_op op, uint32_t nbits,
                                     uint16_t *required_min_d_over_delta);

/* Static degree bounds (host only, no device work).  fresh bound = max(d + dp, max deg T_i):
 * a subset sum of public-key rows plus the plaintext bit (cipher.rs:99-115). */
uint32_t hm_fresh_bound(const hm_ctx *ctx);
/* Mask bytes per ciphertext bit: ceil(tau/8) with tau = the number of rows of the LOADED public
 * key (CipheredBit::cipher takes tau = pk.len(), cipher.rs:101-103; a loaded key may differ from
 * Parameters::tau, context.rs:585-593).  0 when no public key is set. */
uint32_t hm_ctx_mask_bytes(const hm_ctx *ctx);
/* Output bounds of the ripple-carry adder (common.rs:37-56) for input bounds a,b (nbits each). */
hm_status hm_add_out_bounds(uint32_t nbits, const uint32_t *a_bound, const uint32_t *b_bound,
                            uint32_t *out_bound);
/* Output bounds of the carry-save multiplier (common.rs:66-105 / :115-155). */
hm_status hm_mul_out_bounds(uint32_t nbits, const uint32_t *a_bound, const uint32_t *b_bound,
                            int is_signed, uint32_t *out_bound);
/* Cost model of the low k output bits of the nbits-bit carry-save multiplier (host only, no device
 * work): the symbolic run of common.rs:66-105 over static degree bounds, exactly as
 * hm_mul_low_batch plans it but without the engine's size limits, so the full u32 circuit (which
 * no engine can run: SURVEY.md s0.6) can be priced.  word_pairs: 32x32-bit carry-less word
 * products over all carries p_t * x_t; out_bytes: the k output bits at their capacities;
 * max_degree: the largest degree bound of any polynomial the circuit builds.  Outputs may be
 * NULL. */
hm_status hm_mul_cost(uint32_t nbits, uint32_t k, const uint32_t *a_bound, const uint32_t *b_bound,
                      int is_signed, double *word_pairs, double *out_bytes, double *max_degree);
/* The same carry products as the context's plan for hm_mul_low_batch / hm_mul_batch (k = nbits)
 * runs them, with the context's strategy options (hm_ctx_set_mul_options, _products): a schoolbook
 * product counts its word pairs at the static bounds (as hm_mul_cost does), a Karatsuba product its
 * leaf products' word pairs.  No kernel runs, but the plan is built and cached as the multiply
 * would: its task tables are allocated in device memory and copied (synchronously) on the
 * context's stream, so this call is not free and must not be made while that stream is being
 * captured into a graph; HM_ERR_UNSUPPORTED beyond the engine's limits.  The bench's
 * multiply rooflines use it as the issued work. */
hm_status hm_mul_plan_work(hm_ctx *ctx, uint32_t nbits, uint32_t k, const uint32_t *a_bound,
                           const uint32_t *b_bound, int is_signed, double *word_pairs);
/* Output bounds of a gate (common.rs:5-35). */
hm_status hm_gate_out_bounds(hm_op gate, uint32_t nbits, const uint32_t *a_bound,
                             const uint32_t *b_bound, uint32_t *out_bound);
/* Output bounds of the ripple-borrow subtraction: with wb_0 = 0 and
 * wb_{i+1} = max(a_i + b_i, max(a_i, b_i) + wb_i), bit 0 has bound max(a_0, b_0) and bit i
 * max(a_i, b_i, wb_i).  (u32 at d + dp = 256: 2144 limbs per value.) */
hm_status hm_sub_out_bounds(uint32_t nbits, const uint32_t *a_bound, const uint32_t *b_bound,
                            uint32_t *out_bound);
/* Output bounds of a comparison cmp = HM_OP_EQ .. HM_OP_GE (anything else is
 * HM_ERR_INVALID_ARGUMENT) of nbits-bit values: a Ciphered<bool> of 8 ciphertext bits (bincode
 * stores a bool as one byte).  out_bound[0] = wb_nbits for the orderings and sum max(a_i, b_i) for
 * EQ / NE; out_bound[1..7] = 0 (null polynomials). */
hm_status hm_compare_out_bounds(hm_op cmp, uint32_t nbits, const uint32_t *a_bound,
                                const uint32_t *b_bound, uint32_t out_bound[8]);
/* Output bounds of select(cond, a, b): out_bound[i] = cond_bound0 + max(a_i, b_i), with
 * cond_bound0 the bound of the condition's bit 0 (its bits 1..7 are not read). */
hm_status hm_select_out_bounds(uint32_t nbits, uint32_t cond_bound0, const uint32_t *a_bound,
                               const uint32_t *b_bound, uint32_t *out_bound);
/* Output bounds of min(a, b) and of max(a, b): out_bound[i] = wb_nbits + max(a_i, b_i) with the
 * borrow recurrence of hm_sub_out_bounds.  (u32 at d + dp = 256: every bit 8704, 4384 limbs per
 * value.)  Both entries: nbits outside 1..HM_MAX_BITS is HM_ERR_INVALID_ARGUMENT, a bound
 * beyond the engine's degree range HM_ERR_UNSUPPORTED. */
hm_status hm_minmax_out_bounds(uint32_t nbits, const uint32_t *a_bound, const uint32_t *b_bound,
                               uint32_t *out_bound);
/* Output bounds of hm_lookup_batch(a, table): they depend on the table, which is public.  With
 * c_j the algebraic normal form of output bit j (see hm_lookup_batch), out_bound[j] = the largest
 * sum of a_bound[i] over i in S among the sets S of c_j, and 0 when c_j is empty or holds only the
 * empty set: the identity table gives the input's own bounds, a random byte table at one bound D
 * gives 8 D where the top monomial is present and 7 D otherwise.  a_bound: in_bits entries; table:
 * 2^in_bits entries of out_nbytes little-endian bytes; writes 8 out_nbytes bounds.  in_bits
 * outside 1..8, out_nbytes outside {1, 2, 4} or a null pointer is HM_ERR_INVALID_ARGUMENT, a
 * bound beyond the engine's degree range HM_ERR_UNSUPPORTED. */
hm_status hm_lookup_out_bounds(uint32_t in_bits, const uint32_t *a_bound, const uint8_t *table,
                               uint32_t out_nbytes, uint32_t *out_bound);
/* Output bounds of hm_shift_batch(which, a, amount), which = HM_OP_SHL .. HM_OP_ROTR (anything
 * else is HM_ERR_INVALID_ARGUMENT) on nbits-bit values, nbits a power of two in 2..128 (anything
 * else is HM_ERR_INVALID_ARGUMENT, as is a null pointer).  a_bound: nbits entries; s_bound: the
 * log2(nbits) bounds of the amount's low bits.  With S the sum of s_bound, out_bound[j] = S + the
 * widest a_bound[i] among the bits that can reach bit j: i <= j for HM_OP_SHL, i >= j for
 * HM_OP_SHR (logical and arithmetic alike), every i for the rotates.  (u32 at d + dp = 256, a u8
 * or u32 amount: every bit 1536, 800 limbs per value.)  A bound beyond the engine's degree range
 * is HM_ERR_UNSUPPORTED. */
hm_status hm_shift_out_bounds(hm_op which, uint32_t nbits, const uint32_t *a_bound,
                              const uint32_t *s_bound, uint32_t *out_bound);
/* Output bounds of hm_bitcount_batch(which, a), which = HM_OP_COUNT_ONES .. HM_OP_TRAILING_ONES
 * (anything else is HM_ERR_INVALID_ARGUMENT) on nbits-bit values, nbits in 1..128 (anything else
 * is HM_ERR_INVALID_ARGUMENT, as is a null pointer).  a_bound: nbits entries; writes the 8 bounds
 * of a Ciphered<u8>.  Counts: out_bound[k] = the sum of the 2^k largest a_bound.  Runs: the sum of
 * a_bound over the first M literals in the run's order (leading: from bit nbits - 1 down,
 * trailing: from bit 0 up), M the largest multiple of 2^k that is <= nbits.  Bits with
 * 2^k > nbits: 0 (null polynomials).  The zeros ops have the bounds of the ones ops.  (u32 at
 * d + dp = 256: a count 256, 512, 1024, 2048, 4096, 8192, 0, 0, 260 limbs per value; a run 8192
 * in bits 0..5, 776 limbs per value.)  A bound beyond the engine's degree range is
 * HM_ERR_UNSUPPORTED. */
hm_status hm_bitcount_out_bounds(hm_op which, uint32_t nbits, const uint32_t *a_bound,
                                 uint32_t out_bound[8]);
/* Output bounds of hm_array_read_batch(arr, count, index) on nbits-bit elements (nbits in 1..128),
 * count in 2..256 (anything else is HM_ERR_INVALID_ARGUMENT, as is a null pointer).  arr_bound:
 * nbits entries, shared by all elements; s_bound: the k = ceil(log2 count) bounds of the index's
 * low bits.  With S the sum of s_bound, out_bound[j] = S + arr_bound[j].  (u8 x 16 at d + dp = 256,
 * a u8 index: every bit 1280, 168 limbs per value.)  A bound beyond the engine's degree range is
 * HM_ERR_UNSUPPORTED. */
hm_status hm_array_read_out_bounds(uint32_t nbits, const uint32_t *arr_bound, uint32_t count,
                                   const uint32_t *s_bound, uint32_t *out_bound);
/* Output bounds of hm_array_write_batch(arr, count, index, value): as above with x_bound the nbits
 * bounds of the value written; out_bound[j] = S + max(arr_bound[j], x_bound[j]), shared by all
 * elements of the output array. */
hm_status hm_array_write_out_bounds(uint32_t nbits, const uint32_t *arr_bound,
                                    const uint32_t *x_bound, uint32_t count,
                                    const uint32_t *s_bound, uint32_t *out_bound);
/* stride (limbs per value) of a batch with these bounds */
uint64_t hm_batch_stride(uint32_t nbits, const uint32_t *bound);

/* ---------------- cipher (src/cipher.rs) ---------------- */
/* n bytes of the context's mask CSPRNG (device ChaCha20, see hm_ctx_seed_rng) into device
 * memory.  Every call -- and every replay of a graph that captured one -- draws fresh bytes. */
hm_status hm_random_bytes(hm_ctx *ctx, uint8_t *dev_dst, size_t nbytes);
/* Context::encrypt over a batch — Ciphered::try_cipher (cipher.rs:175-191) and
 * CipheredBit::cipher (:99-115).  data: device, n*nbytes plaintext bytes (the bincode fixint LE
 * image of each value).  masks: NULL = the engine draws them from its CSPRNG, as
 * CipheredBit::part (:92-97) draws from getrandom (the default); or device,
 * n*(8*nbytes)*M bytes with M = hm_ctx_mask_bytes(ctx): bit k of value e uses the M bytes at
 * ((e*8*nbytes)+k)*M, mask bit i = byte[i/8] >> (i%8) & 1 — exactly the bytes part() draws (the
 * test contract).  out: nbits = 8*nbytes, every bound >= hm_fresh_bound.  Requires the public
 * key. */
hm_status hm_encrypt_batch(hm_ctx *ctx, const uint8_t *data, uint32_t nbytes,
                           const uint8_t *masks, hm_batch *out);
/* Context::decrypt over a batch — Ciphered::try_decipher (cipher.rs:217-250): bit k =
 * (C_k mod S)(0) (CipheredBit::decipher :119-122), bytes assembled LSB-first.  out: device,
 * n*(nbits/8) bytes.  nbits % 8 != 0 -> HM_ERR_INVALID_CIPHERED_LENGTH.  Requires the secret key;
 * the first call for a given maximum bound builds a per-key table on the host (synchronous). */
hm_status hm_decrypt_batch(hm_ctx *ctx, const hm_batch *in, uint8_t *out);

/* ---------------- operations (HomomorphicOperation2 impls, src/impls/numbers/uint.rs) ------ */
/* Context::apply2::<HomomorphicAddition, uN>: validate (d >= 21*delta) then common::add
 * (common.rs:37-64) per value.  a, b, out: same nbits; out bounds from hm_add_out_bounds. */
hm_status hm_add_batch(hm_ctx *ctx, const hm_batch *a, const hm_batch *b, hm_batch *out);
/* Context::apply2::<HomomorphicMultiplication, uN / iN> (common.rs:66-163) per value.  Needs a
 * device workspace for the carry list; the context grows it on demand (synchronous allocation
 * on first use per size).  Sizes beyond the engine's limits return HM_ERR_UNSUPPORTED. */
hm_status hm_mul_batch(hm_ctx *ctx, const hm_batch *a, const hm_batch *b, int is_signed,
                       hm_batch *out);
/* The low k output bits of the nbits-bit multiplier ("u32-mul column
 * prefix").  Column i of the carry-save circuit (common.rs:66-105) reads input bits <= i and the
 * carries of columns < i only, so output bits 0..k-1 of the nbits-bit circuit equal the k-bit
 * circuit on the low k bits, bit for bit.  The signed circuit (:115-155) differs from the
 * unsigned one only in column nbits-1, so for k < nbits this is also the signed product's low
 * bits.  a, b: nbits-bit batches read in place; out: k bits, bounds from hm_mul_out_bounds over
 * the first k input bounds.  Same requirement as HM_OP_MUL (d >= 64 delta).  Only input bits
 * 0..k-1 of a and b are read and validated: bits k..nbits-1 are not looked at (a corrupted degree
 * word or limb there raises no HM_ERR_BAD_INPUT). */
hm_status hm_mul_low_batch(hm_ctx *ctx, const hm_batch *a, const hm_batch *b, uint32_t k,
                           hm_batch *out);
/* Context::apply2::<HomomorphicAnd/Or/XorGate> and apply1::<HomomorphicNotGate> (common.rs:5-35,
 * uint.rs:8-58).  For HM_OP_NOT, b is ignored (may be NULL). */
hm_status hm_gate_batch(hm_ctx *ctx, hm_op gate, const hm_batch *a, const hm_batch *b,
                        hm_batch *out);

/* a - b per value (wrapping; one circuit for signed and unsigned types): out_i = a_i + b_i + w_i
 * over the borrow chain of HM_OP_SUB above.  Validates HM_OP_SUB at a->nbits.  a, b, out: same
 * nbits and n; out bounds from hm_sub_out_bounds; out may not overlap a or b.  One launch, no
 * workspace; HM_ERR_UNSUPPORTED when a value's chain does not fit a wavefront's share of LDS. */
hm_status hm_sub_batch(hm_ctx *ctx, const hm_batch *a, const hm_batch *b, hm_batch *out);
/* a cmp b per value, cmp = HM_OP_EQ .. HM_OP_GE.  Orderings: a < b is the borrow out of the top
 * bit, w_nbits (is_signed: bit nbits - 1 generates a_i b_i + a_i, the sign bits' roles
 * exchanged); > exchanges the operands; >= and <= add the unit polynomial.  Equality: the product
 * of all a_i + b_i + 1 (is_signed is ignored).  out: a Ciphered<bool> batch, out->nbits == 8,
 * bounds from hm_compare_out_bounds: bit 0 is the result, bits 1..7 are null polynomials.
 * Validates cmp at a->nbits; otherwise as hm_sub_batch. */
hm_status hm_compare_batch(hm_ctx *ctx, hm_op cmp, const hm_batch *a, const hm_batch *b,
                           int is_signed, hm_batch *out);
/* cond ? a : b per value, obliviously: out_i = b_i + c (a_i + b_i) with c bit 0 of cond, a
 * Ciphered<bool> batch (cond->nbits == 8; bits 1..7 are not read), e.g. a comparison's result or
 * an encrypted bool.  A null c gives b's bits unchanged, the unit polynomial a's.  a, b, out: same
 * nbits and n, cond->n == a->n; out bounds from hm_select_out_bounds(cond->bound[0]); out may not
 * overlap cond, a or b (HM_ERR_INVALID_ARGUMENT).  Validates HM_OP_SELECT (see there for a
 * condition that is not fresh).  One launch, no workspace; HM_ERR_UNSUPPORTED when a value does
 * not fit a wavefront's share of LDS. */
hm_status hm_select_batch(hm_ctx *ctx, const hm_batch *cond, const hm_batch *a, const hm_batch *b,
                          hm_batch *out);
/* min(a, b) or max(a, b) per value, which = HM_OP_MIN or HM_OP_MAX (anything else is
 * HM_ERR_INVALID_ARGUMENT): with w = the borrow out of the top bit of a - b (exactly the
 * polynomial hm_compare_batch(HM_OP_LT) returns, is_signed as there), min is
 * out_i = b_i + w (a_i + b_i) and max out_i = a_i + w (a_i + b_i) -- bit for bit
 * hm_select_batch(a < b, a, b) and hm_select_batch(a < b, b, a), in one launch and without w ever
 * leaving the chip.  out bounds from hm_minmax_out_bounds; validates which at a->nbits; otherwise
 * as hm_select_batch. */
hm_status hm_minmax_batch(hm_ctx *ctx, hm_op which, const hm_batch *a, const hm_batch *b,
                          int is_signed, hm_batch *out);

/* table[v] per value, for any plaintext table: v = the unsigned integer of a's low in_bits
 * ciphertext bits (1 <= in_bits <= min(a->nbits, 8); a is read in place and its bits from in_bits
 * up are neither read nor validated, so a Ciphered<u32>'s low nibble or a comparison's bool,
 * in_bits = 1, can be the index), table = 2^in_bits entries of out_nbytes (1, 2 or 4)
 * little-endian bytes in HOST memory, read during the call only (a captured graph holds no pointer
 * to it).  With f_j(v) = bit j of table[v] and c_j its algebraic normal form,
 * c_j[S] = XOR over S' subset of S of f_j(S') (the Moebius transform over the index bits),
 *   out_j = sum over the S with c_j[S] = 1 of the product of a_i over i in S
 * (the empty product is the unit polynomial; a product with a null factor is null): exact in
 * GF(2)[X] whatever the order of evaluation.  out: out->nbits == 8 out_nbytes, out->n == a->n,
 * bounds from hm_lookup_out_bounds over a's first in_bits bounds (larger ones are accepted,
 * smaller ones HM_ERR_INVALID_ARGUMENT); out may not overlap a (HM_ERR_INVALID_ARGUMENT).
 * Validates HM_OP_LOOKUP at in_bits: the requirement covers fresh index bits; an index that came
 * out of another operation carries that operation's depth, which the caller accounts for.  One
 * launch, no workspace; HM_ERR_UNSUPPORTED when a value does not fit a wavefront's share of
 * LDS. */
hm_status hm_lookup_batch(hm_ctx *ctx, const hm_batch *a, uint32_t in_bits, const uint8_t *table,
                          uint32_t out_nbytes, hm_batch *out);

/* a << s, a >> s, a.rotate_left(s) or a.rotate_right(s) per value for an ENCRYPTED amount s,
 * which = HM_OP_SHL, HM_OP_SHR, HM_OP_ROTL or HM_OP_ROTR (anything else is
 * HM_ERR_INVALID_ARGUMENT); is_signed matters for HM_OP_SHR only and makes it arithmetic (the
 * vacated bits take the sign bit's polynomial).  n = a->nbits is a power of two in 2..128 and
 * L = log2 n; the effective amount is s mod n, Rust's wrapping_shl / wrapping_shr / rotate_*:
 * amount is read in place and only its low L ciphertext bits are read and validated
 * (amount->nbits >= L), so a Ciphered<u8> or a Ciphered<u32> can shift a u32.  One stage per
 * amount bit s_t, with step k = 2^t:
 *   y_i = x_i + s_t (x_i + x_src(i)),   src(i) = i - k (SHL), i + k (SHR), (i -+ k) mod n (ROTL,
 *   ROTR); a src outside 0..n-1 is the null polynomial, or x_{n-1} for the arithmetic SHR.
 * The stages are commuting linear maps of the value, so the result is one polynomial whatever
 * order they run in: exact in GF(2)[X].  A null s_t leaves the value unchanged, the unit
 * polynomial moves it by k.  out: out->nbits == a->nbits, amount->n == a->n == out->n, bounds from
 * hm_shift_out_bounds over the amount's first L bounds (larger ones are accepted, smaller ones
 * HM_ERR_INVALID_ARGUMENT); out may not overlap a or amount, in limbs or in degree words
 * (HM_ERR_INVALID_ARGUMENT).  Validates which at a->nbits: the requirement covers fresh operands;
 * operands that came out of another operation carry that operation's depth, which the caller
 * accounts for.  One launch, no workspace: the value stays in LDS across the stages, in place;
 * HM_ERR_UNSUPPORTED (before any launch) when a value does not fit a wavefront's share of LDS
 * (the value at its output bounds, about 1/16 of 160 KiB: every width up to u128 at
 * d + dp = 256, u64 at 512 and u32 at 1024 fit, u128 at d + dp = 512 does not). */
hm_status hm_shift_batch(hm_ctx *ctx, hm_op which, const hm_batch *a, const hm_batch *amount,
                         int is_signed, hm_batch *out);

/* a.count_ones(), count_zeros(), leading_zeros(), leading_ones(), trailing_zeros() or
 * trailing_ones() per value, which = HM_OP_COUNT_ONES .. HM_OP_TRAILING_ONES (anything else is
 * HM_ERR_INVALID_ARGUMENT), of n = a->nbits bits, n in 1..128 (any width: a 24-bit slice counts
 * as 24 bits).  The result is a Ciphered<u8>.  With the literals u_i = x_i (ones) or x_i + 1
 * (zeros: coefficient 0 flipped, so a unit polynomial becomes the null one):
 *   counts  out_k = e_{2^k}(u_0 .. u_{n-1}), the elementary symmetric polynomial: at 0 / 1 values
 *           it is C(c, 2^k) mod 2 for the count c, which is bit k of c (Lucas).  Evaluated by
 *           E_j <- E_j + u_i E_{j-1} (j descending, E_0 = 1), literal after literal, skipping
 *           every update no target 2^k <= n reads any more: 21, 85 and 341 products for u8, u16
 *           and u32 (29, 101, 373 updates with those by E_0 = 1, which are XORs).
 *   runs    with v_1 .. v_n the literals from the end counted (leading: v_j = u_{n-j}, trailing:
 *           v_j = u_{j-1}) and t_j = v_1 .. v_j (the run is at least j),
 *           out_k = sum of t_{m 2^k} over m >= 1, m 2^k <= n: n - 1 products, the sums are XORs.
 * Every output bit is one fixed polynomial of the input bits whatever the order of evaluation:
 * exact in GF(2)[X] (for a byte, the polynomials hm_lookup_batch gives for the same function's
 * table).  Output bits with 2^k > n are null polynomials.  out: out->nbits == 8, out->n == a->n,
 * bounds from hm_bitcount_out_bounds (larger ones are accepted, smaller ones
 * HM_ERR_INVALID_ARGUMENT); out may not overlap a, in limbs or in degree words
 * (HM_ERR_INVALID_ARGUMENT).  Every bit of a is read and validated.  Validates which at a->nbits:
 * the requirement covers fresh operands; operands that came out of another operation carry that
 * operation's depth, which the caller accounts for.  One launch, no workspace: a count keeps
 * E_1 .. E_J at their bounds in LDS (J = n / 2 for a power of two, whose top target e_n is the
 * running product of all literals, else 2^floor(log2 n)), a run its prefix and one accumulator
 * per output bit; HM_ERR_UNSUPPORTED (before any launch) when that does not fit a wavefront's
 * share of LDS, here 2560 words: a quarter of the other circuits' share, so that four blocks stay
 * resident on a compute unit.  At one bound D = d + dp on every bit, words per wave (-: refused):
 *              u8 D=128/256/512   u16 D=128/256/512   u32 D=128/256/512   u64 D=64/128/256
 *   counts     148 / 272 / 520    344 / 652 / 1268    928 / 1796 / -      1486 / - / -
 *   runs       220 / 416 / 808    478 / 930 / 1834    1056 / 2084 / -     1184 / 2338 / -
 * so every op runs u8 and u16 up to D = 512 and u32 up to D = 256 (the headline parameters);
 * u32 at D = 512 and u64 at D = 256 do not fit (a u64 count at 256 would keep E_1 .. E_32, 4288
 * words), and u128 runs up to D = 32 (a count up to D = 16). */
hm_status hm_bitcount_batch(hm_ctx *ctx, hm_op which, const hm_batch *a, hm_batch *out);

/* arr[i] per value for an ENCRYPTED index i: oblivious memory's read.  An array of count elements,
 * count any integer in 2..256, is count consecutive values of an ordinary batch: element v of
 * array e is value e * count + v, and all elements share the batch's bound[] (what hm_encrypt_batch
 * of n * count plaintext values gives).  k = ceil(log2 count); index is read in place and only its
 * low k ciphertext bits s_0 .. s_{k-1} are read and validated (index->nbits >= k), so a
 * Ciphered<u8> or a Ciphered<u32> can index.  With v_t bit t of v, the indicator of element v is
 *   ind_v = prod_t (s_t + 1 + v_t)           (the literal s_t where v_t = 1, s_t + 1 where 0)
 *   out_j = sum over v < count of ind_v T_{v,j}             (T_{v,j}: bit j of element v)
 * so an index >= count reads 0.  It is evaluated as a multiplexer tree, y = L + s_t (L + R) at
 * level t, a right sibling past the array being the null polynomial: one product per tree node
 * with an element below it (count - 1 per output bit for a power of two).  Every output bit is one
 * fixed polynomial of the inputs whatever the order of evaluation: exact in GF(2)[X] (for null /
 * unit elements, the polynomials hm_lookup_batch gives for the same table).  A null s_t takes the
 * left child, the unit polynomial the right.  n = index->n = out->n values; arr->n == count * n:
 * one array per value; arr->n == count: ONE SHARED TABLE read by every index (a private query);
 * anything else is HM_ERR_INVALID_ARGUMENT.  out: out->nbits == arr->nbits, bounds from
 * hm_array_read_out_bounds over the index's first k bounds (larger ones are accepted, smaller ones
 * HM_ERR_INVALID_ARGUMENT); out may not overlap arr or index, in limbs or in degree words
 * (HM_ERR_INVALID_ARGUMENT).  count outside 2..256, index->nbits < k or a null pointer is
 * HM_ERR_INVALID_ARGUMENT; n == 0 is HM_OK.  Every bit of every element and the k index bits are
 * read and validated.  Validates HM_OP_ARRAY_READ at k: the requirement covers fresh operands;
 * operands that came out of another operation carry that operation's depth, which the caller
 * accounts for.  One launch, no workspace: per output bit a wave keeps one waiting left child per
 * tree level in LDS; HM_ERR_UNSUPPORTED (before any launch) when that does not fit a wavefront's
 * share of LDS, the bit counts' 2560 words.  The slice does not depend on the element width: at
 * one bound D on every bit, count 256 takes 624 words at D = 256, 1192 at D = 512 and 2328 at
 * D = 1024; D = 2048 is refused. */
hm_status hm_array_read_batch(hm_ctx *ctx, const hm_batch *arr, uint32_t count,
                              const hm_batch *index, hm_batch *out);
/* arr[i] = x per value for an ENCRYPTED index i, out of place: oblivious memory's write.  Array
 * layout, count, k and the index as for hm_array_read_batch;
 *   out_{v,j} = T_{v,j} + ind_v (x_j + T_{v,j})       for every v < count
 * so an index >= count writes nowhere.  Each indicator is formed once per array, as the suffix
 * products prod_{i >= t} lit_i(v): stepping v forms again only the levels at or below its lowest
 * set bit, about two products per element.  Exact in GF(2)[X]; a null indicator makes its element
 * an exact copy.  value->nbits == arr->nbits == out->nbits, value->n == index->n == n,
 * arr->n == out->n == count * n (no shared form); bounds from hm_array_write_out_bounds (larger
 * ones are accepted, smaller ones HM_ERR_INVALID_ARGUMENT); out may not overlap arr, index or
 * value (HM_ERR_INVALID_ARGUMENT).  Argument errors, n == 0, validation (HM_OP_ARRAY_WRITE at k)
 * and what is read as for the read, with every bit of value.  One launch, no workspace: the index
 * bits, the k suffix products and all of value's bits stay in LDS for the array; count 256 at
 * D = 256 takes 592 words for u8 elements, 856 for u32 and 1912 for u128 ones
 * (HM_ERR_UNSUPPORTED beyond 2560: u128 elements at D = 512, u32 x 256 at D = 1024). */
hm_status hm_array_write_batch(hm_ctx *ctx, const hm_batch *arr, uint32_t count,
                               const hm_batch *index, const hm_batch *value, hm_batch *out);

/* ---------------- polynomial primitives (src/polynomial.rs), for unit parity ---------------- */
/* Polynomial::add (polynomial.rs:190-213) per pair: out = a ^ b, exact degree. */
hm_status hm_poly_add_batch(hm_ctx *ctx, const hm_polys *a, const hm_polys *b, hm_polys *out);
/* Polynomial::mul (polynomial.rs:252-310) per pair: carry-less product, null short-circuit. */
hm_status hm_poly_mul_batch(hm_ctx *ctx, const hm_polys *a, const hm_polys *b, hm_polys *out);
/* Polynomial::rem (polynomial.rs:316-365): remainder by ONE divisor s (host limbs) for every
 * polynomial of a; s = 0 -> HM_ERR_DIVIDE_BY_ZERO, s = 1 -> HM_ERR_DIVISOR_IS_ONE. */
hm_status hm_poly_rem_batch(hm_ctx *ctx, const hm_polys *a, const uint64_t *s_limbs,
                            size_t s_nlimbs, hm_polys *out);

/* ---------------- ciphertext batch wire format ---------------- */
/* The reference serialises no ciphertexts (only keys, src/context.rs:153-194, :239-297); this is
 * the engine's storage / transfer format for a batch, all fields little-endian:
 *   offset 0   magic "HMCB" (4 bytes)      offset 4   version (u32) = 1
 *   offset 8   nbits (u32)                 offset 12  flags (u32) = 0
 *   offset 16  n (u64)                     offset 24  bound[nbits] (u32)
 *   then       degree[n*nbits] (u32), zero padding to a multiple of 8 bytes,
 *   then       limbs[n*stride] (u64) in the batch layout above (stride = hm_batch_stride).
 * One Ciphered<T> is n = 1 with its Vec<CipheredBit> as the nbits polynomials, bit k of the
 * bincode image first-to-last (src/cipher.rs:127-130, :253-259).  Size in bytes of a batch: */
uint64_t hm_wire_bytes(uint32_t nbits, const uint32_t *bound, uint64_t n);
/* Parse a header (host buffer of len bytes): nbits, n and, when bound is non-NULL, the nbits
 * bounds.  HM_ERR_INVALID_ARGUMENT for a bad magic / version / flags or a length that disagrees
 * with the header. */
hm_status hm_wire_peek(const uint8_t *src, size_t len, uint32_t *nbits, uint64_t *n,
                       uint32_t *bound);
/* Device batch -> host wire image (synchronous: waits for the context's stream).  cap: bytes at
 * dst, at least hm_wire_bytes(in). */
hm_status hm_wire_encode(hm_ctx *ctx, const hm_batch *in, uint8_t *dst, size_t cap);
/* Host wire image -> device batch `out` (caller-allocated from hm_wire_peek: same nbits, n and
 * bounds).  Every polynomial is validated on the host first (degree within its bound, its top
 * coefficient set, zeros above it) -> HM_ERR_BAD_INPUT; synchronous. */
hm_status hm_wire_decode(hm_ctx *ctx, const uint8_t *src, size_t len, hm_batch *out);

/* ---------------- status / sync ---------------- */
/* Waits for the context's stream, then returns (and clears) the first device-side error raised by
 * any kernel since the last check (HM_ERR_CAPACITY, HM_ERR_BAD_INPUT) or a HIP error. */
hm_status hm_ctx_synchronize(hm_ctx *ctx);
/* The HIP runtime's error code (hipError_t) behind the context's most recent HM_ERR_HIP, or 0;
 * diagnostic only, not cleared by this call (hm_ctx_synchronize clears it). */
int32_t hm_ctx_last_hip_error(const hm_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* HOMOMORPH_GPU_H */
