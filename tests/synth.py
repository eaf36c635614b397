"""Synthetic operand batches that FILL their static bounds, the case table of the full-bounds tier
and its references.  Shared by test_synth_reference.py (CPU: the references pinned
against the C oracle, every path assertion) and test_gpu_full_bounds.py (GPU: the engine against
the same references, bit-exact).

A genuine fresh ciphertext bit has degree at most d + d', whatever `bound` its batch was allocated
with, so everything the host derives from the bounds (LDS slices, workspace slots, tile widths,
chunk counts, plan selection) only ever met data as long as its slot at the uniform fresh bounds.
Here a polynomial "fills its bound" when its degree EQUALS the bound (kind FULL, MONO, ONES,
SPARSE): the operand then occupies every word the host sized for it.  The other kinds put degrees
at word and limb edges and the null / unit polynomials at every bit position.

A polynomial is a Python int (bit k = coefficient of X^k), a value the list of its bit
polynomials, least significant first (the model form of oracle/gf2_model.py).
"""
from __future__ import annotations

import functools

import numpy as np

import borrow_model as bm
from oracle import gf2_model as model

KINDS = ("FULL", "MONO", "ONES", "NULL", "UNIT", "EDGE", "SPARSE", "LOW")
PARAMS = (64, 64, 1, 64)      # satisfies every operation's d / delta here
DEC_PARAMS = (128, 128, 1, 128)  # the decryption cases' secret key
SEED = 4242


# ------------------------------------------------------------------ polynomials
def _rand_bits(rng, nbits):
    """A uniformly random integer below 2^nbits."""
    if nbits <= 0:
        return 0
    return int.from_bytes(rng.bytes((nbits + 7) // 8), "little") & ((1 << nbits) - 1)


def _exact(rng, deg):
    """Exact degree deg, random below it."""
    return (1 << deg) | _rand_bits(rng, deg)


def edge_degrees(bound):
    b = int(bound)
    return sorted({d for d in (31, 32, 33, 63, 64, 65, b - 1, 64 * (b // 64) - 1, 64 * (b // 64))
                   if 0 <= d <= b})


def poly(kind, bound, rng):
    """One polynomial of the kind, valid for a bit of this bound (degree <= bound)."""
    b = int(bound)
    if kind == "FULL":
        return _exact(rng, b)
    if kind == "MONO":
        return 1 << b
    if kind == "ONES":
        return (1 << (b + 1)) - 1
    if kind == "NULL":
        return 0
    if kind == "UNIT":
        return 1
    if kind == "EDGE":
        e = edge_degrees(b)
        return _exact(rng, e[int(rng.integers(len(e)))])
    if kind == "SPARSE":
        p = 1 << b
        for _ in range(2):
            if b:
                p |= 1 << int(rng.integers(b))
        return p
    if kind == "LOW":
        return _exact(rng, int(rng.integers(b // 2)) if b >= 2 else 0)
    raise KeyError(kind)


def kind_of(e, i, shift=0):
    """The scheduled kind of value e < 8, bit i."""
    return KINDS[(e + i + shift) % 8]


def operands(bound, n, seed, shift=0):
    """n values over the per-bit bounds.  Value e < 8, bit i is of kind (e + i + shift) mod 8, so
    every kind meets every bit position (the two operands of an operation take different shifts);
    later values draw their kinds at random, FULL weighted highest."""
    bound = np.asarray(bound, dtype=np.uint32)
    rng = np.random.default_rng(seed)
    weights = np.array([9.0] + [1.0] * 7) / 16.0
    out = []
    for e in range(n):
        bits = []
        for i, b in enumerate(bound):
            k = kind_of(e, i, shift) if e < 8 else KINDS[int(rng.choice(8, p=weights))]
            bits.append(poly(k, b, rng))
        out.append(bits)
    return out


def full_pair(ba, bb, n, seed):
    """(A, B): every a_i FULL (degree ba_i), every b_i of degree bb_i - 1 exactly.  With ba = bb
    = B this is the pair that maximises deg P_i = deg x_i + deg a_i b_i = 3B - 1: equal tops would
    cancel in x_i.  In every second value b_0 is FULL as well, so that the first carry or borrow
    a_0 b_0 (+ b_0) has its full degree ba_0 + bb_0 and the chain after it stays as long as the
    bounds allow."""
    rng = np.random.default_rng(seed)
    A = [[_exact(rng, int(b)) for b in ba] for _ in range(n)]
    B = [[_exact(rng, max(int(b) - 1, 0)) for b in bb] for _ in range(n)]
    for e in range(1, n, 2):
        B[e][0] = _exact(rng, int(bb[0]))
    return A, B


def batch(ba, bb, nsched, npair, seed):
    """nsched scheduled / random values followed by npair FULL / bound - 1 pairs."""
    A = operands(ba, nsched, seed, 0)
    B = operands(bb, nsched, seed + 1, 3)
    PA, PB = full_pair(ba, bb, npair, seed + 2)
    return A + PA, B + PB


def words(p):
    """32-bit words of a polynomial (0 for the null polynomial), as load_bit counts them."""
    return (int(p).bit_length() + 31) // 32


def u32(x):
    return np.asarray(x, dtype=np.uint32)


def uniform(nbits, b):
    return np.full(nbits, b, dtype=np.uint32)


# ------------------------------------------------------------------ bounds, restated
def gate_bounds(op, ba, bb):
    ba, bb = u32(ba).astype(np.int64), u32(bb).astype(np.int64)
    if op in ("and", "or"):
        return u32(ba + bb)
    return u32(np.maximum(ba, bb)) if op == "xor" else u32(ba)


def add_bounds(ba, bb):
    out, c = [], -1
    for i, (a, b) in enumerate(zip(map(int, ba), map(int, bb))):
        x = max(a, b)
        out.append(max(x, c))
        ab = a + b
        c = ab if c < 0 else max(ab, x + ab + c)
    return u32(out)


def mul_bounds(ba, bb):
    """Carry-save array (common.rs:66-105) over bounds: a column's items are its partial products
    then the carries of the column before; every item after the first sends on a carry."""
    K = len(ba)
    prev, res = [], []
    for i in range(K):
        items = [int(ba[j]) + int(bb[i - j]) for j in range(i + 1)] + prev
        cur, pb = [], -1
        for x in items:
            if i + 1 < K and pb >= 0:
                cur.append(pb + x)
            pb = max(pb, x)
        res.append(max(pb, 0))
        prev = cur
    return u32(res)


def add_plan(ba, bb):
    """plan_add's sizing (add_host.h), restated as an independent model: cntX, maxPw, SC and what
    follows from them (check_add_path holds the planner's own census against it)."""
    wob = lambda b: 0 if b < 0 else b // 32 + 1  # noqa: E731  words_of_bound
    L = len(ba)
    cntX, SC, maxPw, cntAB, cb = 1, 2, 0, 1, -1
    for i in range(L):
        a, b = int(ba[i]), int(bb[i])
        cntX = max(cntX, wob(max(a, b)))
        if i + 1 < L:
            x, ab = max(a, b), a + b
            p = x + ab
            cntAB = max(cntAB, wob(ab))
            maxPw = max(maxPw, wob(p))
            SC = max(SC, max(wob(p) + wob(cb), wob(ab)) + 2)
            cb = ab if cb < 0 else max(ab, p + cb)
    need_w = (SC + 63) // 64
    wmax = 4 if need_w <= 4 else 8 if need_w <= 8 else 12 if need_w <= 12 else 16 if need_w <= 16 else 24
    nc = 0
    for k, rec in ((7, 64), (13, 64), (25, 128)):  # MfmaCfg<NC>: kChunks, kRecWords
        if maxPw <= 2 * k - 1 and cntAB <= 64 and cntX <= 32 and cntX + maxPw + cntAB + 2 <= rec:
            nc = k
            break
    return dict(cntX=cntX, maxPw=maxPw, SC=SC, need_w=need_w, wmax=wmax,
                pad=need_w <= 24 and maxPw <= 25, nc=nc)


# ------------------------------------------------------------------ traces (from the integers)
def gate_trace(A, B):
    """Per (value, bit): (na, nb) words of the operands the gate kernel multiplies; the product
    spans nout = na + nb words, the uniform operand is a_i (nu = na)."""
    return [[(words(a), words(b)) for a, b in zip(x, y)] for x, y in zip(A, B)]


def borrow_trace(a, b, signed=False, eq=False):
    """Per bit of one value, as borrow_kernel runs it: na, nb, np (words of p_i), nw (words of
    the borrow or equality prefix going in) and nout = np + nw of the product p_i w_i."""
    rows, w = [], 1 if eq else 0
    n = len(a)
    for i in range(n):
        p = a[i] ^ b[i] ^ 1
        rows.append(dict(i=i, na=words(a[i]), nb=words(b[i]), np=words(p), nw=words(w),
                         nout=words(p) + words(w)))
        if eq:
            w = model.clmul_fast(p, w)
        else:
            gen = a[i] if signed and i == n - 1 else b[i]
            w = model.clmul_fast(a[i], b[i]) ^ gen ^ model.clmul_fast(p, w)
    return rows


def add_trace(a, b):
    """Per bit i < L - 1 of one value, as the carry chain runs it: words of x_i, P_i, a_i b_i, the
    carry going in, and of the product P_i carry_i."""
    rows, c = [], 0
    for i in range(len(a)):
        x = a[i] ^ b[i]
        if i + 1 == len(a):
            rows.append(dict(i=i, nx=words(x), np=0, nab=0, nc=words(c), nprod=0))
            break
        ab = model.clmul_fast(a[i], b[i])
        p = model.clmul_fast(x, ab ^ 1)
        rows.append(dict(i=i, nx=words(x), np=words(p), nab=words(ab), nc=words(c),
                         nprod=words(p) + words(c) if p and c else 0))
        c = ab ^ model.clmul_fast(p, c)
    return rows


# ------------------------------------------------------------------ reference circuits
def gate_circuit(op, a, b):
    if op == "and":
        return [model.clmul_fast(x, y) for x, y in zip(a, b)]
    if op == "or":
        return [x ^ y ^ model.clmul_fast(x, y) for x, y in zip(a, b)]
    if op == "xor":
        return [x ^ y for x, y in zip(a, b)]
    return [x ^ 1 for x in a]


def mul_ref(a, b, signed=False):
    return model.mul_circuit(a, b, signed=signed, mul=model.clmul_fast)


# ------------------------------------------------------------------ the case table
GATE_OPS = ("and", "or", "xor", "not")


def _per_bit_gate():
    i = np.arange(8)
    return u32(64 * i + 63), u32(1000 - 97 * i)


GATE_CASES = {
    # name: (a bounds, b bounds)
    "chunks": (uniform(8, 700), uniform(8, 700)),
    "w1_edge": (uniform(8, 1023), uniform(8, 1023)),
    "w2_edge": (uniform(8, 1023), uniform(8, 1055)),
    "one_tile": (uniform(8, 8191), uniform(8, 8191)),
    "multi_tile": (uniform(8, 8191), uniform(8, 8223)),
    "lopsided": (uniform(8, 40), uniform(8, 9000)),
    "lopsided_swapped": (uniform(8, 9000), uniform(8, 40)),
    "per_bit": _per_bit_gate(),
}


def _u16_borrow_bounds():
    """Per-bit bounds spread over 63..1100, different per operand: on every bit one operand is
    near the top of the range and the other on a 64-step ladder from 63 up, alternating.  The
    borrow's degree grows by max(ba_i, bb_i) per bit, so a spread whose per-bit maximum averages
    below 16384 / 17 = 964 could not take the last borrow past 512 words; this one averages about
    1080 (the last product p_15 w_15 has degree ba_0 + bb_0 + sum_{i>=1} max(ba_i, bb_i) = 17328,
    542 words)."""
    i = np.arange(16)
    hi, lo = 1100 - 3 * i, 63 + 64 * i
    ba = np.where(i % 2 == 0, hi, lo)
    bb = np.where(i % 2 == 0, lo, hi)
    return u32(ba), u32(bb)


BORROW_CASES = {
    # name: (a bounds, b bounds, scheduled + random values, FULL / bound - 1 pairs)
    "u8_b700": (uniform(8, 700), uniform(8, 700), 9, 2),
    "u16_per_bit": _u16_borrow_bounds() + (8, 2),
    "u8_pair_b255": (uniform(8, 255), uniform(8, 255), 0, 8),
}

ADD_UNIFORM = (138, 139, 266, 267, 522, 523)
ADD_MAXPW = {138: 13, 139: 14, 266: 25, 267: 26, 522: 49, 523: 50}


def _last_wide(top):
    ba = uniform(8, 128)
    ba[7] = top
    return ba, uniform(8, 128)


def _add_per_bit():
    rng = np.random.default_rng(SEED + 7)
    return (u32(rng.integers(64, 267, size=8)), u32(rng.integers(64, 267, size=8)))


ADD_CASES = {f"u8_b{B}": (uniform(8, B), uniform(8, B), 8, 4) for B in ADD_UNIFORM}
ADD_CASES.update({
    "u16_b266": (uniform(16, 266), uniform(16, 266), 8, 2),
    "u32_b266": (uniform(32, 266), uniform(32, 266), 2, 2),
    "last_1023": _last_wide(1023) + (8, 4),
    "last_1024": _last_wide(1024) + (8, 4),
    "per_bit": _add_per_bit() + (8, 4),
})


def _mul_per_bit(nbits, seed):
    rng = np.random.default_rng(seed)
    return (u32(rng.integers(64, 201, size=nbits)), u32(rng.integers(64, 201, size=nbits)))


MUL_CASES = {
    # name: (a bounds, b bounds, signed, k (mul_low) or None, scheduled + random, pairs)
    "u8_b128": (uniform(8, 128), uniform(8, 128), False, None, 8, 2),
    "i8_b128": (uniform(8, 128), uniform(8, 128), True, None, 8, 2),
    "u8_per_bit": _mul_per_bit(8, SEED + 11) + (False, None, 8, 2),
    "u16_low4_per_bit": _mul_per_bit(16, SEED + 12) + (False, 4, 8, 2),
}

def _mc(ba, bb, k=4, signed=False, ka=None):
    """One multiplier class case: u8 operands (an int: that bound on all 8 bits), mul_low(k) or the
    full circuit (k None), Karatsuba options ka = (min words, leaf words) or the defaults."""
    ba = uniform(8, ba) if np.isscalar(ba) else u32(ba)
    bb = uniform(8, bb) if np.isscalar(bb) else u32(bb)
    return dict(ba=ba, bb=bb, k=k, signed=signed, ka=ka)


# One case per product class of the multiplier at its size edges: 8 scheduled
# values + 2 FULL / bound - 1 pairs each; the path of each is asserted from the planner's own
# census (mul_census) in check_mul_class_path.
MUL_CLASS_CASES = {
    "ppv_12w": _mc(383, 383),
    "ppg_tiny_13w": _mc(384, 384),
    "ppg_tiny_20w": _mc(639, 639),
    "ppg_gen_21w": _mc(640, 640),
    "ppg_gen_33w": _mc(1055, 1055),
    "w34_1056": _mc(1056, 1056),
    "w34_1087": _mc(1087, 1087),
    "ppm_35w": _mc(1088, 1088),
    "wide_76": _mc(1152, 1152),
    "ppm_wide": _mc(2304, 2304, k=3),
    "ppm_narrow_2303": _mc(2303, 2303, k=3),
    "rows_v36": _mc(287, 287),
    "tiny_v40": _mc(288, 288),
    "tiny_v40_319": _mc(319, 319),
    "narrow_24": _mc(320, 320),
    "ppg_lopsided": _mc(127, 1055),
    "ppg_lopsided_swapped": _mc(1055, 127),
    "tiny_under_wide_prefix": _mc([1200] + [100] * 7, 100),
    "u8_b640_full": _mc(640, 640, k=None),
    "i8_b640_full": _mc(640, 640, k=None, signed=True),
    "u8_b703_ka224": _mc(703, 703, k=None, ka=(224, 224)),
}

# Degree ladders (ladder): name -> (uniform bound, W values); mul_low(3), so that column 1 pushes
# exactly one carry product, U = a_0 b_1 against V = a_1 b_0.
MUL_LADDERS = {
    "ladder_ppv": (383, 12),
    "ladder_ppg_tiny": (639, 20),
    "ladder_ppg_gen": (1055, 33),
    "ladder_w34": (1087, 34),
    "ladder_ppm": (1088, 35),
    "ladder_rows": (287, 9),
}
for _n, (_b, _w) in MUL_LADDERS.items():
    MUL_CLASS_CASES[_n] = _mc(_b, _b, k=3)


def ladder(ba, bb, W, seed):
    """W values; every a_i of value e has exactly e + 1 words: degree 32 (e + 1) - 1 on even bits
    (the top bit is its word's last; capped at the bound) and 32 e on odd bits (its word's first:
    value 0's odd bits are the unit polynomial), random below the top bit.  Every b_i is FULL."""
    rng = np.random.default_rng(seed)
    A, B = [], []
    for e in range(W):
        A.append([_exact(rng, min(32 * (e + 1) - 1, int(b)) if i % 2 == 0 else 32 * e)
                  for i, b in enumerate(ba)])
        B.append([_exact(rng, int(b)) for b in bb])
    return A, B


DEC_CASES = {
    # name: per-bit bounds (u8, n = 64)
    "b511_ucap": uniform(8, 511),
    "b512": uniform(8, 512),
    "per_bit": u32([63, 482, 902, 1321, 1741, 2160, 2580, 3000]),
    "per_bit_cap32": u32([63, 346, 629, 913, 1196, 1480, 1763, 2047]),
}
DEC_N = 64

# The cipher-paths tier's decryption cases (cipher_paths.py, test_gpu_cipher_paths.py), named for
# the kernel and branch they reach (check_dec_path): name -> (per-bit bounds, n).  A bit of
# capacity C has bound 64 C - 1, so a polynomial that fills it has its top coefficient in the
# last bit of the bit's last limb.
DEC_WIDE_BITS = {0: 193, 1: 255, 62: 256, 63: 257, 64: 449, 65: 512, 127: 513}  # bit -> limbs


def _dec_wide128():
    cap = [1 + i % 4 for i in range(128)]
    for i, c in DEC_WIDE_BITS.items():
        cap[i] = c
    return u32([64 * c - 1 for c in cap])


DEC_PATH_CASES = {f"bits_ucap_c{C}_n{n}": (uniform(8, 64 * C - 1), n)
                  for C in (1, 8) for n in (1, 3, 9)}
DEC_PATH_CASES.update({
    "bits_ucap_c1_16byte_n3": (uniform(128, 63), 3),
    "bits_ucap_c8_16byte_n3": (uniform(128, 511), 3),
    # capacity 1 + (i + i / 32) mod 32: each of 1 .. 32 at four bits whose scheduled kinds differ
    "bits_general_16byte_caps1_32_n3": (u32([64 * (1 + (i + i // 32) % 32) - 1 for i in range(128)]), 3),
    "wave_16byte_wide_n5": (_dec_wide128(), 5),
    "wave_u8_cap512_n6": (uniform(8, 64 * 512 - 1), 6),
})


def _dec_spec(name):
    """(per-bit bounds, n) of a decryption case of either table."""
    return (DEC_CASES[name], DEC_N) if name in DEC_CASES else DEC_PATH_CASES[name]


def _seed(family, name):
    return SEED + sum(ord(c) * (k + 1) for k, c in enumerate(family + "/" + name)) % 100000


@functools.lru_cache(maxsize=None)
def inputs(family, name):
    """dict(ba, bb, A, B, n, nbits) of a case (model form), made once."""
    if family == "gate":
        ba, bb = GATE_CASES[name]
        ns, npair = 8, 2
    elif family == "borrow":
        ba, bb, ns, npair = BORROW_CASES[name]
    elif family == "add":
        ba, bb, ns, npair = ADD_CASES[name]
    elif family == "mul":
        ba, bb, _, _, ns, npair = MUL_CASES[name]
    elif family == "mulc":
        ba, bb = MUL_CLASS_CASES[name]["ba"], MUL_CLASS_CASES[name]["bb"]
        ns, npair = 8, 2
    elif family == "dec":
        ba, ns = _dec_spec(name)
        bb, npair = ba, 0
    else:
        raise KeyError(family)
    if family == "mulc" and name in MUL_LADDERS:
        A, B = ladder(ba, bb, MUL_LADDERS[name][1], _seed(family, name))
    else:
        A, B = batch(ba, bb, ns, npair, _seed(family, name))
    return dict(ba=u32(ba), bb=u32(bb), A=A, B=B, n=len(A), nbits=len(ba))


def packed(family, name):
    """The case's operands in the batch layout: (la, da, lb, db)."""
    c = inputs(family, name)
    return bm.pack(c["A"], c["ba"]) + bm.pack(c["B"], c["bb"])


def _frozen(l, d):
    l.setflags(write=False)
    d.setflags(write=False)
    return l, d


@functools.lru_cache(maxsize=None)
def gate_reference(name, op):
    """(out bounds, limbs, degree words) of the model's gate on the case."""
    c = inputs("gate", name)
    ob = gate_bounds(op, c["ba"], c["bb"])
    vals = [gate_circuit(op, a, b) for a, b in zip(c["A"], c["B"])]
    return (ob, vals) + _frozen(*bm.pack(vals, ob))


@functools.lru_cache(maxsize=None)
def borrow_reference(name, op, signed=False):
    """op: "sub" or a comparison.  (out bounds, values, limbs, degree words)."""
    c = inputs("borrow", name)
    if op == "sub":
        ob = bm.sub_bounds(c["ba"], c["bb"])
        vals = [bm.sub_circuit(a, b) for a, b in zip(c["A"], c["B"])]
    else:
        ob = bm.compare_bounds(op, c["ba"], c["bb"])
        vals = [bm.bool_value(bm.compare_circuit(op, a, b, signed))
                for a, b in zip(c["A"], c["B"])]
    return (ob, vals) + _frozen(*bm.pack(vals, ob))


@functools.lru_cache(maxsize=None)
def add_reference(name):
    c = inputs("add", name)
    ob = add_bounds(c["ba"], c["bb"])
    vals = [model.add_circuit(a, b) for a, b in zip(c["A"], c["B"])]
    return (ob, vals) + _frozen(*bm.pack(vals, ob))


@functools.lru_cache(maxsize=None)
def mul_reference(name):
    c = inputs("mul", name)
    _, _, signed, k, _, _ = MUL_CASES[name]
    k = k or c["nbits"]
    ob = mul_bounds(c["ba"][:k], c["bb"][:k])
    vals = [mul_ref(a[:k], b[:k], signed) for a, b in zip(c["A"], c["B"])]
    return (ob, vals) + _frozen(*bm.pack(vals, ob))


@functools.lru_cache(maxsize=None)
def mul_class_reference(name):
    """(out bounds, values, limbs, degree words) of the model's carry-save circuit on a
    MUL_CLASS_CASES case: the k-bit circuit on the low k bits, or the full (signed) one."""
    c = inputs("mulc", name)
    spec = MUL_CLASS_CASES[name]
    k = spec["k"] or c["nbits"]
    ob = mul_bounds(c["ba"][:k], c["bb"][:k])
    vals = [mul_ref(a[:k], b[:k], spec["signed"]) for a, b in zip(c["A"], c["B"])]
    return (ob, vals) + _frozen(*bm.pack(vals, ob))


# ------------------------------------------------------------------ the planner's census
@functools.lru_cache(maxsize=None)
def _census_driver(name="plan_census"):
    """Builds tests/sanitize/_build/<name> (a planner compiled into a host-only driver, ASan +
    UBSan) once per process."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    san = os.path.join(root, "tests", "sanitize")
    if name != "add_census":  # (plan_census links the library's objects; add_census nothing)
        subprocess.run(["make", "-s", "-C", os.path.join(root, "homomorph-rust_amd")], check=True,
                       timeout=1200)
    subprocess.run(["make", "-s", "-C", san, "_build/" + name], check=True, timeout=1200)
    return os.path.join(san, "_build", name)


def _run_census(name, args):
    import json
    import os
    import subprocess
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([_census_driver(name)] + [str(int(x)) for x in args], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout)


@functools.lru_cache(maxsize=None)
def plan_census(L, K, signed, ka_min, ka_leaf, mfma, ba, bb):
    """The planner's own account of one plan (tests/sanitize/plan_census.cpp), as a dict.  CPU
    only.  Any sanitizer report fails the run."""
    return _run_census("plan_census",
                       [L, K, int(signed), ka_min, ka_leaf, int(mfma)] + list(ba) + list(bb))


@functools.lru_cache(maxsize=None)
def add_census(n, add_chain, fp4, ba, bb):
    """plan_add's own account of one adder plan (tests/sanitize/add_census.cpp), as a dict:
    "status", and when it is 0 every plan field of AddArgs and the kernel instances.  ba, bb:
    tuples of per-bit bounds.  CPU only.  Any sanitizer report fails the run."""
    return _run_census("add_census", [len(ba), n, add_chain, int(fp4)] + list(ba) + list(bb))


def mul_census(name, mfma=True):
    """The census of a MUL_CLASS_CASES case as mul_columns plans it: L = 8, K = k, the signed
    corners only in the full circuit (mul_host.cpp mul_columns: flip = is_signed && K == L), the
    context's Karatsuba defaults (ctx.h: 256, 256) unless the case sets its own."""
    spec = MUL_CLASS_CASES[name]
    K = spec["k"] or 8
    ka = spec["ka"] or (256, 256)
    return plan_census(8, K, spec["signed"] and K == 8, ka[0], ka[1], mfma,
                       tuple(int(x) for x in spec["ba"][:K]), tuple(int(x) for x in spec["bb"][:K]))


@functools.lru_cache(maxsize=None)
def dec_reference(name):
    """The plaintext bytes of the case's operand a under the DEC_PARAMS key (the model's
    decipher_bit; test_synth_reference.py and test_cipher_paths.py pin it to
    oracle.decrypt_batch): (n, nbits / 8) uint8, a value's bytes little-endian."""
    c = inputs("dec", name)
    s, _ = model.keygen(*DEC_PARAMS, SEED)
    nbytes = c["nbits"] // 8
    out = np.array([list(bm.decrypt_value(bits, s).to_bytes(nbytes, "little")) for bits in c["A"]],
                   dtype=np.uint8)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------ path assertions
def check_gate_path(name):
    """The path each gate case is named for (gate_kernel: wave_mul<kQSmall = 10, 8>(a_i, na, b_i,
    nb, ...), nout = na + nb, W = ceil(nout / 64) capped at 8, further tiles MULTI)."""
    c = inputs("gate", name)
    t = [r for v in gate_trace(c["A"], c["B"]) for r in v]
    nu, nout = max(r[0] for r in t), max(r[0] + r[1] for r in t)
    tile_w = min(8, (nout + 63) // 64)
    if name == "chunks":
        assert nu == 22 and (nu + 9) // 10 == 3
    elif name == "w1_edge":
        assert nout == 64 and tile_w == 1
    elif name == "w2_edge":
        assert nout == 65 and tile_w == 2
    elif name == "one_tile":
        assert nout == 512 and tile_w == 8 and nout <= 64 * 8
    elif name == "multi_tile":
        assert nout == 513 and nout > 64 * 8
    elif name == "lopsided":
        assert nu == 2 and max(r[1] for r in t) == 282
    elif name == "lopsided_swapped":
        assert nu == 282 and max(r[1] for r in t) == 2
    elif name == "per_bit":
        ca, cb = c["ba"] // 64 + 1, c["bb"] // 64 + 1
        # within an operand every capacity is distinct, and past bit 0 the two operands never
        # share an offset
        assert len(set(ca.tolist())) == 8 and len(set(cb.tolist())) == 8
        assert not (np.cumsum(ca)[:-1] == np.cumsum(cb)[:-1]).any()
        for i in range(8):  # and every bit's slot is filled by some value
            assert max(r[i][0] for r in gate_trace(c["A"], c["B"])) == int(c["ba"][i]) // 32 + 1
            assert max(r[i][1] for r in gate_trace(c["A"], c["B"])) == int(c["bb"][i]) // 32 + 1
    # the OR scratch Xs = T + na + nb + 2 starts as far in as the case's widest product
    return dict(nu=nu, nout=nout)


def check_borrow_path(name):
    """borrow_kernel: the generate product wave_mul<kQSmall, 8>(a_i, na, b_i, nb, ...) and the
    propagate product wave_mul<kQSmall, 8>(p_i, np, w_i, nw, ...); borrow_run's slots SA = SB = SX
    = 2 cap and cw = SX + chain / 32 + 3."""
    c = inputs("borrow", name)
    lt = [borrow_trace(a, b) for a, b in zip(c["A"], c["B"])]
    rows = [r for t in lt for r in t]
    na, np_, nout = (max(r[k] for r in rows) for k in ("na", "np", "nout"))
    slot = 2 * int(max(c["ba"].max(), c["bb"].max()) // 64 + 1)
    chain = bm.borrow_bounds(c["ba"], c["bb"], c["nbits"])[-1]
    if name == "u8_b700":
        assert na == 22 and (na + 9) // 10 == 3 and np_ == 22 and slot == 22
        # the last product p_7 w_7 is as long as the bounds allow: the borrow buffers are filled
        assert nout == 22 + bm.borrow_bounds(c["ba"], c["bb"], 7)[-1] // 32 + 1 == 198
    elif name == "u16_per_bit":
        assert lt[-1][-1]["nout"] > 512, lt[-1][-1]  # p_15 w_15: a MULTI tile
        assert nout == max(t[-1]["nout"] for t in lt)
        for k, bnd in (("na", c["ba"]), ("nb", c["bb"])):  # every bit's slot is filled
            for i in range(16):
                assert max(t[i][k] for t in lt) == int(bnd[i]) // 32 + 1
    elif name == "u8_pair_b255":
        assert all(r["na"] == 8 and r["np"] == 8 for r in rows) and slot == 8
        assert all(a[i].bit_length() - 1 == 255 for a in c["A"] for i in range(8))
    return dict(na=na, np=np_, nout=nout, chain=chain)


def check_add_path(name):
    """hm_add_batch's plan limits (add_host.h: maxPw <= 2 NC - 1, cntX <= 32, PAD: maxPw <= 25,
    wmax from need_w = ceil(SC / 64)) and data that reaches them."""
    c = inputs("add", name)
    plan = add_plan(c["ba"], c["bb"])
    # the planner's own output (AUTO chain on a device with the fp4 MFMA, the batch as the GPU
    # tier runs it) agrees with the model on every field they share
    cen = add_census(len(c["A"]), 0, True, tuple(int(x) for x in c["ba"]),
                     tuple(int(x) for x in c["bb"]))
    assert cen["status"] == 0
    assert (cen["cntX"], cen["cntP"], cen["max_prod_words"], bool(cen["pad"]), cen["mfma"]) == (
        plan["cntX"], plan["maxPw"], plan["SC"], plan["pad"], plan["nc"]), (cen, plan)
    tr = [add_trace(a, b) for a, b in zip(c["A"], c["B"])]
    rows = [r for t in tr for r in t]
    npw, nx, nprod = (max(r[k] for r in rows) for k in ("np", "nx", "nprod"))
    # the data fills the plan's slots (where ba_i = bb_i the tops cancel in x_i, so P_i stops one
    # short of its bound: that costs a word only where the bound is a multiple of 32)
    reach = max((max(a, b) + a + b - (a == b)) // 32 + 1
                for a, b in zip(map(int, c["ba"][:-1]), map(int, c["bb"][:-1])))
    assert npw == reach >= plan["maxPw"] - 1 and nx == plan["cntX"]
    if name.startswith("u8_b"):
        B = int(name[4:])
        assert npw == ADD_MAXPW[B]
        assert plan["nc"] == {138: 7, 139: 13, 266: 13, 267: 25, 522: 25, 523: 0}[B]
        assert plan["pad"] == (B <= 266)
    elif name in ("u16_b266", "u32_b266"):
        assert npw == 25 and plan["nc"] == 13 and plan["pad"]
        assert (plan["SC"], plan["need_w"], plan["wmax"]) == ((368, 6, 8) if name == "u16_b266"
                                                              else (767, 12, 12))
        assert plan["SC"] - 2 - nprod <= 1  # the widest product fills the carry buffer
    elif name == "last_1023":
        assert plan["cntX"] == 32 and plan["nc"] == 7
        assert max(t[7]["nx"] for t in tr) == 32  # x_7's 32nd word is live
    elif name == "last_1024":
        assert plan["cntX"] == 33 and plan["nc"] == 0
        assert max(t[7]["nx"] for t in tr) == 33
    elif name == "per_bit":
        assert plan["nc"] in (7, 13) and plan["pad"]
        assert len(set((c["ba"] // 64).tolist() + (c["bb"] // 64).tolist())) >= 3
        for i in range(8):  # every bit's slot is filled
            assert max(t[i]["nx"] for t in tr) == int(max(c["ba"][i], c["bb"][i])) // 32 + 1
    return dict(plan, np=npw, nx=nx, nprod=nprod)


def check_mul_path(name):
    """Every kind reaches every column: a NULL and a UNIT partial product and an ONES operand in
    each bit position of each operand (the schedule), and operands that fill their bounds."""
    c = inputs("mul", name)
    nb = c["nbits"]
    for X, bnd, shift in ((c["A"], c["ba"], 0), (c["B"], c["bb"], 3)):
        for i in range(nb):
            col = [X[e][i] for e in range(8)]
            assert 0 in col and 1 in col and (1 << (int(bnd[i]) + 1)) - 1 in col
            assert max(p.bit_length() - 1 for p in col) == int(bnd[i])
    caps = np.concatenate([c["ba"] // 64 + 1, c["bb"] // 64 + 1])
    if "per_bit" in name:
        assert len(set(caps.tolist())) >= 2 and (c["ba"] // 64 != c["bb"] // 64).any()
    return dict(caps=caps)


def _launch(m, instance, umax, vmax=None):
    return (m["nspans"] > 0 and m["instance"] == instance and m["umax"] == umax
            and (vmax is None or m["vmax"] == vmax))


def check_mul_class_path(name):
    """The path each MUL_CLASS_CASES case is named for, from the planner's census of the case's
    bounds (mul_census: which launch mul_columns makes, with which sizes, and the instance
    launch_mul_ppg / launch_mul_mfma pick for it) together with the model's integers (the word
    counts the kernels then branch on: nu = words(a_j) in mul_ppv_kernel / mul_ppg_kernel, nu / 2
    + 1 chunks in one group there, groups of 16 and one tail group of 1..17 in mf_item)."""
    c = inputs("mulc", name)
    spec = MUL_CLASS_CASES[name]
    K = spec["k"] or 8
    cen = mul_census(name)
    cols = cen["cols"]
    TINY, NARROW, WIDE = 0, 1, 2
    assert len(cols) == K
    # VALU plans keep every product off the matrix cores
    valu = mul_census(name, mfma=False)
    assert not valu["ppg"] and not valu["ppv"]
    assert all(not col["ppl"]["nspans"] and not col["nrows"] and
               not any(m["nspans"] for m in col["mfl"]) for col in valu["cols"])
    nua = [[words(v[j]) for j in range(K)] for v in c["A"]]     # per value: words of a_j
    nub = [[words(v[j]) for j in range(K)] for v in c["B"]]
    if name not in MUL_LADDERS:
        # some value fills every operand slot the plan sized (the FULL / bound - 1 pairs)
        for j in range(K):
            assert max(r[j] for r in nua) == int(c["ba"][j]) // 32 + 1
            assert max(r[j] for r in nub) == int(c["bb"][j]) // 32 + 1
        # ... and the schedule puts a null and a unit operand in every bit position
        for X in (c["A"], c["B"]):
            for j in range(K):
                assert {0, 1} <= {X[e][j] for e in range(8)}
    ppl = [col["ppl"] for col in cols]
    pp = cen["pp_instance"]
    if name == "ppv_12w":
        assert cen["ppg"] and cen["ppv"] and cen["ppg_umax"] == 12 and pp == "mul_ppv_kernel"
    elif name in ("ppg_tiny_13w", "ppg_tiny_20w"):
        assert cen["ppg"] and not cen["ppv"] and pp == "mul_ppg_kernel<11>"
        assert cen["ppg_umax"] == {"ppg_tiny_13w": 13, "ppg_tiny_20w": 20}[name]
    elif name in ("ppg_gen_21w", "ppg_gen_33w"):
        assert cen["ppg"] and not cen["ppv"] and pp == "mul_ppg_kernel<17>"
        assert cen["ppg_umax"] == {"ppg_gen_21w": 21, "ppg_gen_33w": 33}[name]
        if name == "ppg_gen_21w":
            assert _launch(cols[1]["mfl"][NARROW], "narrow", 44)
        else:  # 33 words: 17 chunks, the last count mul_ppg_kernel's one group holds
            assert max(r[0] for r in nua) // 2 + 1 == 17
    elif name in ("w34_1056", "w34_1087", "ppm_35w"):
        # 34 words are 18 chunks, one more than mul_ppg_kernel's group: no grouped launch
        # (kMfPPGWords = 33), the partial products are per-column launches on the narrow instance
        assert not cen["ppg"] and not cen["ppv"] and pp == ""
        assert all(_launch(m, "narrow", 36, 36) for m in ppl)
        assert max(r[0] for r in nua) == (35 if name == "ppm_35w" else 34)
        u = 72 if name == "ppm_35w" else 68
        assert _launch(cols[1]["mfl"][NARROW], "narrow", u) and _launch(cols[2]["mfl"][NARROW], "narrow", u)
        assert not any(col["mfl"][WIDE]["nspans"] for col in cols)
    elif name == "wide_76":
        assert all(_launch(m, "narrow", 40, 40) for m in ppl)
        assert _launch(cols[1]["mfl"][WIDE], "wide_win", 76) and _launch(cols[2]["mfl"][WIDE], "wide_win", 76)
        assert not any(col["mfl"][NARROW]["nspans"] for col in cols)
    elif name == "ppm_wide":
        assert not cen["ppg"] and all(_launch(m, "wide", 76, 76) for m in ppl)
    elif name == "ppm_narrow_2303":
        assert not cen["ppg"] and all(_launch(m, "narrow", 72, 72) for m in ppl)
    elif name == "rows_v36":
        col = cols[2]
        assert (col["nrows"], col["rows_uw"], col["rows_vw"], col["rows_qw"]) == (3, 20, 36, 18)
        assert not any(m["nspans"] for col in cols for m in col["mfl"])
    elif name in ("tiny_v40", "tiny_v40_319"):
        col = cols[2]
        assert _launch(col["mfl"][TINY], "tiny", 20, 40) and col["mfl"][TINY]["nspans"] == 1
        assert col["nrows"] == 2 and col["rows_qw"] == (19 if name == "tiny_v40" else 20)
    elif name == "narrow_24":
        assert not any(col["nrows"] for col in cols)
        assert _launch(cols[1]["mfl"][NARROW], "narrow", 24) and _launch(cols[2]["mfl"][NARROW], "narrow", 24)
    elif name == "ppg_lopsided":
        assert (cen["ppg_umax"], cen["ppg_vmax"], pp) == (4, 33, "mul_ppg_kernel<11>")
    elif name == "ppg_lopsided_swapped":
        assert (cen["ppg_umax"], cen["ppg_vmax"], pp) == (33, 4, "mul_ppg_kernel<17>")
    elif name == "tiny_under_wide_prefix":
        assert not cen["ppg"] and all(_launch(m, "tiny", 4, 40) for m in ppl)
        assert _launch(cols[1]["mfl"][TINY], "tiny", 8, 44) and _launch(cols[2]["mfl"][TINY], "tiny", 8, 44)
    elif name in ("u8_b640_full", "i8_b640_full"):
        assert pp == "mul_ppg_kernel<17>" and cen["ppg_umax"] == 21
        for i in (3, 4, 5, 6):
            assert cols[i]["mfl"][NARROW]["instance"] == "narrow"
            assert cols[i]["mfl"][WIDE]["instance"] == "wide_win"
        ka = cols[6]["ka"]
        assert len(ka) == 4 and {g["lane"] for g in ka} == {0, 1}
        assert {g["leaf_umax"] for g in ka} == {192, 256} and not any(g["lean_leaf"] for g in ka)
        # the signed corners: two VALU partial products (+1) in column 7, beside the grouped launch
        assert [col["npp"] for col in cols] == [0] * 7 + [2 if spec["signed"] else 0]
        assert bool(cen["signed"]) == spec["signed"]
    elif name == "u8_b703_ka224":
        lean = [g for col in cols for g in col["ka"] if g["lean_leaf"]]
        assert {g["lane"] for g in lean} == {0, 1}
        assert all(g["leaf_umax"] == 224 and g["leaf_vmax"] == 224 for g in lean)
    elif name in MUL_LADDERS:
        _check_ladder(name, c, cen, nua)
    else:
        raise KeyError(name)
    return cen


def _check_ladder(name, c, cen, nua):
    B, W = MUL_LADDERS[name]
    cols = cen["cols"]
    assert c["n"] == W
    for e in range(W):  # exactly e + 1 words; tops on a word's last bit (even) / first bit (odd)
        assert set(nua[e]) == {e + 1}
        assert c["A"][e][0].bit_length() == min(32 * (e + 1), B + 1)
        assert c["A"][e][1].bit_length() == 32 * e + 1
        assert all(b.bit_length() - 1 == B for b in c["B"][e])
    nu = [r[0] for r in nua]
    chunks = [n // 2 + 1 for n in nu]
    # column 1's carry product: U = p_1 = a_0 b_1 (the prefix; both slots have equal capacity, and
    # mul_host.cpp takes the prefix as U then)
    u1 = [words(model.clmul_fast(a[0], b[1])) for a, b in zip(c["A"], c["B"])]
    if name == "ladder_ppv":
        assert cen["pp_instance"] == "mul_ppv_kernel" and cen["ppg_umax"] == 12
        assert nu == list(range(1, 13))
    elif name == "ladder_ppg_tiny":
        assert cen["pp_instance"] == "mul_ppg_kernel<11>" and cen["ppg_umax"] == 20
        assert set(chunks) == set(range(1, 12))
    elif name == "ladder_ppg_gen":
        assert cen["pp_instance"] == "mul_ppg_kernel<17>" and cen["ppg_umax"] == 33
        assert set(chunks) == set(range(1, 18))
        assert _launch(cols[1]["mfl"][1], "narrow", 68) and u1 == list(range(34, 67))
    elif name in ("ladder_w34", "ladder_ppm"):
        # per-column launches on the narrow instance: chunk counts 1..18, so every tail group
        # 1..17 and, at 18, one full group of 16 and a tail of 2
        assert not cen["ppg"] and all(_launch(col["ppl"], "narrow", 36, 36) for col in cols)
        assert set(chunks) == set(range(1, 19)) and chunks[-1] == 18
        # the carry's U on the narrow instance at every word count 35..68: chunk counts 18..35,
        # every tail size after one full group and after two
        assert _launch(cols[1]["mfl"][1], "narrow", 68 if name == "ladder_w34" else 72)
        assert u1[:34] == list(range(35, 69))
        assert {n // 2 + 1 for n in u1[:34]} == set(range(18, 36))
    elif name == "ladder_rows":
        col = cols[1]
        assert (col["nrows"], col["rows_uw"], col["rows_qw"]) == (1, 20, 18)
        # deg U = deg a_0 + 287: 10 words at value 0, rows_qw = 18 at the last
        assert u1 == list(range(10, 19))


def check_dec_path(name):
    """hm_decrypt_batch: D.ucap = the common capacity when all are equal and <= 8 limbs."""
    if name in DEC_PATH_CASES:
        return _check_dec_path_case(name)
    c = inputs("dec", name)
    caps = (c["ba"] // 64 + 1).tolist()
    ucap = caps[0] if len(set(caps)) == 1 and caps[0] <= 8 else 0
    assert ucap == {"b511_ucap": 8, "b512": 0, "per_bit": 0, "per_bit_cap32": 0}[name]
    if name == "b512":
        assert caps == [9] * 8
    if name == "per_bit":  # launch_decrypt: maxcap > 32, one wave per value (decrypt_kernel)
        assert len(set(caps)) == 8 and caps[0] == 1 and caps[-1] == 47
    if name == "per_bit_cap32":  # maxcap = 32, the last on decrypt_bits_kernel
        assert len(set(caps)) == 8 and caps[0] == 1 and caps[-1] == 32
    for i in range(8):  # some polynomial reaches the last bit of every bit's capacity-defining bound
        assert max(v[i].bit_length() - 1 for v in c["A"]) == int(c["ba"][i])
    return dict(ucap=ucap)


def _check_dec_path_case(name):
    """The DEC_PATH_CASES, against cipher_paths.dec_dispatch (launch_decrypt: `D.maxcap <= 32` picks
    decrypt_bits_kernel, whose `if (D.ucap)` path stages 64 C limbs per wave in LDS; else
    decrypt_kernel, whose 4-way unrolled body runs while `k + (kDecUnroll - 1) * kWave < cap`)."""
    import cipher_paths as cp
    c = inputs("dec", name)
    caps = (c["ba"] // 64 + 1).tolist()
    d = cp.dec_dispatch(c["ba"], c["n"])
    top = lambda i: max(v[i].bit_length() - 1 for v in c["A"]) == int(c["ba"][i])  # noqa: E731
    # some polynomial reaches the top coefficient of every capacity the host sizes a slot by
    for cap in set(caps):
        assert any(top(i) for i in range(c["nbits"]) if caps[i] == cap), (name, cap)
    if name.startswith("bits_ucap"):
        C = int(name.split("_c")[1].split("_")[0])
        assert d["kernel"] == "decrypt_bits_kernel" and d["ucap"] == C and caps == [C] * c["nbits"]
        total = c["n"] * c["nbits"]
        if "16byte" in name:  # 384 bits: a whole block of four waves and half of the next
            assert c["nbits"] == 128 and total == 384 and d["blocks"] == 2 and not d["partial_wave"]
        else:  # 8, 24, 72 bits: below one wave, and one wave + 8 bits
            assert total == {1: 8, 3: 24, 9: 72}[c["n"]] and d["partial_wave"]
    elif name == "bits_general_16byte_caps1_32_n3":
        # both HM_MAX_BITS LDS arrays (bounds, offsets) full; the last capacity of the kernel
        assert d["kernel"] == "decrypt_bits_kernel" and d["ucap"] == 0 and c["nbits"] == 128
        assert set(caps) == set(range(1, 33)) and max(caps) == cp.DEC_BITS_MAXCAP
    elif name == "wave_16byte_wide_n5":
        assert d["kernel"] == "decrypt_kernel" and d["partial_block"] and d["blocks"] == 2
        assert {caps[i] for i in DEC_WIDE_BITS} == {193, 255, 256, 257, 449, 512, 513}
        assert max(caps[i] for i in range(128) if i not in DEC_WIDE_BITS) == 4
        # (lanes entering the unrolled body, its rounds on lane 0, tail rounds on lanes 0 and 63)
        assert [cp.dec_wave_trace(caps[i]) for i in sorted(DEC_WIDE_BITS)] == [
            (1, 1, 0, 3), (63, 1, 0, 3), (64, 1, 0, 0), (64, 1, 1, 0), (64, 2, 0, 3),
            (64, 2, 0, 0), (64, 2, 1, 0)]
        assert cp.dec_wave_trace(4) == (0, 0, 1, 0)
        # bits 0 .. 63 go to m0 and 64 .. 127 to m1: wide bits on both sides of the seam, with
        # FULL, ONES and MONO polynomials at the top coefficient of each
        for i in (0, 63, 64, 127):
            kinds = {kind_of(e, i) for e in range(c["n"])}
            assert {"FULL", "ONES", "MONO"} <= kinds, (i, kinds)
            b = int(c["ba"][i])
            assert any(v[i] == 1 << b for v in c["A"]) and any(v[i] == (1 << (b + 1)) - 1 for v in c["A"])
        assert all(top(i) for i in DEC_WIDE_BITS)
    elif name == "wave_u8_cap512_n6":
        assert d["kernel"] == "decrypt_kernel" and d["partial_block"] and caps == [512] * 8
        assert cp.dec_wave_trace(512) == (64, 2, 0, 0) and all(top(i) for i in range(8))
    else:
        raise KeyError(name)
    return d
