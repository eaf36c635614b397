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

The second half of the module holds the families of the wave-per-value circuits that came after
the tier (select, minmax, lookup, shift, count, array): their case tables, a third operand where
the operation has one, their references (the big-integer models of tests/*_model.py), traces that
replay each kernel's own sequence of products on the model integers, and path assertions that
take every slot size from the plan drivers tests/sanitize/*_plan.cpp.
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
    if family in _WAVE_FAMILIES:  # select, minmax, lookup, shift: a third operand where there is one
        return _WAVE_FAMILIES[family](name)
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
    """The case's operands in the batch layout: (la, da, lb, db), then (lc, dc) where the case has
    a third operand (select's condition: inputs()["C"], ["bc"])."""
    c = inputs(family, name)
    out = bm.pack(c["A"], c["ba"]) + bm.pack(c["B"], c["bb"])
    return out + bm.pack(c["C"], c["bc"]) if "C" in c else out


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
    # mul_plan.h column_walk takes the prefix as U then)
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


# =============================================================================================
# The wave-per-value circuits added after the tier: select, min / max, lookup, shift (kernels.hip).
# All go through wave_mul<kQSmall = 10, 8>(U, nu, V, nv, Add, nadd, Dst): nout = max(nu + nv, nadd)
# words, tile width W = ceil(nout / 64) up to 8, MULTI tiles past 512 words, U read in chunks of 10.
# The traces below replay each kernel's own sequence of products on the model integers.
import lookup_model as lm  # noqa: E402
import select_model as sm  # noqa: E402
import shift_model as shm  # noqa: E402

LDS_WORDS = 10240  # a wave's share of a CU's LDS (circuit_host.h fits_cu_lds)


def wob(b):
    """words_of_bound: the words of a polynomial of degree b."""
    return int(b) // 32 + 1


def product_shape(nu, nv, nadd=0):
    """wave_mul's own sizes: (nout, tile width W, tiles, uniform chunks of kQSmall words)."""
    nout = max(nu + nv, nadd)
    w = max(1, min(8, (nout + 63) // 64))
    return nout, w, max(1, (nout + 64 * w - 1) // (64 * w)), (nu + 9) // 10


def deg(p):
    return p.bit_length() - 1


def _reaches(vals, ob, bits=None):
    """At every output bit some value has degree equal to the output bound."""
    for i in (range(len(ob)) if bits is None else bits):
        assert max(deg(v[i]) for v in vals) == int(ob[i]), (i, int(ob[i]))


# ------------------------------------------------------------------ the plan drivers
@functools.lru_cache(maxsize=None)
def _plan_driver(name):
    """tests/sanitize/<name>_plan.cpp, the planner header compiled alone into an ASan + UBSan
    driver (as test_circuit_plans.py and its siblings build it), once per process."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.path.join(root, "tests", "sanitize", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, f"{name}_plan_{os.getpid()}")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(root, "tests", "sanitize", f"{name}_plan.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    import atexit
    atexit.register(lambda: os.path.exists(exe) and os.remove(exe))
    return exe


@functools.lru_cache(maxsize=None)
def _plan(name, line):
    """The driver's JSON rows for one case line given on stdin."""
    import json
    import os
    import subprocess
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([_plan_driver(name)], input=line + "\n", capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return [json.loads(x) for x in r.stdout.splitlines()]


def _ints(x):
    return " ".join(str(int(v)) for v in x)


def select_plan(cb, ba, bb):
    """plan_select through tests/sanitize/circuit_plan.cpp."""
    return _plan("circuit", f"select {len(ba)} {int(cb)} {_ints(ba)} {_ints(bb)}")[1]


def minmax_plan(ba, bb):
    """hm_minmax_batch's plan_borrow (chain = wb_L) through tests/sanitize/circuit_plan.cpp."""
    return _plan("circuit", f"minmax {len(ba)} 0 {_ints(ba)} {_ints(bb)}")[1]


def lookup_plan(k, ab, table):
    """plan_lookup through tests/sanitize/lookup_plan.cpp (its first row; the driver's own closing
    case follows)."""
    t = np.asarray(table)
    raw = np.ascontiguousarray(t.astype(t.dtype.newbyteorder("<"))).view(np.uint8).reshape(-1)
    return _plan("lookup", f"{k} {t.dtype.itemsize} {_ints(ab[:k])} {raw.tobytes().hex()}")[0]


SHIFT_CODES = {"shl": 18, "shr": 19, "rotl": 20, "rotr": 21}


def shift_plan(op, signed, ba, bs):
    """plan_shift through tests/sanitize/shift_plan.cpp (its first row)."""
    L = shm.stages(len(ba))
    return _plan("shift", f"{SHIFT_CODES[op]} {int(signed)} {len(ba)} {_ints(ba)} {_ints(bs[:L])}")[0]


# ------------------------------------------------------------------ select
def _per_bit_select():
    i = np.arange(8)
    return u32(64 * i + 63), u32(1000 - 97 * i)


SELECT_CASES = {
    # name: (condition bound, a bounds, b bounds)
    "w1_edge": (1023, uniform(8, 1023), uniform(8, 1023)),
    "w2_edge": (1023, uniform(8, 1055), uniform(8, 1055)),
    "one_tile": (8191, uniform(8, 8191), uniform(8, 8191)),
    "multi_tile": (8191, uniform(8, 8223), uniform(8, 8223)),
    "chunks_10_11": (500, uniform(8, 319), uniform(8, 320)),
    "chunks_20_21": (500, uniform(8, 639), uniform(8, 640)),
    "lopsided": (9000, uniform(8, 40), uniform(8, 40)),
    "lopsided_swapped": (40, uniform(8, 9000), uniform(8, 9000)),
    "per_bit": (500,) + _per_bit_select(),
}
COND_SHIFT = 5  # the condition of value e < 8 is of kind (e + 5) mod 8


def _bool_batch(polys, cb):
    """A Ciphered<bool> batch in model form: bit 0 the polynomial, bits 1..7 null at bound 0."""
    return [[p] + [0] * 7 for p in polys], u32([int(cb)] + [0] * 7)


def _select_inputs(name):
    cb, ba, bb = SELECT_CASES[name]
    seed = _seed("select", name)
    rng = np.random.default_rng(seed + 9)
    A, B = operands(ba, 8, seed, 0), operands(bb, 8, seed + 1, 3)
    C = [poly(KINDS[(e + COND_SHIFT) % 8], cb, rng) for e in range(8)]
    # a FULL against b one below its bound, and the other way round: x_i keeps the wider bound
    PA, PB = full_pair(ba, bb, 1, seed + 2)
    QB, QA = full_pair(bb, ba, 1, seed + 3)
    A, B, C = A + PA + QA, B + PB + QB, C + [_exact(rng, int(cb)), _exact(rng, int(cb))]
    if name == "per_bit":
        # b_i as long as both bounds allow and a_i = b_i + one word: x_i is one word, so under a
        # UNIT or a one-word condition the product is shorter than the b_i it is added to
        for c in (1, _exact(rng, 20)):
            bv = [_exact(rng, int(min(x, y))) for x, y in zip(ba, bb)]
            A.append([p ^ _exact(rng, 17) for p in bv])
            B.append(bv)
            C.append(c)
    Cv, bc = _bool_batch(C, cb)
    return dict(ba=u32(ba), bb=u32(bb), bc=bc, A=A, B=B, C=Cv, n=len(A), nbits=len(ba))


@functools.lru_cache(maxsize=None)
def select_reference(name):
    """(out bounds, values, limbs, degree words) of select_model.select_circuit on the case."""
    c = inputs("select", name)
    ob = sm.select_bounds(c["bc"][0], c["ba"], c["bb"])
    vals = [sm.select_circuit(cv[0], a, b) for cv, a, b in zip(c["C"], c["A"], c["B"])]
    return (ob, vals) + _frozen(*bm.pack(vals, ob))


def select_trace(c, a, b):
    """Per bit of one value, as select_kernel runs it: wave_mul(X, nx, C, nc, Bb, nb, T) -- x_i is
    the uniform operand, the condition the per-lane one, b_i is added."""
    rows = []
    for i, (x, y) in enumerate(zip(a, b)):
        nx, nc, nb = words(x ^ y), words(c), words(y)
        nout, w, tiles, chunks = product_shape(nx, nc, nb)
        rows.append(dict(i=i, na=words(x), nb=nb, nx=nx, nc=nc, nout=nout, w=w, tiles=tiles,
                         chunks=chunks, live=bool(nx and nc)))
    return rows


def check_select_path(name):
    """The path each select case is named for, and that the case fills its bounds and its slots
    (plan_select's, from the plan driver)."""
    c = inputs("select", name)
    cb = int(c["bc"][0])
    tr = [select_trace(cv[0], a, b) for cv, a, b in zip(c["C"], c["A"], c["B"])]
    rows = [r for t in tr for r in t]
    live = [r for r in rows if r["live"]]
    top = max(live, key=lambda r: r["nx"] + r["nc"])
    nprod = top["nx"] + top["nc"]
    if name == "w1_edge":
        assert nprod == 64 and (top["w"], top["tiles"]) == (1, 1)
    elif name == "w2_edge":
        assert nprod == 65 and (top["w"], top["tiles"]) == (2, 1)
    elif name == "one_tile":
        assert nprod == 512 and (top["w"], top["tiles"]) == (8, 1)
    elif name == "multi_tile":
        assert nprod == 513 and (top["w"], top["tiles"]) == (8, 2)
    elif name in ("chunks_10_11", "chunks_20_21"):
        lo = 10 if name == "chunks_10_11" else 20
        assert {lo, lo + 1} <= {r["nx"] for r in live}
        assert {lo // 10, lo // 10 + 1} <= {r["chunks"] for r in live}
    elif name == "lopsided":
        assert max(r["nx"] for r in live) == 2 and max(r["nc"] for r in live) == 282
    elif name == "lopsided_swapped":
        assert max(r["nx"] for r in live) == 282 and (282 + 9) // 10 == 29
        assert max(r["nc"] for r in live) == 2
    elif name == "per_bit":
        ca, cbb = c["ba"] // 64 + 1, c["bb"] // 64 + 1
        assert len(set(ca.tolist())) == 8 and len(set(cbb.tolist())) == 8
        for i in range(8):  # every bit's slot is filled by some value
            assert max(t[i]["na"] for t in tr) == wob(c["ba"][i])
            assert max(t[i]["nb"] for t in tr) == wob(c["bb"][i])
        # the product shorter than what it is added to: nout = nadd
        short = [r for r in live if r["nb"] > r["nx"] + r["nc"]]
        assert {r["i"] for r in short} == set(range(1, 8))  # (bit 0's b_0 has two words itself)
        assert all(r["nout"] == r["nb"] for r in short)
    else:
        raise KeyError(name)
    # the condition's kinds over the values: NULL has a null product over nout = max(nx, nb)
    # words, an exact copy of b_i; UNIT has nc = 1
    kinds = [KINDS[(e + COND_SHIFT) % 8] for e in range(8)]
    e0, e1 = kinds.index("NULL"), kinds.index("UNIT")
    ob, vals, _, _ = select_reference(name)
    assert all(r["nc"] == 0 and r["nout"] == max(r["nx"], r["nb"]) and not r["live"] for r in tr[e0])
    assert vals[e0] == c["B"][e0] and any(r["nx"] > r["nb"] for r in tr[e0])
    assert all(r["nc"] == 1 for r in tr[e1])
    # fills: every output bound, and every slot of the plan to the last word its bound allows
    _reaches(vals, ob)
    p = select_plan(cb, c["ba"], c["bb"])
    assert p["status"] == 0 and p["lds_per_wave"] <= LDS_WORDS
    nc, na, nb, nx = (max(r[k] for r in rows) for k in ("nc", "na", "nb", "nx"))
    assert nc == wob(cb) and 0 <= p["SC"] - nc <= 1
    assert na == wob(c["ba"].max()) and 0 <= p["SA"] - na <= 1
    assert nb == wob(c["bb"].max()) and 0 <= p["SB"] - nb <= 1
    assert nx == max(na, nb) and 0 <= p["SX"] - nx <= 1
    tcap = p["lds_per_wave"] - p["oT"]  # the product buffer: SC + SX + 2 words
    assert tcap == p["SC"] + p["SX"] + 2 and nprod == nc + nx and nprod <= tcap
    assert max(r["nout"] for r in rows) <= tcap
    return dict(nprod=nprod, plan=p, rows=rows)


# ------------------------------------------------------------------ min / max
MINMAX_OWN = {
    # name: (a bounds, b bounds, scheduled + random values, FULL / bound - 1 pairs)
    "p2_one_tile": (uniform(8, 1632), uniform(8, 1632), 8, 2),
    "p2_multi_tile": (uniform(8, 1636), uniform(8, 1636), 8, 2),
    "null_borrow": (uniform(8, 255), uniform(8, 255), 0, 2),
}
MINMAX_CASES = tuple(BORROW_CASES) + tuple(MINMAX_OWN)


def _minmax_inputs(name):
    if name in BORROW_CASES:
        c = dict(inputs("borrow", name))
        if (c["ba"] != c["bb"]).all():
            # full_pair's b_i, one below its bound, leaves p_i short wherever bb_i > ba_i; with
            # no two bounds equal nothing cancels, and one all-FULL value takes w_n to its bound
            rng = np.random.default_rng(_seed("minmax", name))
            c["A"] = c["A"] + [[_exact(rng, int(b)) for b in c["ba"]]]
            c["B"] = c["B"] + [[_exact(rng, int(b)) for b in c["bb"]]]
            c["n"] += 1
        return c
    ba, bb, ns, npair = MINMAX_OWN[name]
    seed = _seed("minmax", name)
    A, B = batch(ba, bb, ns, npair, seed)
    if name == "null_borrow":
        # w_{i+1} = (a_i + 1) b_i + p_i w_i stays null when every b_i is null or every a_i is the
        # unit: a = b bit for bit over {0, 1} (x_i null as well), then b null under a of every kind
        pat = [[(v >> i) & 1 for i in range(8)] for v in (0x00, 0xFF, 0xA5)]
        A = [list(p) for p in pat] + operands(ba, 3, seed + 6, 0) + A
        B = [list(p) for p in pat] + [[0] * 8 for _ in range(3)] + B
    return dict(ba=u32(ba), bb=u32(bb), A=A, B=B, n=len(A), nbits=len(ba))


@functools.lru_cache(maxsize=None)
def minmax_reference(name, op, signed=False):
    """op "min" or "max": (out bounds, values, limbs, degree words) of select_model's circuits."""
    c = inputs("minmax", name)
    ob = sm.minmax_bounds(c["ba"], c["bb"])
    f = sm.min_circuit if op == "min" else sm.max_circuit
    vals = [f(a, b, signed) for a, b in zip(c["A"], c["B"])]
    return (ob, vals) + _frozen(*bm.pack(vals, ob))


def minmax_trace(a, b, is_max=False, signed=False):
    """minmax_kernel's phase 2 on one value: wave_mul(X, nx, W, nw, is_max ? Ab : Bb, .., Wn) with
    W = w_n, the last borrow of phase 1 (borrow_trace is phase 1)."""
    w = sm.less_than(a, b, signed)
    rows = []
    for i, (x, y) in enumerate(zip(a, b)):
        nx, nw, nadd = words(x ^ y), words(w), words(x if is_max else y)
        nout, tw, tiles, chunks = product_shape(nx, nw, nadd)
        rows.append(dict(i=i, nx=nx, nw=nw, nadd=nadd, nout=nout, w=tw, tiles=tiles,
                         chunks=chunks, live=bool(nx and nw)))
    return rows


def check_minmax_path(name):
    """Phase 2 of minmax_kernel (phase 1 is borrow_step: check_borrow_path) in plan_borrow's layout
    with chain = wb_L: the product x_i w_n goes to a borrow buffer of cw words."""
    c = inputs("minmax", name)
    tr = [minmax_trace(a, b) for a, b in zip(c["A"], c["B"])]
    rows = [r for t in tr for r in t]
    live = [r for r in rows if r["live"]]
    top = max(live, key=lambda r: r["nx"] + r["nw"])
    nprod = top["nx"] + top["nw"]
    if name == "p2_one_tile":
        assert (top["nx"], top["nw"], nprod) == (52, 460, 512) and (top["w"], top["tiles"]) == (8, 1)
    elif name == "p2_multi_tile":
        assert (top["nx"], top["nw"], nprod) == (52, 461, 513) and (top["w"], top["tiles"]) == (8, 2)
    elif name == "null_borrow":
        null = [t for t in tr if all(r["nw"] == 0 for r in t)]
        assert len(null) == 6
        # ... x_i null too (three values) and x_i of every kind under the null borrow (three)
        assert sum(all(r["nx"] == 0 for r in t) for t in null) >= 2
        assert any(r["nx"] == 8 for t in null for r in t)
        assert all(r["nout"] == max(r["nx"], r["nadd"]) and not r["live"] for t in null for r in t)
        for op in ("min", "max"):  # min copies b, max copies a
            _, vals, _, _ = minmax_reference(name, op)
            src = c["B"] if op == "min" else c["A"]
            assert vals[:6] == src[:6]
    elif name == "u16_per_bit":
        assert nprod > 512 and top["tiles"] == 2
    elif name not in BORROW_CASES:
        raise KeyError(name)
    # fills.  Bit 0 with ba_0 = bb_0 cannot: w_n at its bound needs a_0 and b_0 both at theirs (the
    # first borrow a_0 b_0 + b_0), and then the tops cancel in x_0: one below the bound there
    ob, vals, _, _ = minmax_reference(name, "min")
    rest = range(int(c["ba"][0] == c["bb"][0]), c["nbits"])
    _reaches(vals, ob, rest)
    _reaches(minmax_reference(name, "max")[1], ob, rest)
    if c["ba"][0] == c["bb"][0]:
        assert max(deg(v[0]) for v in vals) == int(ob[0]) - 1
    p = minmax_plan(c["ba"], c["bb"])
    assert p["status"] == 0 and p["lds_per_wave"] <= LDS_WORDS
    chain = bm.borrow_bounds(c["ba"], c["bb"], c["nbits"])[-1]
    assert p["chain"] == chain and max(r["nw"] for r in rows) == wob(chain)
    nx = max(r["nx"] for r in rows)
    assert nx == wob(max(c["ba"].max(), c["bb"].max())) and 0 <= p["SX"] - nx <= 1
    # the borrow buffer holds the widest product and is filled to the last word the bounds allow
    assert nprod == nx + wob(chain) and p["cw"] - 2 - nprod == p["SX"] - nx
    assert max(r["nout"] for r in rows) <= p["cw"]
    return dict(nprod=nprod, plan=p, rows=rows)


# ------------------------------------------------------------------ lookup
def _lk(k, ab, nbits=8, dtype=np.uint8):
    ab = list(ab) + [63] * (nbits - len(ab))  # the bits above the index are not read
    return dict(k=k, ab=u32(ab), dtype=np.dtype(dtype))


LOOKUP_CASES = {
    "w1_edge": _lk(2, [1023, 1023]),
    "w2_edge": _lk(2, [1023, 1055]),
    "one_tile": _lk(8, [2040] * 8),
    "multi_tile": _lk(8, [2040] * 7 + [2072]),
    "chunks_319": _lk(4, [319] * 4),
    "chunks_320": _lk(4, [320] * 4),
    "chunks_639": _lk(4, [639] * 4),
    "chunks_640": _lk(4, [640] * 4),
    "odd_split_per_bit": _lk(5, [63 + 97 * i for i in range(5)], nbits=16),
    "wide_out": _lk(3, [700] * 3, dtype=np.uint32),
}
LOOKUP_TABLES = ("all", "top", "random")


def lookup_table(name, which):
    """all: t[0] = 1 (all output bits of t[0] for wide_out, so that every one of its 32 bits has an
    accumulator), every ANF coefficient set; top: t[2^k - 1] alone, the top monomial only; random:
    seeded."""
    spec = LOOKUP_CASES[name]
    E, dt = 1 << spec["k"], spec["dtype"]
    t = np.zeros(E, dtype=dt)
    one = np.iinfo(dt).max if name == "wide_out" else 1
    if which == "all":
        t[0] = one
    elif which == "top":
        t[E - 1] = one
    else:
        rng = np.random.default_rng(_seed("lookup", name) + 77)
        t = rng.integers(0, np.iinfo(dt).max, size=E, dtype=dt, endpoint=True)
    t.setflags(write=False)
    return t


def _lookup_inputs(name):
    spec = LOOKUP_CASES[name]
    seed = _seed("lookup", name)
    rng = np.random.default_rng(seed + 3)
    A = operands(spec["ab"], 8, seed, 0)
    A += [[_exact(rng, int(b)) for b in spec["ab"]] for _ in range(2)]  # products never cancel
    return dict(ba=spec["ab"], bb=spec["ab"], A=A, B=A, n=len(A), nbits=len(spec["ab"]), k=spec["k"])


@functools.lru_cache(maxsize=None)
def _model_monomials(name):
    c = inputs("lookup", name)
    return [lm.monomials(a, c["k"]) for a in c["A"]]


@functools.lru_cache(maxsize=None)
def lookup_reference(name, which):
    """(out bounds, values, limbs, degree words): lookup_model's circuit, out_j = the XOR of its
    monomials (lookup_model.monomials, made once per case) over the table's coefficient masks
    (lookup_model.moebius)."""
    c = inputs("lookup", name)
    t = lookup_table(name, which)
    ob = lm.lookup_bounds(c["ba"], t)
    vals = []
    for M in _model_monomials(name):
        out = []
        for f in lm.moebius(t):
            p = 0
            for S, on in enumerate(f):
                if on:
                    p ^= M[S]
            out.append(p)
        vals.append(out)
    return (ob, vals) + _frozen(*bm.pack(vals, ob))


def lookup_trace(a, k, masks, need):
    """lookup_kernel on one value: the monomials of the low kl and the high kh index bits by
    doubling on the top bit (M[s | 1 << i] = a_i M[s], a_i uniform, only those in the plan's need
    mask), then per output bit the accumulate P <- MH[t] I_jt + P.  Returns (mono: id -> words,
    dbl: the doubling products' (id, nb, nm), acc: the accumulate products' dicts, out)."""
    kl = (k + 1) // 2
    kh = k - kl
    M = {0: 1, 16: 1}
    dbl = []
    for h, kk, base in ((0, kl, 0), (16, kh, kl)):
        for i in range(kk):
            M[h + (1 << i)] = a[base + i]
        for i in range(1, kk):
            for s in range(1, 1 << i):
                mid = h + (1 << i) + s
                if not (need >> mid) & 1:
                    continue
                u, v = M[h + (1 << i)], M[h + s]
                M[mid] = model.clmul_fast(u, v)
                dbl.append((mid, words(u), words(v)))
    acc, out = [], []
    for j, mask in enumerate(masks):
        p = 0
        for t in range(1 << kh):
            m = (mask >> (t << kl)) & ((1 << (1 << kl)) - 1)
            if not m:
                continue
            inner = 0
            for s in range(1 << kl):
                if (m >> s) & 1:
                    inner ^= M[s]
            if t == 0:
                p = inner
                continue
            nh = words(M[16 + t])
            if not nh or not inner:
                continue
            nout, w, tiles, chunks = product_shape(nh, words(inner), words(p))
            acc.append(dict(j=j, t=t, nh=nh, ni=words(inner), np=words(p), nout=nout, w=w,
                            tiles=tiles, chunks=chunks))
            p ^= model.clmul_fast(M[16 + t], inner)
        out.append(p)
    return {s: words(p) for s, p in M.items()}, dbl, acc, out


@functools.lru_cache(maxsize=None)
def lookup_traces(name, which):
    c = inputs("lookup", name)
    t = lookup_table(name, which)
    p = lookup_plan(c["k"], c["ba"], t)
    assert p["status"] == 0, p
    masks = lm.coefficient_masks(t)
    assert [int(x, 16) for x in p["masks"]] == masks
    return p, [lookup_trace(a, c["k"], masks, p["need"]) for a in c["A"]]


def check_lookup_path(name):
    """The path each lookup case is named for, on the "all" table (every monomial in use) unless
    noted; plan_lookup's slots (off[], cI, cP) from the plan driver, each filled."""
    c = inputs("lookup", name)
    k, ab = c["k"], [int(x) for x in c["ba"][:c["k"]]]
    kl = (k + 1) // 2
    kh = k - kl
    p, tr = lookup_traces(name, "all")
    assert (p["kl"], p["kh"]) == (kl, kh) and p["lds_per_wave"] <= LDS_WORDS
    acc = [r for _, _, a, _ in tr for r in a]
    dbl = [r for _, d, _, _ in tr for r in d]
    top = max(acc, key=lambda r: r["nh"] + r["ni"])
    nprod = top["nh"] + top["ni"]
    if name == "w1_edge":
        assert (top["nh"], top["ni"]) == (32, 32) and (top["w"], top["tiles"]) == (1, 1)
    elif name == "w2_edge":
        assert (top["nh"], top["ni"]) == (33, 32) and (top["w"], top["tiles"]) == (2, 1)
    elif name == "one_tile":
        assert (top["nh"], top["ni"]) == (256, 256) and (top["w"], top["tiles"]) == (8, 1)
    elif name == "multi_tile":
        assert (top["nh"], top["ni"]) == (257, 256) and (top["w"], top["tiles"]) == (8, 2)
    elif name.startswith("chunks_"):
        nu = {"chunks_319": 10, "chunks_320": 11, "chunks_639": 20, "chunks_640": 21}[name]
        assert max(r[1] for r in dbl) == nu and (nu + 9) // 10 == {10: 1, 11: 2, 20: 2, 21: 3}[nu]
    elif name == "odd_split_per_bit":
        assert (kl, kh) == (3, 2)
        sizes = [b - a for a, b in zip(sorted(set(p["off"]))[1:], sorted(set(p["off"]))[2:])]
        assert len(set(sizes)) >= 6  # distinct slot sizes
        # the `need` mask: all 8 + 4 monomials under the all and the random table; under the top
        # table only each half's top monomial and the chain it is formed from (s without its top
        # bit), so the doubling's `continue` is taken
        pr, pt = lookup_traces(name, "random")[0], lookup_traces(name, "top")[0]
        assert pr["need"] == p["need"] == 0x000F00FF
        assert pt["need"] == 0x000B008B, hex(pt["need"])  # low 7 <- 3 <- 1 <- 0, high 3 <- 1 <- 0
    elif name == "wide_out":
        assert len(tr[-1][3]) == 32 and {r["j"] for r in acc} == set(range(32))
        assert all(sum(1 for r in a if r["j"] == j) == (1 << kh) - 1 for j in range(32)
                   for a in (tr[-1][2],))  # P / Pn exchanged an odd number of times per bit
    else:
        raise KeyError(name)
    # the index bits' kinds: a NULL bit nulls every monomial above it (skipped on `!nh` or on a
    # null inner sum), a UNIT bit makes its product a copy
    assert any(w == 0 for mono, _, _, _ in tr[:8] for s, w in mono.items() if s not in (0, 16))
    assert any(nb == 1 or nm == 1 for _, nb, nm in dbl) or k == 2
    # fills: the output bounds, then every slot of the plan
    for which in ("all", "top"):
        ob, vals, _, _ = lookup_reference(name, which)
        used = [j for j in range(len(ob)) if any(lm.moebius(lookup_table(name, which))[j])]
        _reaches(vals, ob, used)
    offs = sorted(set(p["off"]) | {p["oI"]})
    for s in range(1, 32):
        if not (p["need"] >> s) & 1 or s in (0, 16):
            continue
        bits = [(0 if s < 16 else kl) + i for i in range(4) if ((s & 15) >> i) & 1]
        if s < 16 and not all(i < kl for i in bits) or s >= 16 and not all(i < k for i in bits):
            continue
        bound = sum(ab[i] for i in bits)
        slot = offs[offs.index(p["off"][s]) + 1] - p["off"][s]
        got = max(mono.get(s, 0) for mono, _, _, _ in tr)
        assert got == wob(bound) and got <= slot <= got + 3, (s, got, slot)
    cI = max(r["ni"] for r in acc)
    cH = max(r["nh"] for r in acc)
    assert cI == p["cI"] == wob(sum(ab[:kl])) and cH == wob(sum(ab[kl:]))
    assert p["oP"] - p["oI"] >= cI and nprod == cI + cH and 0 <= p["cP"] - 2 - nprod <= 1
    assert p["lds_per_wave"] == p["oP"] + 2 * p["cP"]
    return dict(nprod=nprod, plan=p)


# ------------------------------------------------------------------ shift
def _sh(bs, ba, params=PARAMS):
    bs = list(bs) + [0] * (8 - len(bs))  # the amount is a u8 batch; its low log2 n bits are read
    return dict(bs=u32(bs), ba=u32(ba), params=params)


SHIFT_CASES = {
    "w1_edge": _sh([255] * 3, [1279] * 8),
    "w2_edge": _sh([255] * 3, [1311] * 8),
    "one_tile": _sh([255] * 3, [15615] * 8),
    "multi_tile": _sh([255] * 3, [15647] * 8),
    "chunks": _sh([319, 320, 639], [200 + 7 * i for i in range(8)]),
    # (64 i + 63 up to bit 4, then down again: ascending bounds alone would give every SHR slot
    # the same suffix maximum)
    "per_bit": _sh([63, 700, 320], [63, 191, 319, 447, 511, 383, 255, 127]),
    "stage_subsets": _sh([255] * 3, [300 + 5 * i for i in range(8)]),
    "u32_headline_shape": _sh([256] * 5, [256] * 32, DEC_PARAMS),
}
AMOUNT_SHIFT = 5  # amount bit t of value e < 8 is of kind (e + t + 5) mod 8


def _shift_inputs(name):
    spec = SHIFT_CASES[name]
    ba, bs = spec["ba"], spec["bs"]
    n, L = len(ba), shm.stages(len(ba))
    seed = _seed("shift", name)
    rng = np.random.default_rng(seed + 4)
    full_s = lambda: [_exact(rng, int(bs[t])) if t < L else 0 for t in range(8)]  # noqa: E731
    if name == "stage_subsets":  # value e: s_t null iff bit t of e is clear; FULL otherwise
        A = [[_exact(rng, int(b)) for b in ba] for _ in range(8)]
        S = [[_exact(rng, int(bs[t])) if (e >> t) & 1 else 0 for t in range(L)] + [0] * (8 - L)
             for e in range(8)]
    else:
        A = operands(ba, 8, seed, 0)
        S = [[poly(kind_of(e, t, AMOUNT_SHIFT), bs[t], rng) if t < L else 0 for t in range(8)]
             for e in range(8)]
    if len(set(ba.tolist())) == 1:
        # equal tops cancel: an output's top coefficient is the parity of the FULL bits among its
        # sources, so one bit FULL and the others one below -- bit 0 (shl, the rotates), the top
        # bit (shr) and the one below it (the arithmetic shr, whose top bit stays a_{n-1} itself)
        for hot in (0, n - 1, n - 2):
            A.append([_exact(rng, int(b) - (i != hot)) for i, b in enumerate(ba)])
            S.append(full_s())
    else:
        for _ in range(2):
            A.append([_exact(rng, int(b)) for b in ba])
            S.append(full_s())
    return dict(ba=ba, bb=bs, A=A, B=S, n=len(A), nbits=n, L=L, params=spec["params"])


@functools.lru_cache(maxsize=None)
def shift_reference(name, op, signed=False):
    """(out bounds, values, limbs, degree words) of shift_model.shift_circuit (stages ascending)."""
    c = inputs("shift", name)
    ob = shm.shift_bounds(op, c["ba"], c["bb"])
    vals = [shm.shift_circuit(op, a, s, signed) for a, s in zip(c["A"], c["B"])]
    return (ob, vals) + _frozen(*bm.pack(vals, ob))


def shift_trace(op, signed, a, s):
    """shift_kernel on one value: the stages from the widest step down to `last`, the lowest t
    whose s_t is not null, null stages skipped; per product wave_mul(S, ns, V, nv, xi, ni, T) with
    V = x_i + x_src (x_i alone where the source is null).  Every stage but `last` rewrites the
    slots; a rotate saves the 2^t bits that wrap first.  Returns (last, rows, slot: the widest
    content of each slot, saved: t -> the widest saved bit, out)."""
    n = len(a)
    L = shm.stages(n)
    x = list(a)
    slot = [words(p) for p in x]
    saved, rows = {}, []
    live = [t for t in range(L) if s[t]]
    last = live[0] if live else -1
    if last < 0:
        return last, rows, slot, saved, x
    for t in range(L - 1, last - 1, -1):
        if not s[t]:
            continue
        k, fin = 1 << t, t == last
        if op in ("rotl", "rotr") and not fin:
            wrap = x[n - k:] if op == "rotl" else x[:k]
            saved[t] = max(words(p) for p in wrap)
        y = []
        for i in range(n):
            j = shm.source(op, n, k, i, signed)
            v = x[i] ^ (x[j] if j is not None else 0)
            nout, w, tiles, chunks = product_shape(words(s[t]), words(v), words(x[i]))
            rows.append(dict(t=t, i=i, fin=fin, ns=words(s[t]), nv=words(v), ni=words(x[i]),
                             nout=nout, w=w, tiles=tiles, chunks=chunks))
            y.append(x[i] ^ model.clmul_fast(s[t], v))
        x = y
        if not fin:
            slot = [max(q, words(p)) for q, p in zip(slot, x)]
    return last, rows, slot, saved, x


@functools.lru_cache(maxsize=None)
def shift_traces(name, op, signed=False):
    c = inputs("shift", name)
    return [shift_trace(op, signed, a, s) for a, s in zip(c["A"], c["B"])]


def check_shift_path(name, op, signed=False):
    """The path each shift case is named for, in one mode; plan_shift's slots (off[], the X / T
    buffers, the rotates' save area sv[t]) from the plan driver, each filled as far as a value in
    LDS can fill it (the final stage's products go from T to the output, not to a slot)."""
    c = inputs("shift", name)
    n, L = c["nbits"], c["L"]
    ba, bs = [int(b) for b in c["ba"]], [int(b) for b in c["bb"][:L]]
    tr = shift_traces(name, op, signed)
    rows = [r for _, rs, _, _, _ in tr for r in rs]
    fin0 = [r for r in rows if r["fin"] and r["t"] == 0]
    top = max(fin0, key=lambda r: r["ns"] + r["nv"])
    nprod = top["ns"] + top["nv"]
    edge = {"w1_edge": (8, 56, 1, 1), "w2_edge": (8, 57, 2, 1), "one_tile": (8, 504, 8, 1),
            "multi_tile": (8, 505, 8, 2)}
    if name in edge:
        assert (top["ns"], top["nv"], top["w"], top["tiles"]) == edge[name]
    elif name == "chunks":
        assert {t: max(r["ns"] for r in rows if r["t"] == t) for t in range(3)} == {0: 10, 1: 11, 2: 20}
        assert {r["chunks"] for r in rows} >= {1, 2}
    elif name == "stage_subsets":
        assert [t[0] for t in tr[:8]] == [-1, 0, 1, 0, 2, 0, 1, 0]
        assert {r["t"] for r in tr[5][1]} == {0, 2}  # the middle stage skipped
        assert tr[0][4] == c["A"][0]  # the null amount: the copy-out
    elif name == "u32_headline_shape":
        assert (n, L) == (32, 5) and {r["t"] for r in rows} == set(range(5))
    elif name != "per_bit":
        raise KeyError(name)
    ob, vals, _, _ = shift_reference(name, op, signed)
    if signed:
        # an arithmetic shr keeps its top bit, out_{n-1} = a_{n-1}, and bit j takes a_{n-1} under
        # the sum of j + 1 amount indicators, whose common top term cancels when j + 1 is even: the
        # bound is out of reach there unless a bit below the top one is as wide
        assert all(v[n - 1] == a[n - 1] for v, a in zip(vals, c["A"]))
        _reaches(vals, ob, [j for j in range(n - 1) if j % 2 == 0 or max(ba[j:n - 1]) >= ba[n - 1]])
    else:
        _reaches(vals, ob)
    p = shift_plan(op, signed, ba, bs)
    assert p["status"] == 0 and p["lds_per_wave"] <= LDS_WORDS and p["bounds"] == ob.tolist()
    sizes = [b - a for a, b in zip(p["off"], p["off"][1:] + [p["cV"]])]
    widest = p["oT"] - p["oX"]
    assert widest == p["oS"] - p["oT"] == max(sizes)
    # T and X: the widest product (the final stage's: its factors' words, one more than the
    # result's when the top word stays empty) reaches the last word the widest bound allows
    assert wob(max(ob)) <= max(r["nout"] for r in rows) <= wob(max(ob)) + 1 <= widest
    assert widest - wob(max(ob)) <= 2
    # a slot holds what the stages above stage 0 leave in it (the last stage's products go from T
    # to the output): the bounds through those stages, bit by bit
    reach = list(ba)
    for t in range(L - 1, 0, -1):
        src = [shm.source(op, n, 1 << t, i, signed) for i in range(n)]
        reach = [b if j == i else bs[t] + max(b, reach[j] if j is not None else 0)
                 for i, (b, j) in enumerate(zip(reach, src))]
    content = [max(t[2][i] for t in tr) for i in range(n)]
    assert max(content) == wob(max(reach))
    for i in range(n):
        assert content[i] <= wob(reach[i]) <= sizes[i], (i, content, reach, sizes)
        # (under equal bounds, and under the arithmetic shr's repeated top bit, tops cancel by
        # parity at some bits; the u8 cases' one-FULL-bit values avoid it at every bit)
        if not signed and (n == 8 or len(set(ba)) == n):
            assert content[i] == wob(reach[i]), (i, content, reach)
    if name == "per_bit" and op in ("shl", "shr"):
        assert len(set(sizes)) >= 4  # prefix (shl) / suffix (shr) maxima: per-bit slots
        assert sizes == sorted(sizes, reverse=(op == "shr"))
    if name == "u32_headline_shape":
        assert sizes == [sizes[0]] * 32 and ob.tolist() == [1536] * 32
    if op in ("rotl", "rotr"):
        for t in range(1, L):  # stage t's save area: the amount bounds above t plus the widest a
            got = max(tr_[3].get(t, 0) for tr_ in tr)
            full = wob(sum(bs[t + 1:]) + max(ba))
            assert got <= full and 0 <= p["sv"][t] - 1 - full <= 1, (t, got)
            if len(set(ba)) == 1:  # (per-bit bounds: the bits that wrap need not be the widest)
                assert got == full, (t, got)
        assert p["oV"] - p["oS"] == max((1 << t) * p["sv"][t] for t in range(L))
    return dict(nprod=nprod, plan=p)


# ------------------------------------------------------------------ counts and runs
import array_model as am  # noqa: E402
import bitcount_model as bcm  # noqa: E402

SHARE_WORDS = 2560  # a wave's slice for the bit counts and the array circuits (bitcount_host.h)


def _bits8(b, **at):
    v = [b] * 8
    for i, x in at.items():
        v[int(i[1:])] = x
    return u32(v)


COUNT_OPS = tuple(bcm.OPS)
COUNT_CASES = {
    # name: (a bounds, the ops run)
    "w1_edge": (_bits8(255), COUNT_OPS),
    "w2_edge_top": (_bits8(255, b7=287), COUNT_OPS),
    "w2_edge_low": (_bits8(255, b0=287), COUNT_OPS),  # (bit 0: the last literal of a leading run)
    "chunks_319": (_bits8(319), COUNT_OPS),
    "chunks_320": (_bits8(320), COUNT_OPS),
    # (at 2040 the last running product is 64 + 447 = 511 words: 2047 is the bound whose product
    # has 512; the planner takes the counts there and refuses the runs)
    "one_tile": (_bits8(2047), COUNT_OPS[:2]),
    "multi_tile": (_bits8(2047, b7=2079), COUNT_OPS[:2]),
}


def _count_inputs(name):
    ba, _ = COUNT_CASES[name]
    seed = _seed("count", name)
    rng = np.random.default_rng(seed + 1)
    A = operands(ba, 8, seed, 0)
    # equal tops cancel by parity in a symmetric sum: all FULL reaches e_8 (and, with one wider
    # bit, every e_{2^k}); seven FULL and bit 3 one below reach e_1, e_2, e_4 under equal bounds
    A.append([_exact(rng, int(b)) for b in ba])
    A.append([_exact(rng, int(b) - (i == 3)) for i, b in enumerate(ba)])
    return dict(ba=ba, bb=ba, A=A, B=A, n=len(A), nbits=len(ba))


@functools.lru_cache(maxsize=None)
def count_reference(name, op):
    """(out bounds, values, limbs, degree words) of bitcount_model.circuit."""
    c = inputs("count", name)
    ob = bcm.bitcount_bounds(op, c["ba"])
    vals = [bcm.circuit(op, a) for a in c["A"]]
    return (ob, vals) + _frozen(*bm.pack(vals, ob))


def count_plan(op, ba):
    """plan_bitcount through tests/sanitize/bitcount_plan.cpp (its first row)."""
    return _plan("bitcount", f"{bcm.CODES[op]} {len(ba)} {_ints(ba)}")[0]


def count_trace(a, zeros):
    """bitcount_kernel on one value: E_j <- E_j + u_i E_{j-1} over the slots E_1 .. E_J (pruned by
    bitcount_needed, formed in T), and past slot J the running product of all literals in D / Dn,
    wave_mul(U, nu, P, np, ..) with the literal uniform.  Returns (the running products' (i, nu,
    np), the slot products' (i, j, nu, np, ne), the widest content of each slot, out)."""
    n = len(a)
    top = 1 << (n.bit_length() - 1)
    J = n // 2 if top == n and n >= 2 else top
    diag = J < top
    E, D = [1] + [0] * J, 0
    emax, drows, erows = [0] * (J + 1), [], []
    for i in range(1, n + 1):
        u = a[i - 1] ^ 1 if zeros else a[i - 1]
        if diag and i > J:
            P = E[J] if i == J + 1 else D
            if u and P:
                drows.append((i, words(u), words(P)))
            D = model.clmul_fast(u, P) if u and P else 0
        if not u:
            continue
        for j in range(min(i, J), 1, -1):
            if not bcm.needed(n, i, j) or not E[j - 1]:
                continue
            erows.append((i, j, words(u), words(E[j - 1]), words(E[j])))
            E[j] ^= model.clmul_fast(u, E[j - 1])
        E[1] ^= u
        emax = [max(m, words(p)) for m, p in zip(emax, E)]
    out = [E[1 << k] if 1 << k <= J else (D if diag and 1 << k == n else 0)
           for k in range(bcm.OUT_BITS)]
    return drows, erows, emax, out


def run_trace(a, zeros, leading):
    """bitrun_kernel on one value: t_j = t_{j-1} v_j in D / Dn, wave_mul(U, nu, D, np, ..), XORed
    into the accumulator of every output bit k with 2^k | j; a null t_j ends the chain."""
    n = len(a)
    v = [x ^ 1 for x in a] if zeros else list(a)
    if leading:
        v = v[::-1]
    K = n.bit_length()
    acc, rows, t = [0] * K, [], 0
    for j in range(1, n + 1):
        if j > 1 and not t:
            continue
        u = v[j - 1]
        if j == 1:
            t = u
        elif u:
            rows.append((j, words(u), words(t)))
            t = model.clmul_fast(u, t)
        else:
            t = 0
        if t:
            for k in range(K):
                if j & ((1 << k) - 1):
                    break
                acc[k] ^= t
    return rows, acc + [0] * (bcm.OUT_BITS - K)


@functools.lru_cache(maxsize=None)
def count_traces(name, op):
    run, zeros, leading = bcm.OPS[op]
    c = inputs("count", name)
    return [run_trace(a, zeros, leading) if run else count_trace(a, zeros) for a in c["A"]]


def check_count_path(name, op):
    """The path each count case is named for, in one op; plan_bitcount's buffers (the running
    product's D / Dn of cD words, the slots E_j or the runs' accumulators at off[]) from the plan
    driver, the output ones filled to the last word their bounds allow."""
    run, zeros, leading = bcm.OPS[op]
    c = inputs("count", name)
    ba = [int(b) for b in c["ba"]]
    tr = count_traces(name, op)
    chain = [r for t in tr for r in t[0]]  # the products in D / Dn: (position, nu, np)
    top = max(chain, key=lambda r: (r[1] + r[2], r[1]))
    nprod = top[1] + top[2]
    _, w, tiles, _ = product_shape(top[1], top[2])
    wide_last = (name == "w2_edge_top") != leading  # is the wide bit the chain's last literal?
    if name == "w1_edge":
        assert top[1:] == (8, 56) and (nprod, w, tiles) == (64, 1, 1) and top[0] == 8
    elif name in ("w2_edge_top", "w2_edge_low"):
        assert top[1:] == ((9, 56) if wide_last else (8, 57)) and (nprod, w) == (65, 2) and top[0] == 8
    elif name in ("chunks_319", "chunks_320"):
        nu = 10 if name == "chunks_319" else 11
        assert max(r[1] for r in chain) == nu and (nu + 9) // 10 == nu - 9
    elif name == "one_tile":
        assert top[1:] == (64, 448) and (nprod, w, tiles) == (512, 8, 1)
    elif name == "multi_tile":
        assert top[1:] == (65, 448) and (nprod, w, tiles) == (513, 8, 2)
    else:
        raise KeyError(name)
    ob, vals, _, _ = count_reference(name, op)
    live = [k for k in range(bcm.OUT_BITS) if 1 << k <= len(ba)]
    _reaches(vals, ob, live)
    assert all(v[k] == 0 for v in vals for k in range(bcm.OUT_BITS) if k not in live)
    p = count_plan(op, ba)
    assert p["status"] == 0 and p["lds_per_wave"] <= SHARE_WORDS and p["bounds"] == ob.tolist()
    assert nprod <= p["cD"] and p["cD"] - nprod <= 3  # even(sum / 32 + 2) words for sum / 32 + 1
    ends = p["off"][1:p["J"] + 1] + [p["lds_per_wave"] - p["oE"]] if not run else \
        p["off"][:p["K"]] + [p["lds_per_wave"] - p["oE"]]
    sizes = [b - a for a, b in zip(ends, ends[1:])]
    if run:
        for k in range(p["K"]):
            assert max(words(v[k]) for v in vals) == wob(ob[k]) <= sizes[k] <= wob(ob[k]) + 2
    else:
        assert p["J"] == 4 and p["diag"] == 1
        sums = [sum(sorted(ba, reverse=True)[:j]) for j in range(p["J"] + 1)]
        emax = [max(t[2][j] for t in tr) for j in range(p["J"] + 1)]
        for j in range(1, p["J"] + 1):
            assert emax[j] <= wob(sums[j]) <= sizes[j - 1] <= wob(sums[j]) + 2, (j, emax, sizes)
            if j & (j - 1) == 0:  # an output's slot
                assert emax[j] == wob(sums[j])
        # T holds the widest slot product, u_i E_{J-1} + E_J
        tmax = max(max(r[2] + r[3], r[4]) for t in tr for r in t[1])
        assert tmax <= p["oD"] - p["oT"] and p["oD"] - p["oT"] - tmax <= 3
    return dict(nprod=nprod, plan=p)


# ------------------------------------------------------------------ array read and write
def _arr(count, ba, bx=None, bs=255):
    k = am.index_bits(count)
    return dict(count=count, ba=u32(ba), bx=u32(ba if bx is None else bx),
                bs=u32([bs] * k + [0] * (8 - k)))


ARRAY_CASES = {
    "w1_edge": _arr(4, [1535] * 8),
    "w2_edge": _arr(4, [1567] * 8),
    "count5_per_bit": _arr(5, [63 + 97 * i for i in range(8)], [700 - 83 * i for i in range(8)]),
}
INDEX_SHIFT, VALUE_SHIFT = 5, 6


def _array_inputs(name):
    """A: the array batch, count consecutive values per array; B: the index batch (u8, its low k
    bits read); C: the written value."""
    spec = ARRAY_CASES[name]
    count, ba, bx, bs = spec["count"], spec["ba"], spec["bx"], spec["bs"]
    k = am.index_bits(count)
    seed = _seed("array", name)
    rng = np.random.default_rng(seed + 2)
    els = [operands(ba, 8, seed + 10 + v, v) for v in range(count)]  # element v of arrays 0 .. 7
    arrs = [[els[v][e] for v in range(count)] for e in range(8)]
    S = [[poly(kind_of(e, t, INDEX_SHIFT), bs[t], rng) if t < k else 0 for t in range(8)]
         for e in range(8)]
    X = operands(bx, 8, seed + 3, VALUE_SHIFT)
    # the read's top coefficient is the parity of the elements at their bound: one FULL element
    # and the others one below, x FULL; then every element FULL under an x one below its bound
    full = lambda bnd, d=0: [_exact(rng, max(int(b) - d, 0)) for b in bnd]  # noqa: E731
    arrs.append([full(ba, int(v != 0)) for v in range(count)])
    arrs.append([full(ba) for v in range(count)])
    X += [full(bx), full(bx, 1)]
    S += [[_exact(rng, int(bs[t])) if t < k else 0 for t in range(8)] for _ in range(2)]
    flat = [el for arr in arrs for el in arr]
    return dict(ba=ba, bb=bs, bc=bx, A=flat, B=S, C=X, arrays=arrs, n=len(S), nbits=len(ba),
                count=count, k=k)


@functools.lru_cache(maxsize=None)
def array_reference(name, what):
    """what "read" or "write": (out bounds, values, limbs, degree words) of array_model's circuits
    (the write's values: the output array batch, count elements per array)."""
    c = inputs("array", name)
    if what == "read":
        ob = am.read_bounds(c["ba"], c["count"], c["bb"])
        vals = [am.circuit_read(arr, s) for arr, s in zip(c["arrays"], c["B"])]
    else:
        ob = am.write_bounds(c["ba"], c["bc"], c["count"], c["bb"])
        vals = [el for arr, s, x in zip(c["arrays"], c["B"], c["C"])
                for el in am.circuit_write(arr, s, x)]
    return (ob, vals) + _frozen(*bm.pack(vals, ob))


def array_plan(what, count, ba, bs, bx=None):
    """plan_array_read / plan_array_write through tests/sanitize/array_plan.cpp (its first row)."""
    k = am.index_bits(count)
    mid = f" {_ints(bx)}" if what == "write" else ""
    return _plan("array", f"{am.CODES[what]} {len(ba)} {count} {_ints(ba)}{mid} {_ints(bs[:k])}")[0]


def read_trace(arr, s):
    """array_read_kernel on one array: per output bit the multiplexer tree, a level-t join as
    wave_mul(s_t, ns, V, nv, Add, nadd, ..) with V = L + R and Add = L (under the last element with
    nothing beside it V = Add = the node); a null s_t or V skips the product.  Rows (j, t, ns,
    nv, nadd); the widest node per level."""
    k = am.index_bits(len(arr))
    rows, lvl = [], [0] * (k + 1)
    for j in range(len(arr[0])):
        level = [el[j] for el in arr]
        for t in range(k):
            lvl[t] = max([lvl[t]] + [words(p) for p in level])
            nxt = []
            for q in range(0, len(level), 2):
                L = level[q]
                V = L ^ level[q + 1] if q + 1 < len(level) else L
                if s[t] and V:
                    rows.append((j, t, words(s[t]), words(V), words(L)))
                    nxt.append(L ^ model.clmul_fast(s[t], V))
                else:
                    nxt.append(L)
            level = nxt
        lvl[k] = max(lvl[k], words(level[0]))
    return rows, lvl


def write_trace(arr, s, x):
    """array_write_kernel on one array: the indicator Q_0 of every element by suffix products,
    then per bit wave_mul(X, nx, Q0, nind, T, nt, O) with X = x_j + T_j the uniform operand.
    Rows (v, j, nx, nind, nt)."""
    k = am.index_bits(len(arr))
    rows, qmax = [], 0
    for v, el in enumerate(arr):
        ind = am.indicator(s, v, k, model.clmul_fast)
        qmax = max(qmax, words(ind))
        for j, (T, xj) in enumerate(zip(el, x)):
            if ind and xj ^ T:
                rows.append((v, j, words(xj ^ T), words(ind), words(T)))
    return rows, qmax


def check_array_path(name):
    """The paths of the array cases and plan_array_read's / plan_array_write's buffers from the plan
    driver, filled."""
    c = inputs("array", name)
    count, k = c["count"], c["k"]
    ba, bx, bs = ([int(b) for b in c[key]] for key in ("ba", "bc", "bb"))
    S = sum(bs[:k])
    rt = [read_trace(arr, s) for arr, s in zip(c["arrays"], c["B"])]
    wt = [write_trace(arr, s, x) for arr, s, x in zip(c["arrays"], c["B"], c["C"])]
    l1 = max((r for t in rt for r in t[0] if r[1] == 1), key=lambda r: r[2] + r[3])
    wr = max((r for t in wt for r in t[0]), key=lambda r: r[2] + r[3])
    if name == "w1_edge":
        assert l1[2:4] == (8, 56) and wr[2:4] == (48, 16)
    elif name == "w2_edge":
        assert l1[2:4] == (8, 57) and wr[2:4] == (49, 16)
    elif name == "count5_per_bit":
        assert (count, k) == (5, 3) and len(set(ba)) == 8
        # the last element rises alone: V = Add = the node at levels 0 and 1
        assert any(r[3] == r[4] and r[1] < 2 for t in rt for r in t[0])
    else:
        raise KeyError(name)
    ob, vals, _, _ = array_reference(name, "read")
    _reaches(vals, ob)
    p = array_plan("read", count, ba, bs)
    assert p["status"] == 0 and p["lds_per_wave"] <= SHARE_WORDS and p["bounds"] == ob.tolist()
    lv = [max(t[1][q] for t in rt) for q in range(k + 1)]
    bound = [max(ba) + sum(bs[:q]) for q in range(k + 1)]
    assert lv == [wob(b) for b in bound]  # every level's widest node, the root's included
    ends = [p["oL"], p["oX"], p["oP"], p["oP"] + p["cP"], p["oP"] + 2 * p["cP"]] + \
        p["slot"][1:k] + [p["lds_per_wave"]]
    sizes = [b - a for a, b in zip(ends, ends[1:])]
    for size, q in zip(sizes, [0, k - 1, k, k] + list(range(k))):
        assert lv[q] <= size <= lv[q] + 2, (sizes, lv)
    assert p["slot"][0] == p["oP"] + 2 * p["cP"]
    ob, vals, _, _ = array_reference(name, "write")
    _reaches(vals, ob)
    p = array_plan("write", count, ba, bs, bx)
    assert p["status"] == 0 and p["lds_per_wave"] <= SHARE_WORDS and p["bounds"] == ob.tolist()
    wide = max(max(ba), max(bx))
    assert max(t[1] for t in wt) == wob(S) and wr[2] == wob(wide)
    osize = p["qoff"][k - 1] - p["oO"]
    assert wr[2] + wr[3] == wob(S) + wob(wide) <= osize <= wob(S + wide) + 2
    assert p["oO"] - p["oX"] >= wr[2] and p["oO"] - p["oX"] - wr[2] <= 2
    return dict(read=l1, write=wr)


_WAVE_FAMILIES = {"select": _select_inputs, "minmax": _minmax_inputs, "lookup": _lookup_inputs,
                  "shift": _shift_inputs, "count": _count_inputs, "array": _array_inputs}


# =============================================================================================
# The multiplier's chunk loop, its staging checks and the plans with K > 32
# (test_gpu_mul_chunks.py).  mul_columns (mul_host.cpp) cuts a batch into chunks of
# values that share one workspace; hm_ctx_set_mul_chunk caps the chunk, so that e0 > 0, a short
# last chunk and an arena last written by longer operands are met at batches of 10 values.

# The smallest case per launch family, (family, name): run chunked against the unchunked references
# above (mul_reference, mul_class_reference).
CHUNK_CASES = (
    ("mul", "u8_b128"), ("mul", "i8_b128"), ("mul", "u16_low4_per_bit"),
    ("mulc", "ppv_12w"), ("mulc", "ppg_tiny_13w"), ("mulc", "ppg_gen_33w"), ("mulc", "rows_v36"),
    ("mulc", "ppm_wide"), ("mulc", "u8_b640_full"), ("mulc", "u8_b703_ka224"),
)
STALE_LADDERS = ("ladder_ppg_gen", "ladder_ppm", "ladder_rows")


def mul_spec(family, name):
    """dict(k, signed, ka) of a "mul" or "mulc" case, and its reference function."""
    if family == "mul":
        _, _, signed, k, _, _ = MUL_CASES[name]
        return dict(k=k, signed=signed, ka=None), mul_reference
    spec = MUL_CLASS_CASES[name]
    return dict(k=spec["k"], signed=spec["signed"], ka=spec["ka"]), mul_class_reference


@functools.lru_cache(maxsize=None)
def descending(name):
    """A ladder with its values in descending order (the widest a_i first), operands and reference
    rows permuted alike: (la, da, lb, db, out bounds, rl, rd).  Every chunk after the first then
    meets arena slots last written by longer operands."""
    c = inputs("mulc", name)
    ob, vals, _, _ = mul_class_reference(name)
    perm = list(range(c["n"]))[::-1]
    words_a = [words(c["A"][e][0]) for e in perm]
    assert words_a == sorted(words_a, reverse=True) and words_a[0] > words_a[-1]
    la, da = bm.pack([c["A"][e] for e in perm], c["ba"])
    lb, db = bm.pack([c["B"][e] for e in perm], c["bb"])
    return (la, da, lb, db, ob) + _frozen(*bm.pack([vals[e] for e in perm], ob))


STALE_BLOCK = 4


@functools.lru_cache(maxsize=None)
def interleaved(name):
    """16 values over a ladder case's bounds (mul_low(3)), in blocks of STALE_BLOCK: every bit of a
    and b FULL; then a NULL under b FULL and a FULL over b NULL, two values each (every partial
    product null); FULL again; then a = b = UNIT in two values, a UNIT under b FULL, a FULL over
    b UNIT (products of one word, or copies of the other operand).  With a chunk of STALE_BLOCK
    values, chunks of full operands alternate with chunks whose every product is null or short, in
    the slots the full ones filled.  dict(A, B, ba, bb, n, ob, vals) + packed operands and
    reference."""
    c = inputs("mulc", name)
    ba, bb, k = c["ba"], c["bb"], MUL_CLASS_CASES[name]["k"]
    rng = np.random.default_rng(_seed("interleaved", name))
    full = lambda bnd: [_exact(rng, int(b)) for b in bnd]  # noqa: E731
    null, unit = [0] * len(ba), [1] * len(ba)
    A = [full(ba) for _ in range(4)] + [null, null, full(ba), full(ba)] + \
        [full(ba) for _ in range(4)] + [unit, unit, unit, full(ba)]
    B = [full(bb) for _ in range(4)] + [full(bb), full(bb), null, null] + \
        [full(bb) for _ in range(4)] + [unit, unit, full(bb), unit]
    ob = mul_bounds(ba[:k], bb[:k])
    vals = [mul_ref(a[:k], b[:k]) for a, b in zip(A, B)]
    assert all(v == [0] * k for v in vals[4:8]) and vals[12] == [1, 0, 0][:k]  # 7 * 7 = 49
    return dict(A=A, B=B, ba=ba, bb=bb, n=16, k=k, ob=ob, vals=vals,
                a=bm.pack(A, ba), b=bm.pack(B, bb), ref=_frozen(*bm.pack(vals, ob)))


# ------------------------------------------------------------------ staging validation
STAGE_BOUND, STAGE_N, STAGE_CHUNK = 383, 8, 3
CORRUPTIONS = ("bit_above_degree", "degree_above_bound", "top_bit_cleared", "limb_past_degree")


@functools.lru_cache(maxsize=None)
def stage_inputs():
    """The clean batch of the staging-validation tests: u8 at the uniform bound 383 (the ppv plan:
    mul_stage_value_kernel, 6 limbs per bit), the 8 scheduled values."""
    ba = uniform(8, STAGE_BOUND)
    A, B = batch(ba, ba, STAGE_N, 0, _seed("stage", "u8_b383"))
    return dict(ba=ba, bb=ba, A=A, B=B, n=STAGE_N, nbits=8, a=bm.pack(A, ba), b=bm.pack(B, ba))


@functools.lru_cache(maxsize=None)
def stage_reference(what):
    """what: "low4" (mul_low(4)), "full" (the unsigned multiply), "and", "not"."""
    c = stage_inputs()
    if what in ("low4", "full"):
        k = 4 if what == "low4" else 8
        ob = mul_bounds(c["ba"][:k], c["bb"][:k])
        vals = [mul_ref(a[:k], b[:k]) for a, b in zip(c["A"], c["B"])]
    else:
        ob = gate_bounds(what, c["ba"], c["bb"])
        vals = [gate_circuit(what, a, b) for a, b in zip(c["A"], c["B"])]
    return (ob, vals) + _frozen(*bm.pack(vals, ob))


def corruptible(p, bound, how):
    """Whether polynomial p of a bit of this bound can take the corruption inside the bit's own
    limbs: bit_above_degree sets coefficient deg + 1 in the degree's limb; top_bit_cleared needs a
    top coefficient that the degree word is checked against (deg > 0); limb_past_degree sets a
    coefficient in the bit's last limb, which must lie past the degree's limb."""
    d, cap = model.degree(p), int(bound) // 64 + 1
    if how == "bit_above_degree":
        return (d + 1) % 64 != 0 and d + 1 <= int(bound)
    if how == "top_bit_cleared":
        return d > 0
    if how == "limb_past_degree":
        return d // 64 < cap - 1
    return how == "degree_above_bound"


def corruption_site(values, bound, how, bits, first=STAGE_CHUNK):
    """The first (value e >= first, bit i in bits) whose polynomial can take the corruption: with a
    chunk of `first` values the corrupted value is in a chunk with e0 > 0.  A polynomial of degree
    above 0 where there is one, else a null or unit one."""
    for nonconstant in (True, False):
        for e in range(first, len(values)):
            for i in bits:
                p = values[e][i]
                if corruptible(p, bound[i], how) and (p > 1 or not nonconstant):
                    return e, i
    raise LookupError(how)


def corrupt(limbs, deg, bound, n, e, i, how):
    """A copy of the packed batch with one corruption in value e, bit i.  Every write stays inside
    that bit's own cap limbs and its own degree word."""
    bound = u32(bound)
    cap = (bound // 64 + 1).astype(np.int64)
    limbs, deg = limbs.copy(), deg.copy().reshape(n, len(bound))
    base = e * int(cap.sum()) + int(cap[:i].sum())
    d, last = int(deg[e, i]), base + int(cap[i]) - 1
    if how == "bit_above_degree":
        g = base + (d + 1) // 64
        assert g == base + d // 64 <= last
        limbs[g] |= np.uint64(1 << ((d + 1) % 64))
    elif how == "degree_above_bound":
        deg[e, i] = int(bound[i]) + 1
    elif how == "top_bit_cleared":
        assert d > 0
        limbs[base + d // 64] &= np.uint64(~(1 << (d % 64)) & (2**64 - 1))
    elif how == "limb_past_degree":
        assert base + d // 64 < last
        limbs[last] |= np.uint64(1 << 7)
    else:
        raise KeyError(how)
    return limbs, deg.reshape(-1)


# ------------------------------------------------------------------ plans with K > 32
# u64 operands whose every bit has bound 0: each ciphertext bit is the null or the unit polynomial,
# the only bounds at which build_plan (mul_plan.h) accepts K > 32 at a size a test can run.  2 K > 64
# takes launch_mul_stage off mul_stage_value_kernel, onto mul_stage_kernel (one wave per (value,
# bit)).  name -> (K, signed); K = 64 is the full circuit.
WIDE_CASES = {"low33": (33, False), "low40": (40, False), "full64": (64, False),
              "full64_signed": (64, True)}
WIDE_ASTRIDE = {33: 6352, 40: 9376, 64: 24208}  # arena words per value
_M64 = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def wide_values():
    """The six (a, b) pairs as integers: all NULL under all UNIT, all UNIT twice, alternating bits
    against their complement, two random patterns (one against an all-NULL b), 2^63 + 1 squared."""
    rng = np.random.default_rng(_seed("wide", "u64_b0"))
    r = [_rand_bits(rng, 64) for _ in range(3)]
    alt = int("AA" * 8, 16)
    top = (1 << 63) | 1
    return ((0, _M64), (_M64, _M64), (alt, alt >> 1), (r[0], r[1]), (r[2], 0), (top, top))


def _bits64(v):
    return [(v >> i) & 1 for i in range(64)]


@functools.lru_cache(maxsize=None)
def wide_inputs():
    ba = uniform(64, 0)
    A = [_bits64(a) for a, _ in wide_values()]
    B = [_bits64(b) for _, b in wide_values()]
    return dict(ba=ba, bb=ba, A=A, B=B, n=len(A), nbits=64, a=bm.pack(A, ba), b=bm.pack(B, ba))


@functools.lru_cache(maxsize=None)
def wide_reference(name):
    """(out bounds, values, limbs, degree words) of the model's K-bit circuit on the low K bits."""
    K, signed = WIDE_CASES[name]
    c = wide_inputs()
    ob = mul_bounds(c["ba"][:K], c["bb"][:K])
    vals = [mul_ref(a[:K], b[:K], signed) for a, b in zip(c["A"], c["B"])]
    return (ob, vals) + _frozen(*bm.pack(vals, ob))


def wide_census(name, mfma=True, ba=None):
    K, signed = WIDE_CASES[name]
    b = tuple(int(x) for x in (wide_inputs()["ba"] if ba is None else ba)[:K])
    return plan_census(64, K, signed and K == 64, 256, 256, mfma, b, tuple([0] * K))


def check_mul_wide_path(name):
    """The path of a WIDE_CASES case from the planner's census: K > 32 (so 2 K > 64 and
    launch_mul_stage takes mul_stage_kernel), the arena stride, where the K (K + 1) / 2 partial
    products run, and every column's scan: column i has its i + 1 partial products and the carries
    of the column before, one per item but the first, so 1 + i (i + 1) / 2 items; the scan stages
    20 bytes per item in LDS (launch_mul_scan: at most 64 KiB)."""
    K, signed = WIDE_CASES[name]
    assert K > 32 and 2 * K > 64
    flip = signed and K == 64
    for mfma in (True, False):
        cen = wide_census(name, mfma)
        cols = cen["cols"]
        assert cen["K"] == K and len(cols) == K and bool(cen["signed"]) == flip
        assert cen["astride"] == WIDE_ASTRIDE[K] < 10**5
        assert not cen["ppg"] and not cen["ppv"] and cen["pp_instance"] == ""  # no grouped launch
        nitems = [col["nitems"] for col in cols]
        assert nitems == [1 + i * (i + 1) // 2 for i in range(K)]
        assert 20 * max(nitems) <= 64 * 1024
        assert {col["res_bound"] for col in cols} == {0} and {col["maxwords"] for col in cols} == {4}
        assert not any(col["ka"] for col in cols)
        vpp = [col["npp"] for col in cols]       # partial products on mul_pp_kernel
        mpp = [col["ppl"]["nspans"] for col in cols]  # ... and on the matrix cores
        if mfma:  # the signed corners a_0 b_63 + 1 and a_63 b_0 + 1 stay on the VALU
            assert vpp == [0] * (K - 1) + [2 if flip else 0]
            assert mpp == [i + 1 for i in range(K - 1)] + [K - (2 if flip else 0)]
            assert all(_launch(col["ppl"], "tiny", 4, 4) for col in cols[:K - 1])
            # carry products, i (i + 1) / 2 in column i < K - 1 (4 x 4 words each): one
            # mul_rows_kernel launch up to column 28's 406, one launch on the tiny MFMA instance
            # from column 29's 435 on, where the rows no longer fit a wave's share of LDS
            for i, col in enumerate(cols):
                c = i * (i + 1) // 2 if i + 1 < K else 0
                tiny = col["mfl"][0]
                assert (col["nrows"], tiny["nspans"]) == ((c, 0) if i <= 28 else (0, c)), i
                assert not c or i <= 28 or _launch(tiny, "tiny", 4, 4)
                assert not col["mfl"][1]["nspans"] and not col["mfl"][2]["nspans"]
        else:
            assert vpp == [i + 1 for i in range(K)] and not any(mpp)
            assert not any(col["nrows"] for col in cols)
            assert not any(m["nspans"] for col in cols for m in col["mfl"])
            # one W = 1 tile per carry product: none in column 0, none pushed by the last column
            # of the full circuit
            carries = sum(n - 1 for n in nitems[:K - 1])
            assert sum(col["ntiles"][0] for col in cols) == carries
    return cen


# One bit of a wider bound among the bound-0 bits of the K = 33 plan: a_32 at bound 64 (two limbs,
# read by column 32 alone, which pushes no carries), so that stage_one's check of the limbs past the
# degree's limb has a limb to look at.
WIDE_STAGE_BIT, WIDE_STAGE_BOUND = 32, 64


@functools.lru_cache(maxsize=None)
def wide_stage_inputs():
    c = wide_inputs()
    ba = c["ba"].copy()
    ba[WIDE_STAGE_BIT] = WIDE_STAGE_BOUND
    rng = np.random.default_rng(_seed("wide", "stage"))
    A = [list(v) for v in c["A"]]
    for e, v in enumerate(A):  # degrees 0 .. 64 at the wide bit: the degree's limb is the first or the second
        v[WIDE_STAGE_BIT] = (0, 1, _exact(rng, 5), _exact(rng, 63), _exact(rng, 64), _exact(rng, 40))[e]
    K = WIDE_CASES["low33"][0]
    ob = mul_bounds(ba[:K], c["bb"][:K])
    vals = [mul_ref(a[:K], b[:K]) for a, b in zip(A, c["B"])]
    return dict(ba=ba, bb=c["bb"], A=A, B=c["B"], n=c["n"], K=K, ob=ob, vals=vals,
                a=bm.pack(A, ba), b=c["b"], ref=_frozen(*bm.pack(vals, ob)))
