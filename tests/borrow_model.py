"""Model circuits of the ripple-borrow operations (subtraction, ==, !=, <, <=, >, >=) over the
big-integer GF(2)[X] model (oracle/gf2_model.py): the specification the engine's borrow kernel is
bit-exact against, its static degree bounds, and the batch-layout packing the
tests compare with.  A polynomial is a Python int (bit k = coefficient of X^k); a value is the
list of its bit polynomials, least significant first.

    x_i = a_i + b_i,  p_i = x_i + 1
    w_0 = 0,  w_{i+1} = a_i b_i + b_i + p_i w_i      (signed <: bit n-1 generates a_i b_i + a_i)
    a - b:   out_i = x_i + w_i                        (w_n is never formed)
    a < b:   w_n;   a > b: operands exchanged;   >= and <=: plus 1
    a == b:  e_n with e_0 = 1, e_{i+1} = p_i e_i;     !=: plus 1
"""
from __future__ import annotations

import numpy as np

from oracle import gf2_model as model

COMPARISONS = ("eq", "ne", "lt", "le", "gt", "ge")
NUMPY_OPS = {"eq": np.equal, "ne": np.not_equal, "lt": np.less, "le": np.less_equal,
             "gt": np.greater, "ge": np.greater_equal}


def borrows(a, b, signed=False, last=True):
    """[w_0 .. w_n] (w_0 .. w_{n-1} when not last)."""
    n = len(a)
    w = [0]
    for i in range(n if last else n - 1):
        gen = a[i] if signed and i == n - 1 else b[i]
        p = a[i] ^ b[i] ^ 1
        w.append(model.clmul(a[i], b[i]) ^ gen ^ model.clmul(p, w[i]))
    return w


def sub_circuit(a, b):
    w = borrows(a, b, last=False)
    return [a[i] ^ b[i] ^ w[i] for i in range(len(a))]


def equal_circuit(a, b):
    e = 1
    for x, y in zip(a, b):
        e = model.clmul(x ^ y ^ 1, e)
    return e


def compare_circuit(op, a, b, signed=False):
    """The result polynomial (bit 0 of the Ciphered<bool>)."""
    if op in ("eq", "ne"):
        return equal_circuit(a, b) ^ (op == "ne")
    if op in ("gt", "le"):
        a, b = b, a
    return borrows(a, b, signed)[-1] ^ (op in ("ge", "le"))


# ------------------------------------------------------------------ static bounds
def borrow_bounds(ba, bb, upto):
    wb = [0]
    for i in range(upto):
        wb.append(max(int(ba[i]) + int(bb[i]), max(int(ba[i]), int(bb[i])) + wb[i]))
    return wb


def sub_bounds(ba, bb):
    n = len(ba)
    wb = borrow_bounds(ba, bb, n - 1)
    return np.array([max(int(ba[i]), int(bb[i]), wb[i]) for i in range(n)], dtype=np.uint32)


def compare_bounds(op, ba, bb):
    n = len(ba)
    if op in ("eq", "ne"):
        r = sum(max(int(x), int(y)) for x, y in zip(ba, bb))
    elif op in ("gt", "le"):
        r = borrow_bounds(bb, ba, n)[n]
    else:
        r = borrow_bounds(ba, bb, n)[n]
    return np.array([r] + [0] * 7, dtype=np.uint32)


# ------------------------------------------------------------------ batch layout
def pack(values, bound):
    """values: per value the list of its bit polynomials (ints) -> (limbs, degree words) in the
    batch layout with these per-bit bounds (exact degrees; the null polynomial has degree 0)."""
    bound = np.asarray(bound, dtype=np.uint32)
    cap = bound // 64 + 1
    limbs, deg = [], []
    for bits in values:
        assert len(bits) == len(bound)
        for p, c in zip(bits, cap):
            limbs += model.int_to_limbs(p, int(c))
            deg.append(model.degree(p))
    return np.array(limbs, dtype=np.uint64), np.array(deg, dtype=np.uint32)


def bool_value(p):
    """A comparison's Ciphered<bool>: the result polynomial and seven null bits."""
    return [p] + [0] * 7


def decrypt_value(bits, s):
    """The plaintext integer of one value (bit polynomials, LSB first) under the secret key s."""
    return sum(model.decipher_bit(p, s) << i for i, p in enumerate(bits))
