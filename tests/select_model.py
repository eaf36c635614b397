"""Model circuits of select, min and max over the big-integer GF(2)[X] model
(oracle/gf2_model.py) and the ripple-borrow model (tests/borrow_model.py): the specification the
engine's select_kernel and minmax_kernel are bit-exact against, and their static
degree bounds.  A polynomial is a Python int; a value is the list of its bit polynomials, least
significant first.

    x_i = a_i + b_i
    select(c, a, b):  out_i = b_i + c x_i         (c: bit 0 of a Ciphered<bool>; 1 gives a, 0 gives b)
    min(a, b):        out_i = b_i + w_n x_i       (w_n: the borrow out of the top bit of a - b,
    max(a, b):        out_i = a_i + w_n x_i        the polynomial a < b returns; no operand exchange)
"""
from __future__ import annotations

import numpy as np

import borrow_model as bm
from oracle import gf2_model as model


def select_circuit(c, a, b):
    """c: the condition polynomial (bit 0 of the Ciphered<bool>)."""
    return [y ^ model.clmul(c, x ^ y) for x, y in zip(a, b)]


def less_than(a, b, signed=False):
    return bm.borrows(a, b, signed)[-1]


def min_circuit(a, b, signed=False):
    w = less_than(a, b, signed)
    return [y ^ model.clmul(w, x ^ y) for x, y in zip(a, b)]


def max_circuit(a, b, signed=False):
    w = less_than(a, b, signed)
    return [x ^ model.clmul(w, x ^ y) for x, y in zip(a, b)]


# ------------------------------------------------------------------ static bounds
def select_bounds(cond_bound0, ba, bb):
    return np.array([int(cond_bound0) + max(int(x), int(y)) for x, y in zip(ba, bb)],
                    dtype=np.uint32)


def minmax_bounds(ba, bb):
    n = len(ba)
    return select_bounds(bm.borrow_bounds(ba, bb, n)[n], ba, bb)
