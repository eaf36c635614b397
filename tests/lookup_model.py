"""Model circuit of the table lookup over the big-integer GF(2)[X] model (oracle/gf2_model.py):
the specification the engine's lookup_kernel is bit-exact against, and its
table-dependent static degree bounds.  A polynomial is a Python int; a value is the list of its bit
polynomials, least significant first.

    f_j(v) = bit j of table[v]                        (v over the 2^k values of the k index bits)
    c_j[S] = XOR over S' subset of S of f_j(S')       (algebraic normal form, Moebius transform)
    out_j  = sum over S with c_j[S] = 1 of prod_{i in S} a_i      (the empty product is 1)

The model forms all 2^k monomials; GF(2)[X] is commutative, so any evaluation order gives the same
polynomials.  Batch packing: borrow_model.pack.
"""
from __future__ import annotations

import numpy as np

from borrow_model import pack  # noqa: F401  (the batch layout the tests compare with)
from oracle import gf2_model as model


def table_bits(table):
    """(entries as unsigned ints of the table's bit patterns, output bits)."""
    t = np.asarray(table)
    nbits = 8 * t.dtype.itemsize
    u = t.astype(np.uint8) if t.dtype == np.bool_ else t.view(np.dtype(f"u{t.dtype.itemsize}"))
    return [int(x) for x in u], nbits


def index_bits(table):
    n = len(table)
    k = n.bit_length() - 1
    assert n == 1 << k and 1 <= k <= 8, "a table has 2^k entries, k in 1..8"
    return k


def moebius(table):
    """c[j] = the list over S in 0 .. 2^k - 1 of the coefficient of the monomial of the index bits
    in S, for every output bit j."""
    entries, nbits = table_bits(table)
    k = index_bits(entries)
    out = []
    for j in range(nbits):
        f = [(e >> j) & 1 for e in entries]
        for i in range(k):
            for v in range(1 << k):
                if (v >> i) & 1:
                    f[v] ^= f[v ^ (1 << i)]
        out.append(f)
    return out


def coefficient_masks(table):
    """c[j] as one integer per output bit: bit S = the coefficient of monomial S."""
    return [sum(b << S for S, b in enumerate(f)) for f in moebius(table)]


def monomials(a, k):
    """All 2^k products of the index bits a[0:k]: M[S] = prod_{i in S} a[i], M[0] = 1."""
    M = [1] * (1 << k)
    for S in range(1, 1 << k):
        low = S & -S
        M[S] = model.clmul(M[S ^ low], a[low.bit_length() - 1])
    return M


def lookup_circuit(a, table):
    """The output bit polynomials of table[v], v = the low k bits of the value a."""
    k = index_bits(table)
    M = monomials(a, k)
    out = []
    for f in moebius(table):
        p = 0
        for S, c in enumerate(f):
            if c:
                p ^= M[S]
        out.append(p)
    return out


def lookup_bounds(a_bound, table):
    """out_bound[j] = max over S with c_j[S] = 1 of the sum of a_bound over S (0 when none)."""
    k = index_bits(table)
    sums = [sum(int(a_bound[i]) for i in range(k) if (S >> i) & 1) for S in range(1 << k)]
    return np.array([max([sums[S] for S, c in enumerate(f) if c], default=0)
                     for f in moebius(table)], dtype=np.uint32)
