"""Model circuits of the oblivious array read and write by an encrypted index over the big-integer
GF(2)[X] model (oracle/gf2_model.py): the specification the engine's array_read_kernel and
array_write_kernel are bit-exact against, their static degree bounds, and the
integer semantics.  A polynomial is a Python int; a value is the list of its bit polynomials, least
significant first; an array is the list of its count elements (2..256), each such a value.

    k = ceil(log2 count) index bits s_0 .. s_{k-1} are read
    ind_v  = prod_t (s_t + 1 + v_t)       (v_t bit t of v: the literal s_t where 1, s_t + 1 where 0)
    read:    out_j = sum over v < count of ind_v T_{v,j}, evaluated as a multiplexer tree: level t
             joins siblings by y = L + s_t (L + R); a right sibling past the array is the null
             polynomial, a subtree with no element at all is skipped
    write:   out_{v,j} = T_{v,j} + ind_v (x_j + T_{v,j}) for every v < count

Both are fixed polynomials of their inputs, so any evaluation order gives the same ones (the tree
and the indicator sum agree: circuit_read_sum).  Batch packing: borrow_model.pack.
"""
from __future__ import annotations

import numpy as np

from borrow_model import pack  # noqa: F401  (the batch layout the tests compare with)
from oracle import gf2_model as model

CODES = {"read": 28, "write": 29}


def index_bits(count):
    assert 2 <= count <= 256, "an array has 2..256 elements"
    return (int(count) - 1).bit_length()


def degree_of(k):
    """m, the circuits' degree in fresh bits: the requirement is 2m + 1 = 2k + 3."""
    return k + 1


def indicator(s, v, k, mul=model.clmul):
    p = 1
    for t in range(k):
        p = mul(p, s[t] ^ (((v >> t) & 1) ^ 1))
    return p


def circuit_read(arr, s, mul=model.clmul):
    """The output bit polynomials of arr[i], i the low k bits of the index value s, as the tree."""
    count, k = len(arr), index_bits(len(arr))
    assert len(s) >= k
    out = []
    for j in range(len(arr[0])):
        level = [el[j] for el in arr]
        for t in range(k):
            nxt = []
            for p in range(0, len(level), 2):  # (only nodes with an element below them exist)
                L = level[p]
                R = level[p + 1] if p + 1 < len(level) else 0
                nxt.append(L ^ mul(s[t], L ^ R))
            level = nxt
        assert len(level) == 1
        out.append(level[0])
    return out


def circuit_read_sum(arr, s, mul=model.clmul):
    """The same polynomials as the plain sum of indicator times element."""
    k = index_bits(len(arr))
    ind = [indicator(s, v, k, mul) for v in range(len(arr))]
    out = []
    for j in range(len(arr[0])):
        p = 0
        for v, el in enumerate(arr):
            p ^= mul(ind[v], el[j])
        out.append(p)
    return out


def circuit_write(arr, s, x, mul=model.clmul):
    """The output array of arr with arr[i] = x: count elements of bit polynomials."""
    k = index_bits(len(arr))
    assert len(s) >= k and len(x) == len(arr[0])
    out = []
    for v, el in enumerate(arr):
        ind = indicator(s, v, k, mul)
        out.append([T ^ mul(ind, xj ^ T) for T, xj in zip(el, x)])
    return out


def read_bounds(arr_bound, count, s_bound):
    """out_bound[j] = S + arr_bound[j], S the sum of the index's low k bounds."""
    S = sum(int(b) for b in s_bound[:index_bits(count)])
    return np.array([S + int(b) for b in arr_bound], dtype=np.uint32)


def write_bounds(arr_bound, x_bound, count, s_bound):
    """out_bound[j] = S + max(arr_bound[j], x_bound[j]), shared by all elements."""
    S = sum(int(b) for b in s_bound[:index_bits(count)])
    return np.array([S + max(int(a), int(x)) for a, x in zip(arr_bound, x_bound)], dtype=np.uint32)


def read_products(nbits, count):
    """Products per value at most: one per tree node above the leaves with an element below it."""
    return nbits * sum(-(-count >> t) for t in range(1, index_bits(count) + 1))


def indicator_products(count):
    """Suffix products formed while v walks 0 .. count - 1 (level k - 1 is a literal: a copy)."""
    k = index_bits(count)
    c = k - 1
    for v in range(1, count):
        top = (v & -v).bit_length() - 1
        c += top + 1 - (top == k - 1)
    return c


def write_products(nbits, count):
    return indicator_products(count) + nbits * count


def int_read(arr, i, count):
    """The plaintext semantics on integers: an index >= count (taken mod 2^k) reads 0."""
    i &= (1 << index_bits(count)) - 1
    return int(arr[i]) if i < count else 0


def int_write(arr, i, x, count):
    """... and writes nowhere."""
    i &= (1 << index_bits(count)) - 1
    out = [int(a) for a in arr]
    if i < count:
        out[i] = int(x)
    return out
