"""Model circuit of the shifts and rotates by an encrypted amount over the big-integer GF(2)[X]
model (oracle/gf2_model.py): the specification the engine's shift_kernel is bit-exact against
(DESIGN.md s4.4d), and its static degree bounds.  A polynomial is a Python int; a value is the list
of its bit polynomials, least significant first.

    n = len(a) a power of two, L = log2 n; one stage per amount bit s_t, step k = 2^t:
        y_i = x_i + s_t (x_i + x_src(i))
    shl: src = i - k    shr: src = i + k    (outside 0..n-1: null; signed shr: x_{n-1})
    rotl: src = (i - k) mod n    rotr: src = (i + k) mod n

The stages are commuting linear maps of the value, so any stage order gives the same polynomials;
the model runs them in ascending order unless told otherwise.  Batch packing: borrow_model.pack.
"""
from __future__ import annotations

import numpy as np

from borrow_model import pack  # noqa: F401  (the batch layout the tests compare with)
from oracle import gf2_model as model

OPS = ("shl", "shr", "rotl", "rotr")
MODES = (("shl", False), ("shr", False), ("shr", True), ("rotl", False), ("rotr", False))


def stages(n):
    L = int(n).bit_length() - 1
    assert 2 <= n <= 128 and n == 1 << L, "a shifted value has a power of two of bits in 2..128"
    return L


def source(op, n, k, i, signed=False):
    """The bit a stage of step k mixes into bit i; None: the null polynomial."""
    if op == "shl":
        return i - k if i >= k else None
    if op == "shr":
        return i + k if i + k < n else (n - 1 if signed else None)
    if op == "rotl":
        return (i - k) % n
    assert op == "rotr"
    return (i + k) % n


def shift_circuit(op, a, s, signed=False, order=None):
    """The output bit polynomials of a (op) s: a has n bits, s at least log2 n (its low ones are
    read).  order: the stages' order (default ascending)."""
    n = len(a)
    L = stages(n)
    assert len(s) >= L
    x = list(a)
    for t in (range(L) if order is None else order):
        y = []
        for i in range(n):
            j = source(op, n, 1 << t, i, signed)
            y.append(x[i] ^ model.clmul(s[t], x[i] ^ (x[j] if j is not None else 0)))
        x = y
    return x


def shift_bounds(op, ba, bs):
    """out_bound[j] = the sum of the amount's low log2 n bounds plus the widest bound of a among
    the bits that can reach bit j (at or below j: shl; at or above: shr; all: the rotates)."""
    n = len(ba)
    L = stages(n)
    S = sum(int(b) for b in bs[:L])
    ba = [int(b) for b in ba]
    if op == "shl":
        reach = [max(ba[:j + 1]) for j in range(n)]
    elif op == "shr":
        reach = [max(ba[j:]) for j in range(n)]
    else:
        reach = [max(ba)] * n
    return np.array([S + r for r in reach], dtype=np.uint32)


def numpy_shift(op, v, s, signed=False):
    """The plaintext results by numpy's own <<, >> and | on v (an unsigned array of 8..64-bit
    values: the bit patterns) and the amounts s, taken mod the width; the same unsigned dtype."""
    n = 8 * v.dtype.itemsize
    k = (np.asarray(s).astype(np.uint64) % np.uint64(n)).astype(v.dtype)
    back = ((np.uint64(n) - k.astype(np.uint64)) % np.uint64(n)).astype(v.dtype)
    if op == "shl":
        return v << k
    if op == "shr":
        if signed:
            sv = v.view(np.dtype(f"i{v.dtype.itemsize}"))
            return (sv >> k.astype(sv.dtype)).view(v.dtype)
        return v >> k
    if op == "rotl":
        return (v << k) | (v >> back)
    assert op == "rotr"
    return (v >> k) | (v << back)


def int_shift(op, x, k, n, signed=False):
    """The same on one Python integer x of n bits (any width: numpy has no u128)."""
    k %= n
    mask = (1 << n) - 1
    if op == "shl":
        return (x << k) & mask
    if op == "shr":
        r = x >> k
        return r | (mask & ~(mask >> k)) if signed and x >> (n - 1) else r
    if op == "rotl":
        return ((x << k) | (x >> (n - k))) & mask
    assert op == "rotr"
    return ((x >> k) | (x << (n - k))) & mask
