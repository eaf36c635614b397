"""Model circuits of the bit counts (count_ones, count_zeros, leading / trailing zeros / ones) over
the big-integer GF(2)[X] model (oracle/gf2_model.py): the specification the engine's
bitcount_kernel and bitrun_kernel are bit-exact against, their static degree
bounds, and the integer references.  A polynomial is a Python int; a value is the list of its bit
polynomials, least significant first; the result is the 8 bit polynomials of a Ciphered<u8>.

    literals: u_i = x_i (the "ones" ops) or x_i + 1 (the "zeros" ops)
    counts:   out_k = e_{2^k}(u_0 .. u_{n-1}), by E_j <- E_j + u_i E_{j-1} (j descending, E_0 = 1)
              over EVERY j: the plain full recurrence, nothing pruned
    runs:     v_j = u_{n-j} (leading) or u_{j-1} (trailing), t_j = v_1 .. v_j,
              out_k = sum of t_{m 2^k} over m >= 1, m 2^k <= n
    2^k > n:  the null polynomial
"""
from __future__ import annotations

import numpy as np

from borrow_model import pack  # noqa: F401  (the batch layout the tests compare with)
from oracle import gf2_model as model

#       name              (run, zeros, leading), the hm_op code
OPS = {"count_ones": (False, False, False), "count_zeros": (False, True, False),
       "leading_zeros": (True, True, True), "leading_ones": (True, False, True),
       "trailing_zeros": (True, True, False), "trailing_ones": (True, False, False)}
CODES = {name: 22 + k for k, name in enumerate(OPS)}
OUT_BITS = 8


def literals(a, zeros):
    return [x ^ 1 for x in a] if zeros else list(a)


def count_circuit(a, zeros, mul=model.clmul_fast):
    """The 8 output polynomials of count_ones (count_zeros) of the bit polynomials a."""
    n = len(a)
    E = [1] + [0] * n
    for u in literals(a, zeros):
        for j in range(n, 0, -1):
            E[j] ^= mul(u, E[j - 1])
    return [E[1 << k] if 1 << k <= n else 0 for k in range(OUT_BITS)]


def run_circuit(a, zeros, leading, mul=model.clmul_fast):
    """The 8 output polynomials of the leading (trailing) run of ones (zeros literals: zeros)."""
    n = len(a)
    u = literals(a, zeros)
    v = u[::-1] if leading else u
    t, prefix = 1, [1]
    for x in v:
        t = mul(t, x)
        prefix.append(t)  # prefix[j] = t_j
    out = []
    for k in range(OUT_BITS):
        s = 0
        for j in range(1 << k, n + 1, 1 << k):
            s ^= prefix[j]
        out.append(s)
    return out


def circuit(op, a):
    run, zeros, leading = OPS[op]
    return run_circuit(a, zeros, leading) if run else count_circuit(a, zeros)


def bitcount_bounds(op, ba):
    """Counts: out_bound[k] = the 2^k largest bounds summed; runs: the first M bounds in the run's
    order, M the largest multiple of 2^k <= n; 0 where 2^k > n."""
    run, _, leading = OPS[op]
    ba = [int(b) for b in ba]
    n = len(ba)
    out = []
    for k in range(OUT_BITS):
        if 1 << k > n:
            out.append(0)
        elif run:
            order = ba[::-1] if leading else ba
            out.append(sum(order[:(n >> k) << k]))
        else:
            out.append(sum(sorted(ba, reverse=True)[:1 << k]))
    return np.array(out, dtype=np.uint32)


def degree_of(op, n):
    """m, the circuit's degree in fresh bits: the requirement is 2m + 1."""
    return n if OPS[op][0] else 1 << (int(n).bit_length() - 1)


def needed(n, i, j):
    """After i of n literals, is E_j read by some target T = 2^k <= n?  (The rule the kernel
    prunes by; test_bitcount_host.py checks it against reachability.)"""
    T = 1
    while T <= n:
        if j <= T and T - j <= n - i:
            return True
        T <<= 1
    return False


def int_count(op, x, n):
    """The plaintext result on one Python integer x of n bits: int.bit_count and bit scans."""
    run, zeros, leading = OPS[op]
    x &= (1 << n) - 1
    if zeros:
        x ^= (1 << n) - 1  # count the ones of the complement
    if not run:
        return x.bit_count()
    bits = [(x >> i) & 1 for i in range(n)]
    r = 0
    for b in (bits[::-1] if leading else bits):
        if not b:
            break
        r += 1
    return r


def table(op):
    """The op's 256-entry byte table (the u8 function, for ctx.lookup)."""
    return np.array([int_count(op, v, 8) for v in range(256)], dtype=np.uint8)
