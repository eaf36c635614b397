"""The MFMA carry chain's rotating wave priorities (adder_mfma.hip, HM_CHAIN_PRIO): each wave reads
its slot on its SIMD once and, at the top of every bit, picks one of four `s_setprio` immediates
by scalar branches.  None of that may reach a result bit, so every assertion here is bit-exact:

  - each chunk-count instance (NC = 7, 13, 25) at batch sizes where a SIMD holds different numbers
    of chain waves and the last block is ragged (n = 1, 3, 4, 5, 17 at four waves per block),
    against the CPU oracle, limbs and degrees;
  - one batch that gives some SIMDs two waves and others one (n = 1100), the MFMA chain limb for
    limb against the VALU chain on the same inputs.

What they would catch: SCC, VCC or M0 clobbered around the scalar switch (a wrong branch, a wrong
record DMA address), a branch that is not wave-uniform, an early-exit wave that leaves its block
short.  `reference(nc)` needs no GPU; the oracle runs once per instance on 17 values and the
smaller batches are its first n values.
"""
import functools

import numpy as np
import pytest

from helpers import as_bytes, assert_batches_equal, fresh_bound, keys, masks, offsets, plain

pytestmark = pytest.mark.gpu

SEED = 47
NMAX = 17
BATCHES = (1, 3, 4, 5, 17)
INSTANCES = {7: ((64, 64, 1, 64), np.uint16),
             13: ((128, 128, 1, 128), np.uint16),
             25: ((256, 256, 1, 256), np.uint8)}


@pytest.fixture(scope="module")
def H():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import homomorph
    homomorph.lib()  # loud failure if the engine is not built
    return homomorph


def _inputs(nc, n=NMAX):
    params, dtype = INSTANCES[nc]
    nbits = 8 * np.dtype(dtype).itemsize
    a, b = plain(n, dtype, 100 + nc), plain(n, dtype, 200 + nc)
    ma, mb = masks(n, nbits, params[3], 300 + nc), masks(n, nbits, params[3], 400 + nc)
    return params, dtype, nbits, a, b, ma, mb, fresh_bound(params[0], params[1], nbits)


@functools.lru_cache(maxsize=None)
def reference(nc):
    """The oracle's add of the instance's NMAX values (computed once, shared, read-only)."""
    import homomorph as H
    from oracle import oracle_py as oracle
    oracle.build()
    params, dtype, nbits, a, b, ma, mb, bound = _inputs(nc)
    sk, pk, _ = keys(*params, SEED)
    la, da = oracle.encrypt_batch(pk, as_bytes(a), ma, bound)
    lb, db = oracle.encrypt_batch(pk, as_bytes(b), mb, bound)
    ob = H.add_out_bounds(bound, bound)
    rl, rd = oracle.add_batch(la, da, bound, lb, db, bound, nbits, NMAX, ob)
    rl = np.asarray(rl, dtype=np.uint64).reshape(-1)
    rd = np.asarray(rd, dtype=np.uint32).reshape(-1)
    for v in (rl, rd):
        v.setflags(write=False)
    return dict(ob=ob, rl=rl, rd=rd)


def _context(H, params):
    ctx = H.Context(H.Parameters(*params))
    ctx.seed_rng(SEED)
    ctx.generate_secret_key()
    ctx.generate_public_key()
    return ctx


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("nc", sorted(INSTANCES))
def test_instance_batches_equal_oracle(H, nc, n):
    """n values through the forced MFMA chain: the oracle's limbs and degrees, bit for bit."""
    ref = reference(nc)
    params, dtype, nbits, a, b, ma, mb, bound = _inputs(nc)
    ctx = _context(H, params)
    ctx.set_add_options("mfma")
    ca = ctx.encrypt(a[:n], masks=ma[:n], bound=bound)
    cb = ctx.encrypt(b[:n], masks=mb[:n], bound=bound)
    cs = ctx.apply2(H.HomomorphicAddition, ca, cb)
    dec = ctx.decrypt(cs)
    ctx.synchronize()
    assert np.array_equal(cs.bound, ref["ob"])
    _, _, stride = offsets(ref["ob"])
    gl, gd = cs.to_host()
    assert_batches_equal(gl, gd, ref["rl"][:n * stride], ref["rd"][:n * nbits], ref["ob"], n,
                         f"NC={nc} n={n}")
    assert np.array_equal(dec, (a[:n] + b[:n]).astype(dtype))


def test_uneven_simd_fill_equals_valu_chain(H):
    """1100 u8 values at d + d' = 128: 275 blocks of four waves over 1024 SIMDs, so some SIMDs
    hold two chain waves and others one.  The MFMA chain against the VALU chain, limb for limb."""
    params, dtype, n, nbits = (64, 64, 1, 64), np.uint8, 1100, 8
    a, b = plain(n, dtype, 501), plain(n, dtype, 502)
    ma, mb = masks(n, nbits, params[3], 503), masks(n, nbits, params[3], 504)
    bound = fresh_bound(params[0], params[1], nbits)
    ctx = _context(H, params)
    ca = ctx.encrypt(a, masks=ma, bound=bound)
    cb = ctx.encrypt(b, masks=mb, bound=bound)
    got = {}
    for chain in ("mfma", "valu"):
        ctx.set_add_options(chain)
        cs = ctx.apply2(H.HomomorphicAddition, ca, cb)
        dec = ctx.decrypt(cs)
        ctx.synchronize()
        assert np.array_equal(dec, (a + b).astype(dtype)), chain
        got[chain] = (cs.to_host(), np.asarray(cs.bound))
    (ml, md), mbnd = got["mfma"]
    (vl, vd), vbnd = got["valu"]
    assert np.array_equal(mbnd, vbnd)
    assert_batches_equal(ml, md, vl, vd, mbnd, n, "n=1100 mfma vs valu")
