"""The adder prep's uniform-bound fast path (adder.hip add_prep_uniform_kernel<5>) against the
general prep kernel and the CPU oracle, bit-exact.

Operands whose bits all carry the bound 256 (fresh u32 ciphertexts at d = d' = tau = 128) take the
fast path: compile-time slot sizes, and the degrees of ab_i and P_i by arithmetic from the inputs'.
The same plaintexts and masks encrypted with bit 31's bound set to 257 have the same limb layout
(5 limbs per bit either way) but are not uniform, and 257 is no multiple of 32, so that add runs
the general kernel with product rows for every word: the two sums must agree limb for limb and
degree for degree.
"""
import numpy as np
import pytest

from helpers import as_bytes, assert_batches_equal, keys, masks, plain

pytestmark = pytest.mark.gpu

PARAMS = (128, 128, 1, 128)
SEED = 181
UNI = np.full(32, 256, dtype=np.uint32)
GEN = UNI.copy()
GEN[31] = 257


@pytest.fixture(scope="module")
def H():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import homomorph
    homomorph.lib()  # loud failure if the engine is not built
    return homomorph


@pytest.fixture(scope="module")
def world(H):
    ctx = H.Context(H.Parameters(*PARAMS))
    ctx.seed_rng(SEED)
    ctx.generate_secret_key()
    ctx.generate_public_key()
    _, pk, _ = keys(*PARAMS, SEED)
    return ctx, pk


def _both_adds(H, ctx, a, ma, b, mb):
    """a + b on the fast path (uniform bounds) and on the general kernel (bit 31's bound 257)."""
    fast = ctx.apply2(H.HomomorphicAddition, ctx.encrypt(a, masks=ma, bound=UNI),
                      ctx.encrypt(b, masks=mb, bound=UNI))
    gen = ctx.apply2(H.HomomorphicAddition, ctx.encrypt(a, masks=ma, bound=GEN),
                     ctx.encrypt(b, masks=mb, bound=GEN))
    ctx.synchronize()
    # the last bit's x bound is far below its carry bound: the same output layout
    assert np.array_equal(fast.bound, gen.bound), (fast.bound, gen.bound)
    return fast, gen


def _check(H, oracle, pk, fast, gen, a, ma, b, mb, m, k, what):
    fl, fd = H.value_slice(fast, 0, m).to_host()
    gl, gd = H.value_slice(gen, 0, m).to_host()
    assert_batches_equal(fl, fd, gl, gd, fast.bound, m, f"{what}: fast path vs general kernel")
    la, da = oracle.encrypt_batch(pk, as_bytes(a[:k]), ma[:k], UNI)
    lb, db = oracle.encrypt_batch(pk, as_bytes(b[:k]), mb[:k], UNI)
    rl, rd = oracle.add_batch(la, da, UNI, lb, db, UNI, 32, k, fast.bound)
    fl, fd = H.value_slice(fast, 0, k).to_host()
    assert_batches_equal(fl, fd, rl, rd, fast.bound, k, f"{what}: fast path vs oracle")


@pytest.mark.parametrize("n", [7, 4096, 16387])
def test_fast_path_equals_general_kernel(H, oracle, world, n):
    """Batches that reach each prep geometry: 7 (8 waves per value, 4 bits per wave), 4096 (4 waves,
    8 bits) and 16,387 (2 waves, 16 bits in two row passes; the last block is not full).  At most
    1024 values are compared on the host, 16 with the oracle."""
    ctx, pk = world
    a, b = plain(n, np.uint32, 182 + n), plain(n, np.uint32, 183 + n)
    ma, mb = masks(n, 32, 128, 184 + n), masks(n, 32, 128, 185 + n)
    fast, gen = _both_adds(H, ctx, a, ma, b, mb)
    _check(H, oracle, pk, fast, gen, a, ma, b, mb, min(n, 1024), min(n, 16), f"n = {n}")


def test_degree_arithmetic_corners(H, oracle, world):
    """One batch of 64 values with hand-made masks.  A bit whose mask is all zero is the constant
    0 (null) or 1, which gives every corner of the degree rules: null a_i, b_i or both, ab_i = 1,
    x_i = 0 with ab_i != 0.
      0..7    both operands constants in every bit
      8..15   every bit of either operand a constant with probability 1/2
      16..23  a is 0 in every bit (one operand all null), b ordinary
      24..31  a all constants, b ordinary
      32..47  b = a, masks included: add(ca, ca), x_i null in every bit
      48..63  ordinary fresh values: deg a_i = deg b_i, and the top of x_i cancels"""
    ctx, pk = world
    n = 64
    rng = np.random.default_rng(186)
    a, b = plain(n, np.uint32, 187), plain(n, np.uint32, 188)
    ma, mb = masks(n, 32, 128, 189), masks(n, 32, 128, 190)
    ma[0:8] = 0
    mb[0:8] = 0
    ma[8:16][rng.random((8, 32)) < 0.5] = 0
    mb[8:16][rng.random((8, 32)) < 0.5] = 0
    a[16:24] = 0
    ma[16:32] = 0
    b[32:48], mb[32:48] = a[32:48], ma[32:48]
    a[0], b[0] = 0xFFFFFFFF, 0xFFFFFFFF  # ab_i = 1 and x_i = 0 in every bit
    a[1], b[1] = 0, 0
    a[2], b[2] = 0xFFFFFFFF, 0
    fast, gen = _both_adds(H, ctx, a, ma, b, mb)
    _check(H, oracle, pk, fast, gen, a, ma, b, mb, n, n, "corners")
    dec = ctx.decrypt(fast)
    ctx.synchronize()
    assert np.array_equal(dec, (a + b).astype(np.uint32))


@pytest.mark.parametrize("how", ["bit_above_degree", "degree_above_bound", "top_bit_cleared"])
def test_validation_is_unchanged(H, world, how):
    """A uniform batch with one corrupted limb or degree word is refused with HM_ERR_BAD_INPUT, as
    the general kernel refuses it."""
    from homomorph import _lib
    ctx, _ = world
    n, v, i = 8, 5, 13
    a, b = plain(n, np.uint32, 191), plain(n, np.uint32, 192)
    ca = ctx.encrypt(a, masks=masks(n, 32, 128, 193), bound=UNI)
    cb = ctx.encrypt(b, masks=masks(n, 32, 128, 194), bound=UNI)
    ctx.synchronize()
    limbs, deg = ca.to_host()
    limbs, deg = limbs.copy(), deg.copy().reshape(n, 32)
    base = v * ca.stride + i * 5
    d = int(deg[v, i])
    assert 64 <= d <= 256
    if how == "bit_above_degree":
        limbs[base + (d + 1) // 64] |= np.uint64(1 << ((d + 1) % 64))
    elif how == "degree_above_bound":
        deg[v, i] = 300
    else:
        limbs[base + d // 64] &= np.uint64(~(1 << (d % 64)) & (2**64 - 1))
    for bound in (UNI, GEN):  # the fast path, then today's kernel: the same refusal
        bad = H.Ciphered.from_host(limbs, deg, bound, n, ctx.device, np.dtype(np.uint32))
        other = H.Ciphered(cb.limbs, cb.degree, bound, 32, n, cb.plain_dtype)
        with pytest.raises(H.EngineError) as ei:
            ctx.apply2(H.HomomorphicAddition, bad, other)
            ctx.synchronize()
        assert ei.value.status == _lib.ERR_BAD_INPUT, how
    ctx.synchronize()  # the flag is cleared by the check


def test_u128_add_one_row_per_bit_big_batch(H, oracle):
    """The plan's waves per value never fall below ceil(nbits / 64): a u128 add whose prep has one
    product row per bit (bound 32: two words, the top one a copy) at a batch of 16,384 asked for
    one wave per value, 128 bits in a wave, and was refused as unsupported.  An add needs
    d >= 21 delta, so the bound 32 is d = 24, d' = 8 here.  8 values equal the oracle's."""
    params = (24, 8, 1, 8)
    ctx = H.Context(H.Parameters(*params))
    ctx.seed_rng(195)
    ctx.generate_secret_key()
    ctx.generate_public_key()
    _, pk, _ = keys(*params, 195)
    n, k = 16384, 8
    rng = np.random.default_rng(196)
    av = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    bv = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    ma, mb = masks(n, 128, 8, 197), masks(n, 128, 8, 198)
    bound = np.full(128, 32, dtype=np.uint32)
    s = ctx.apply2(H.HomomorphicAddition, ctx.encrypt(av, masks=ma, bound=bound),
                   ctx.encrypt(bv, masks=mb, bound=bound))
    ctx.synchronize()
    la, da = oracle.encrypt_batch(pk, av[:k], ma[:k], bound)
    lb, db = oracle.encrypt_batch(pk, bv[:k], mb[:k], bound)
    rl, rd = oracle.add_batch(la, da, bound, lb, db, bound, 128, k, s.bound)
    gl, gd = H.value_slice(s, 0, k).to_host()
    assert_batches_equal(gl, gd, rl, rd, s.bound, k, "u128 add, one row per bit")
