"""What the GPU tests of the wave-per-value circuits share (test_gpu_compare, test_gpu_select,
test_gpu_lookup, test_gpu_shift): the engine's loader, the per-parameter-set contexts with the
oracle's keys, and one operand encrypted on both sides.  Each module wraps the first two in
fixtures of its own."""
import numpy as np

from helpers import as_bytes, bit_ints, keys, masks


def load_engine():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import homomorph
    homomorph.lib()  # loud failure if the engine is not built
    return homomorph


def make_world(H, seed):
    """Contexts and oracle keys per parameter set, made once (same seed on both sides)."""
    cache = {}

    def get(params):
        if params not in cache:
            ctx = H.Context(H.Parameters(*params))
            ctx.seed_rng(seed)
            ctx.generate_secret_key()
            ctx.generate_public_key()
            cache[params] = (ctx, keys(*params, seed))
        return cache[params]
    return get


def encrypt_both(H, oracle, world, params, vals, mask_seed, bound=None, zero_masks=False,
                 wide=False):
    """(device batch, its model polynomials per value) of one operand; vals: an integer array, or
    (wide) the (n, nbytes) little-endian bytes of wider values."""
    ctx, (sk, pk, _) = world(params)
    raw = vals if wide and vals.ndim == 2 else as_bytes(vals)
    n, nbits = raw.shape[0], 8 * raw.shape[1]
    m = masks(n, nbits, params[3], mask_seed)
    if zero_masks:
        m[:] = 0
    if bound is None:
        bound = np.full(nbits, params[0] + params[1], np.uint32)
    dev = ctx.encrypt(vals, masks=m, bound=bound)
    l, d = oracle.encrypt_batch(pk, raw, m, bound)
    return dev, [bit_ints(l, d, bound, e) for e in range(n)]
