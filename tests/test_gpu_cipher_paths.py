"""GPU: every encrypt, decrypt and mask-draw kernel variant of csrc/cipher.hip at its dispatch edges
(tests/cipher_paths.py, synth.DEC_PATH_CASES), exact against the C oracle and the ChaCha20
restatement of tests/helpers.py.

Each case is named for the kernel variant and branch it reaches; test_cipher_paths.py (CPU) holds
the names against a plain-Python restatement of launch_enc_pc / launch_decrypt, so the path
assertions run without a GPU and this file only compares results.  There is no tolerance
anywhere: limbs, degree words, plaintext bytes and keystream bytes are compared for equality, and
every case ends on a clean ctx.synchronize().

Outputs are written into views of larger, sentinel-filled tensors (a guard band on both sides):
the sentinel must survive outside the view and be gone from every word inside it, which is the
only check that sees a store masked one lane too wide or a zero fill one limb too long.  The
kernels write inside memory the test owns either way.
"""
import ctypes

import numpy as np
import pytest

import cipher_paths as cp
import synth
from helpers import assert_batches_equal, keys, seeded_random_bytes, seeded_value_masks

pytestmark = pytest.mark.gpu

PAD = 512                      # guard words on each side of an output
SENT64 = 0x5A5AA5A55A5AA5A5    # (fits int64 / int32 / uint8 without a sign flip)
SENT32 = 0x5A5AA5A5
SENT8 = 0xA5


@pytest.fixture(scope="module")
def H():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import homomorph
    homomorph.lib()  # loud failure if the engine is not built
    return homomorph


@pytest.fixture(scope="module")
def keyed(H):
    """One context per loaded key (tau, pc, kind): the rows are uploaded and tabulated once."""
    cache = {}

    def get(tau, pc, kind):
        k = (tau, pc, kind)
        if k not in cache:
            ctx = H.Context(H.Parameters(64, 64, 1, 64))
            ctx.set_public_key(H.PublicKey(cp.make_key(tau, pc, kind)))
            cache[k] = ctx
        return cache[k]
    return get


@pytest.fixture(scope="module")
def dec_world(H):
    """The seeded context of synth.DEC_PARAMS (its secret key decrypts the synthetic operands)."""
    ctx = H.Context(H.Parameters(*synth.DEC_PARAMS))
    ctx.seed_rng(synth.SEED)
    ctx.generate_secret_key()
    return ctx


def guarded(torch, device, words, dtype, sentinel):
    """(whole tensor, the view of `words` elements PAD in from both ends), all sentinel."""
    big = torch.full((words + 2 * PAD,), sentinel, dtype=dtype, device=device)
    return big, big[PAD:PAD + words]


def guard_intact(big, words, sentinel):
    return bool((big[:PAD] == sentinel).all()) and bool((big[PAD + words:] == sentinel).all())


def offset_copy(torch, host, device, off):
    """The bytes of `host` on the device, `off` bytes past a 16-byte-aligned address."""
    flat = np.ascontiguousarray(host).reshape(-1)
    buf = torch.zeros(flat.size + 16, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + flat.size]
    view.copy_(torch.from_numpy(flat))
    assert view.data_ptr() % 16 == off % 16
    return view


def encrypt_guarded(H, ctx, data, masks, bound, off=0):
    """hm_encrypt_batch into a guarded output.  Returns (limbs, degree words) on the host after
    checking the guard bands and that no sentinel is left inside."""
    import torch
    n, nbytes = data.shape
    bound = np.ascontiguousarray(bound, dtype=np.uint32)
    nbits, stride = bound.size, H.batch_stride(bound)
    big_l, lv = guarded(torch, ctx.device, n * stride, torch.int64, SENT64)
    big_d, dv = guarded(torch, ctx.device, n * nbits, torch.int32, SENT32)
    out = H.Ciphered(lv, dv.view(n, nbits), bound, nbits, n)
    c = out._c()
    dev_data = torch.from_numpy(np.ascontiguousarray(data)).to(ctx.device)
    dev_masks = offset_copy(torch, masks, ctx.device, off)
    ctx._launch(lambda: H.lib().hm_encrypt_batch(ctx._h, dev_data.data_ptr(), nbytes,
                                                 dev_masks.data_ptr(), ctypes.byref(c)), "encrypt")
    ctx.synchronize()
    assert guard_intact(big_l, n * stride, SENT64), "limbs written outside the batch"
    assert guard_intact(big_d, n * nbits, SENT32), "degree words written outside the batch"
    assert not bool((lv == SENT64).any()), "a limb inside the batch was not written"
    assert not bool((dv == SENT32).any()), "a degree word inside the batch was not written"
    return out.to_host()


# ------------------------------------------------------------------ encryption
@pytest.mark.parametrize("name", list(cp.ENC_CASES))
def test_encrypt(H, keyed, oracle, name):
    """hm_encrypt_batch under LOADED keys of chosen shape, limb for limb against
    oracle.encrypt_batch on the same rows, data and masks.  The keys are seeded random rows, not
    a key pair: NOTHING HERE DECRYPTS, and no round trip can be added to these cases.

    launch_enc_pc (cipher.hip) picks the kernel; the case name gives the variant, the restatement
    (cipher_paths.enc_dispatch, held on the CPU by test_cipher_paths.py) the flags:
      top1_*    encrypt_table_kernel<PC,32,TOP1>: `E.tau == 128 && aligned && E.top1 && PC > 1`;
                PC = 2, 3 (one table pair), 4, 9, 17 and a key with topcol = 0; enc_lookup2<PC - 1>
                takes `if constexpr (PC % 2)` at even PC
      gc32_*    encrypt_table_kernel<PC,32>: tau = 128 with a top limb above 1, odd and even PC
      gc0_*     encrypt_table_kernel<PC,0>: tau = 1, 3, 4, 5, 33, 40, 100 (`(mb & 3u) != 0`, byte
                mask reads; G no multiple of 8; rows past tau in the last nibble group), 64 and
                the tau = 128 calls whose masks sit 8 bytes off a 16-byte boundary (`mb & 3 ==
                0`, word reads), tau = 130; the last table that fits (tau = 1536 at PC = 2) and
                the last LDS budget that does (tau = 160 at PC = 17)
      fallback_table_*  encrypt_kernel<PC>: `tab <= kEncTableBytes` fails (tau = 1537, 2048 at PC = 2)
      fallback_lds_*    encrypt_kernel<PC>: the table is built but `lds <= 160 * 1024` fails
                (PC = 16 at tau = 192, PC = 17 at tau = 168)
      *_n1_u8, *_n9_u8  8 and 72 ciphertext bits: less than a wave; a wave and 8 bits (`lim`)
      *_3byte   `E.lognbits = -1`: the value index by division;  *_16byte: HM_MAX_BITS bits
      *_zero_fill      per-bit capacities PC .. PC + 3: `for (l = PC; l < cap; ++l) dst[l] = 0`
      *_rows_padded_*  rows of 5 (2) limbs with degrees <= 100 (40) into capacity 2 (1): `if (l <
                cap) dst[l] = acc[l]`, the dropped limbs zero, so no capacity flag
      *_strides three grid strides at per_cu = 1, n from the card's CU count (stride_n): the
                prefetched mask of `t0 + step`, a third pass in three blocks, a partial last wave
      unsupported_pc18            `c->pk_cap > 17`: HM_ERR_UNSUPPORTED
      invalid_bound_below_maxdeg  `out->bound[i] < c->pk_maxdeg`: HM_ERR_INVALID_ARGUMENT
    Every batch sits in a guard band (encrypt_guarded)."""
    import torch
    from homomorph import _lib
    c = cp.ENC_CASES[name]
    ctx = keyed(c.tau, c.pc, c.kind)
    cus = torch.cuda.get_device_properties(ctx.device).multi_processor_count
    n = c.n if c.n is not None else cp.stride_n(c, cus)
    if c.n is None:  # the count was derived for this card: it does take its strides here
        d = c.dispatch(cus, n)
        assert d["strides"] == cp.STRIDES and d["partial_wave"] and d["kernel"] == c.kernel
    data, masks = cp.enc_inputs(name, n)
    bound = c.bounds()
    if c.status != "ok":
        with pytest.raises(H.EngineError) as ei:
            ctx.encrypt(data, masks=masks, bound=bound)
        assert ei.value.status == {"unsupported": _lib.ERR_UNSUPPORTED,
                                   "invalid": _lib.ERR_INVALID_ARGUMENT}[c.status]
        ctx.synchronize()
        return
    gl, gd = encrypt_guarded(H, ctx, data, masks, bound, c.off)
    rl, rd = oracle.encrypt_batch(c.rows(), data, masks, bound)
    assert_batches_equal(gl, gd, rl, rd, bound, n, name)
    if c.off:  # the aligned call of the same masks is the other variant; both equal the oracle
        al, ad = encrypt_guarded(H, ctx, data, masks, bound, 0)
        assert_batches_equal(al, ad, rl, rd, bound, n, name + " (aligned)")
    ctx.synchronize()


# ------------------------------------------------------------------ decryption
@pytest.mark.parametrize("name", list(synth.DEC_PATH_CASES))
def test_decrypt(H, dec_world, oracle, name):
    """hm_decrypt_batch on synthetic operands that fill their bounds (synth.operands: FULL, MONO,
    ONES, ... scheduled per value and bit), byte for byte against oracle.decrypt_batch and the
    model's decipher_bit (synth.dec_reference, every bit of every value).  launch_decrypt
    (cipher.hip; paths by synth.check_dec_path on the CPU):
      bits_ucap_c{1,8}_n{1,3,9}  decrypt_bits_kernel, `if (D.ucap)`: C = 1 and the last C = 8; 8,
                24 and 72 bits in all -- `lim = (total - g0) * C` on a partly filled wave, the byte
                tail of the ballot store
      bits_ucap_c*_16byte_n3     the same at 128 bits per value: 384 bits, one block and a half
      bits_general_16byte_caps1_32_n3  the general path with both HM_MAX_BITS LDS arrays full,
                per-bit capacities 1 .. 32 (`D.maxcap <= 32`, the last on this kernel), each reached
      wave_16byte_wide_n5  decrypt_kernel: bits 0, 1, 62, 63, 64, 65, 127 of 193, 255, 256, 257,
                449, 512, 513 limbs -- the unrolled body `k + (kDecUnroll - 1) * kWave < cap`
                entered by lane 0 only, by 63 lanes, by all; one and two rounds; every tail
                length; plaintext words m0 and m1 on both sides of bit 64; n = 5 leaves three
                idle waves in the second block
      wave_u8_cap512_n6    every bit two full unrolled rounds, no tail
    The plaintext lands in a guard band as well."""
    import torch
    ctx = dec_world
    c = synth.inputs("dec", name)
    la, da, _, _ = synth.packed("dec", name)
    n, nbits = c["n"], c["nbits"]
    a = H.Ciphered.from_host(la, da, c["ba"], n, ctx.device, None)
    big, view = guarded(torch, ctx.device, n * nbits // 8, torch.uint8, SENT8)
    cb = a._c()
    ctx._launch(lambda: H.lib().hm_decrypt_batch(ctx._h, ctypes.byref(cb), view.data_ptr()), "decrypt")
    ctx.synchronize()
    assert guard_intact(big, n * nbits // 8, SENT8), "plaintext written outside the batch"
    got = view.cpu().numpy().reshape(n, nbits // 8)
    sk, _, _ = keys(*synth.DEC_PARAMS, synth.SEED)
    assert np.array_equal(got, oracle.decrypt_batch(sk, la, da, c["ba"], nbits, n)), name
    assert np.array_equal(got, synth.dec_reference(name)), name
    # the public entry (its own output tensor) agrees
    assert np.array_equal(ctx.decrypt_bytes(a).cpu().numpy(), got)
    ctx.synchronize()


# ------------------------------------------------------------------ mask draw
def _draw_into(H, ctx, view):
    ctx._launch(lambda: H.lib().hm_random_bytes(ctx._h, view.data_ptr(), view.numel()), "random_bytes")


def _assert_draw(got, seed, draw, length, what):
    for lo, hi in cp.draw_windows(length):
        want = seeded_random_bytes(seed, draw, hi - lo, start=lo)
        assert np.array_equal(got[lo:hi], want), f"{what}: bytes [{lo}, {hi}) of draw {draw}"


def _draw_lengths(H, oracle):
    """hm_random_bytes at every length of cp.DRAW_LENGTHS, one after the other on one seeded
    context: rand_fill_kernel's last block (`blk * 64 + 64 <= R.nbytes` else the byte loop), its
    block-of-threads edge at 16384 bytes, lengths below one ChaCha20 block.  Every non-empty draw
    uses the next nonce; an empty one launches nothing and leaves the nonce.  Each draw writes its
    nbytes and nothing else (guard band)."""
    import torch
    ctx = H.Context(H.Parameters(64, 64, 1, 64))
    ctx.seed_rng(cp.DRAW_SEED)
    draw = 0
    for length in cp.DRAW_LENGTHS:
        big, view = guarded(torch, ctx.device, length, torch.uint8, SENT8)
        assert view.data_ptr() % 16 == 0
        _draw_into(H, ctx, view)
        ctx.synchronize()
        assert guard_intact(big, length, SENT8), f"a draw of {length} bytes wrote outside them"
        _assert_draw(view.cpu().numpy(), cp.DRAW_SEED, draw, length, f"length {length}")
        draw += length > 0
    assert draw == len(cp.DRAW_LENGTHS) - 1
    # the public entry continues the sequence
    assert np.array_equal(ctx.random_bytes(100).cpu().numpy(), seeded_random_bytes(cp.DRAW_SEED, draw, 100))


def _draw_misaligned(H, oracle):
    """A destination that is not 16-byte aligned sends FULL blocks down rand_fill_kernel's byte
    path (`((uintptr_t)dst & 15u) == 0` fails): 16385 bytes into buf[1:] and into buf[8:] of a
    sentinel tensor carry the same keystream an aligned draw at that nonce does, and the
    sentinel survives on both sides."""
    import torch
    ctx = H.Context(H.Parameters(64, 64, 1, 64))
    ctx.seed_rng(cp.DRAW_SEED + 1)
    L = cp.DRAW_MISALIGN_LEN
    for draw, off in enumerate(cp.DRAW_MISALIGN):
        big = torch.full((L + 2 * PAD,), SENT8, dtype=torch.uint8, device=ctx.device)
        assert big.data_ptr() % 16 == 0 and PAD % 16 == 0
        view = big[PAD + off:PAD + off + L]
        assert view.data_ptr() % 16 == off
        _draw_into(H, ctx, view)
        ctx.synchronize()
        assert bool((big[:PAD + off] == SENT8).all()) and bool((big[PAD + off + L:] == SENT8).all())
        _assert_draw(view.cpu().numpy(), cp.DRAW_SEED + 1, draw, L, f"offset {off}")
    aligned = ctx.random_bytes(L).cpu().numpy()  # and the aligned draw at the next nonce
    _assert_draw(aligned, cp.DRAW_SEED + 1, len(cp.DRAW_MISALIGN), L, "aligned")


def _engine_masks(H, oracle):
    """Encryption with engine-drawn masks (masks = None) at tau = 33 (5 mask bytes per bit, `mb &
    3 != 0`) and n * nbits * mb = 360 bytes, no multiple of 64 (hm_encrypt_batch rounds the mask
    buffer up): the oracle, fed the seeded ChaCha20 bytes of the same draw, gives the same limbs.
    Two encryptions of 9 values, then one of 37, for which d_masks grows between draws."""
    e = cp.ENGINE_MASKS
    seed = cp.DRAW_SEED + 2
    rows = cp.make_key(e["tau"], e["pc"], e["kind"])
    ctx = H.Context(H.Parameters(64, 64, 1, 64))
    ctx.seed_rng(seed)
    ctx.set_public_key(H.PublicKey(rows))
    nbits = 8 * e["nbytes"]
    bound = np.full(nbits, 64 * e["pc"] - 1, dtype=np.uint32)
    assert ctx.mask_bytes() == 5
    for draw, n in enumerate(e["n"]):
        data = np.random.default_rng([seed, draw]).integers(0, 256, size=(n, e["nbytes"]), dtype=np.uint8)
        c = ctx.encrypt(data, bound=bound)
        ctx.synchronize()
        m = seeded_value_masks(seed, draw, np.arange(n), nbits, ctx.mask_bytes())
        rl, rd = oracle.encrypt_batch(rows, data, m, bound)
        gl, gd = c.to_host()
        assert_batches_equal(gl, gd, rl, rd, bound, n, f"engine masks, draw {draw}")
    # the encryption kernel advanced the nonce each time: the next draw is number 3
    assert np.array_equal(ctx.random_bytes(64).cpu().numpy(), seeded_random_bytes(seed, len(e["n"]), 64))


def _refused_encrypt_draws_nothing(H, oracle):
    """hm_encrypt_batch refuses a key of 18 limbs per row BEFORE it draws masks (capi.cpp: "reject
    the rest BEFORE a mask draw"): with masks = None the refusal leaves the CSPRNG where it was,
    and the next draw is the next seeded ChaCha20 draw."""
    from homomorph import _lib
    c = cp.ENC_CASES["unsupported_pc18"]
    seed = cp.DRAW_SEED + 3
    ctx = H.Context(H.Parameters(64, 64, 1, 64))
    ctx.seed_rng(seed)
    ctx.set_public_key(H.PublicKey(c.rows()))
    assert np.array_equal(ctx.random_bytes(200).cpu().numpy(), seeded_random_bytes(seed, 0, 200))
    data, _ = cp.enc_inputs("unsupported_pc18", c.n)
    with pytest.raises(H.EngineError) as ei:
        ctx.encrypt(data, bound=c.bounds())
    assert ei.value.status == _lib.ERR_UNSUPPORTED
    ctx.synchronize()
    assert np.array_equal(ctx.random_bytes(200).cpu().numpy(), seeded_random_bytes(seed, 1, 200))


DRAW_CASES = {"lengths": _draw_lengths, "misaligned": _draw_misaligned,
              "engine_masks": _engine_masks, "refused_encrypt_draws_nothing": _refused_encrypt_draws_nothing}


@pytest.mark.parametrize("name", list(DRAW_CASES))
def test_draw(H, oracle, name):
    """rand_fill_kernel (cipher.hip), one 64-byte ChaCha20 block per thread, against the
    pure-Python generator of tests/helpers.py (seeded_random_bytes).  Cases (each function's
    docstring has the branch): lengths, misaligned, engine_masks, refused_encrypt_draws_nothing."""
    DRAW_CASES[name](H, oracle)
