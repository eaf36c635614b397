"""The cipher kernels' dispatch, restated, and the case table of the cipher-paths tier.

csrc/cipher.hip picks its kernel variants on the host (launch_enc_pc, launch_decrypt) from the
key's shape, the output bounds, the mask pointer and the LDS budget, and the kernels branch again
inside (uniform_cap, mb & 3, lognbits, odd / even limb counts, the grid stride, the last wave's
store mask).  enc_dispatch / dec_dispatch restate those decisions in plain Python from the
constants of engine.h and cipher.hip; every case below is named for the path it reaches and
test_cipher_paths.py (CPU) holds each name against the restatement, so a case that stops reaching
its path fails there.  test_gpu_cipher_paths.py then runs the engine on the same cases, limb for
limb against the C oracle.

Encryption keys are LOADED (hm_ctx_set_public_key takes any (tau, limbs_per_poly)), not
generated: seeded random rows of a chosen shape reach every (tau, PC, top1) without running keygen
at large parameters.  They are no key pair: nothing encrypted under them decrypts.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

# ------------------------------------------------------------------ constants, quoted
K_ENC_TABLE_BYTES = 96 * 1024  # engine.h kEncTableBytes: largest nibble table staged in LDS
K_ENC_BLOCK = 512              # cipher.hip kEncBlock: threads of an encrypt_table_kernel block
LDS_BYTES = 160 * 1024         # cipher.hip launch_enc_pc: `lds <= 160 * 1024`, one CU's LDS
HM_MAX_BITS = 128              # include/homomorph_gpu.h
MAX_PC = 17                    # cipher.hip launch_encrypt: `case 17`, then HM_ERR_UNSUPPORTED
DEC_BITS_MAXCAP = 32           # cipher.hip launch_decrypt: `D.maxcap <= 32`
DEC_UCAP_MAX = 8               # capi.cpp hm_decrypt_batch: `cap_of(in->bound[0]) <= 8`
DEC_WAVES_PER_BLOCK = 4        # cipher.hip launch_decrypt: `wpb = 4u`
DEC_UNROLL = 4                 # cipher.hip kDecUnroll
RAND_BLOCK_BYTES = 64 * 256    # cipher.hip launch_random: one 64-byte ChaCha20 block per thread
SEED = 5150


def caps(bound):
    return np.asarray(bound, dtype=np.uint32) // 64 + 1


# ------------------------------------------------------------------ the dispatch, restated
def key_top1(rows):
    """hm_ctx_set_public_key: `c->pk_top1 = tau <= 128 && lpp > 1` and no top limb above 1."""
    tau, pc = rows.shape
    return bool(tau <= 128 and pc > 1 and int(rows[:, pc - 1].max()) <= 1)


def table_bytes(tau, pc):
    """upload_pk / launch_enc_pc: `tab = ((tau + 3) / 4) * ((PC + 1) / 2) * 16 * 16`."""
    return ((tau + 3) // 4) * ((pc + 1) // 2) * 256


def enc_lds(tau, pc, t1=False):
    """launch_enc_pc: `lds = (t1 ? tab1 : tab) + kEncBlock * PC * 8 + 2 * HM_MAX_BITS * 4`, with
    `tab1 = ((tau + 3) / 4) * (PC / 2) * 16 * 16` (the table without the top limb)."""
    tab = ((tau + 3) // 4) * (pc // 2) * 256 if t1 else table_bytes(tau, pc)
    return tab + K_ENC_BLOCK * pc * 8 + 2 * HM_MAX_BITS * 4


def enc_dispatch(tau, pc, top1, bound, nbytes, n, cus, masks_aligned=True):
    """What hm_encrypt_batch (capi.cpp) and launch_enc_pc (cipher.hip) decide for one call: a dict
    of the kernel variant, the branch flags the kernel then takes and the grid strides of the
    busiest wave.  top1: key_top1 of the loaded rows; bound: the output's per-bit bounds;
    masks_aligned: `((uintptr_t)E.masks & 15u) == 0`."""
    if pc == 0 or pc > MAX_PC:  # `if (c->pk_cap == 0 || c->pk_cap > 17) return HM_ERR_UNSUPPORTED`
        return dict(kernel="unsupported")
    nbits = 8 * nbytes
    cap = caps(bound)
    assert cap.size == nbits
    lognbits = -1  # `for (s < 8) if ((8u * nbytes) == (1u << s)) E.lognbits = s`
    for s in range(8):
        if nbits == 1 << s:
            lognbits = s
    mb = (tau + 7) // 8
    threads = n * nbits
    tab = table_bytes(tau, pc)
    has_tab = tab <= K_ENC_TABLE_BYTES  # upload_pk: `words * 8 <= kEncTableBytes`
    # `E.top1 = c->pk_top1 && c->d_pk_tab1`; `t1 = E.tau == 128 && aligned && E.top1 && PC > 1`
    t1 = tau == 128 and masks_aligned and top1 and has_tab and pc > 1
    lds = enc_lds(tau, pc, t1)
    out = dict(uniform_cap=bool((cap == pc).all()), lognbits=lognbits, mask_words=mb % 4 == 0,
               mb=mb, partial_wave=threads % 64 != 0, lds=lds, table=tab)
    if has_tab and lds <= LDS_BYTES:  # `E.pk_tab && tab <= kEncTableBytes && lds <= 160 * 1024`
        want = (threads + K_ENC_BLOCK - 1) // K_ENC_BLOCK
        per_cu = max(1, min(4, LDS_BYTES // lds))
        blocks = min(want, cus * per_cu)
        if t1:
            kernel = f"encrypt_table_kernel<{pc},32,TOP1>"
            out["odd_lookup"] = (pc - 1) % 2 == 1  # enc_lookup2<PL = PC - 1>: `if constexpr (PC % 2)`
        elif tau == 128 and masks_aligned:
            kernel = f"encrypt_table_kernel<{pc},32>"
            out["odd_lookup"] = pc % 2 == 1
        else:
            kernel = f"encrypt_table_kernel<{pc},0>"
        step = blocks * K_ENC_BLOCK
        out.update(kernel=kernel, per_cu=per_cu, blocks=blocks,
                   strides=(threads + step - 1) // step if threads else 0)
    else:
        out.update(kernel=f"encrypt_kernel<{pc}>", blocks=(threads + 255) // 256, strides=1,
                   fallback="table" if not has_tab else "lds")
    return out


def dec_dispatch(bound, n):
    """hm_decrypt_batch / launch_decrypt: D.ucap = the common capacity when every bit's is equal
    and at most 8 limbs; `D.maxcap <= 32` picks decrypt_bits_kernel (one lane per bit), else
    decrypt_kernel (one wave per value, four waves per block)."""
    cap = caps(bound).tolist()
    ucap = cap[0] if len(set(cap)) == 1 and cap[0] <= DEC_UCAP_MAX else 0
    total = n * len(cap)
    if max(cap) <= DEC_BITS_MAXCAP:
        return dict(kernel="decrypt_bits_kernel", ucap=ucap, blocks=(total + 255) // 256,
                    partial_wave=total % 64 != 0)
    return dict(kernel="decrypt_kernel", ucap=ucap,
                blocks=(n + DEC_WAVES_PER_BLOCK - 1) // DEC_WAVES_PER_BLOCK,
                partial_block=n % DEC_WAVES_PER_BLOCK != 0)


def dec_wave_trace(cap):
    """decrypt_kernel on one bit of `cap` limbs: (lanes that enter the 4-way unrolled body, its
    rounds on lane 0, tail iterations on lane 0, on lane 63).  The body runs while
    `k + (kDecUnroll - 1) * kWave < cap` from k = lane in steps of 256, the tail while `k < cap`
    in steps of 64."""
    def walk(lane):
        k, rounds = lane, 0
        while k + (DEC_UNROLL - 1) * 64 < cap:
            k, rounds = k + DEC_UNROLL * 64, rounds + 1
        tail = 0
        while k < cap:
            k, tail = k + 64, tail + 1
        return rounds, tail
    entering = sum(1 for lane in range(64) if walk(lane)[0])
    return entering, walk(0)[0], walk(0)[1], walk(63)[1]


# ------------------------------------------------------------------ keys (loaded, never a pair)
@functools.lru_cache(maxsize=None)
def make_key(tau, pc, kind, seed=0):
    """(tau, pc) uint64 rows.  kind:
      wide     random limbs, some top limb above 1 (never a top1 key)
      top1     every top limb 0 or 1, both present (a mixed topcol)
      top0     every top limb 0 (topcol = 0)
      low<D>   random below degree D, exact degree D in row 0, the limbs above zero (rows padded
               beyond what they need)"""
    rng = np.random.default_rng([SEED, tau, pc, seed, sum(map(ord, kind))])
    rows = rng.integers(0, 2**64, size=(tau, pc), dtype=np.uint64)
    if kind == "wide":
        rows[0, pc - 1] |= np.uint64(1 << 63)
    elif kind == "top1":
        rows[:, pc - 1] = rng.integers(0, 2, size=tau, dtype=np.uint64)
        if tau > 1:
            rows[0, pc - 1], rows[tau - 1, pc - 1] = 1, 0
    elif kind == "top0":
        rows[:, pc - 1] = 0
    elif kind.startswith("low"):
        deg = int(kind[3:])
        w, b = deg // 64, deg % 64
        assert w < pc
        rows[:, w + 1:] = 0
        rows[:, w] &= np.uint64((1 << (b + 1)) - 1)
        rows[0, w] |= np.uint64(1 << b)
    else:
        raise KeyError(kind)
    rows.setflags(write=False)
    return rows


def key_maxdeg(rows):
    top = 0
    for r in rows:
        nz = np.nonzero(r)[0]
        if nz.size:
            top = max(top, 64 * int(nz[-1]) + int(r[nz[-1]]).bit_length() - 1)
    return top


# ------------------------------------------------------------------ encryption cases
@dataclass(frozen=True)
class EncCase:
    """tau, pc, kind: the key (make_key).  nbytes, n: the batch; n = None: derived from the CU
    count for `strides` grid strides (stride_n).  bound: None = 64 pc - 1 on every bit (capacity
    pc); an int = that bound on every bit; a tuple = the per-bit bounds.  off: bytes the device
    masks are offset from their 16-byte-aligned allocation.  kernel: the variant the case is
    named for; flags: the branch flags it is named for (a subset of enc_dispatch's output)."""
    tau: int
    pc: int
    kind: str
    kernel: str
    nbytes: int = 4
    n: int | None = 37
    bound: object = None
    off: int = 0
    flags: tuple = ()
    status: str = "ok"

    def rows(self):
        return make_key(self.tau, self.pc, self.kind)

    def bounds(self):
        nbits = 8 * self.nbytes
        if self.bound is None:
            return np.full(nbits, 64 * self.pc - 1, dtype=np.uint32)
        if np.isscalar(self.bound):
            return np.full(nbits, self.bound, dtype=np.uint32)
        b = np.asarray(self.bound, dtype=np.uint32)
        assert b.size == nbits
        return b

    def dispatch(self, cus=256, n=None):
        n = n if n is not None else (self.n if self.n is not None else stride_n(self, cus))
        return enc_dispatch(self.tau, self.pc, key_top1(self.rows()), self.bounds(), self.nbytes,
                            n, cus, masks_aligned=self.off % 16 == 0)


STRIDES = 3


def stride_n(case, cus):
    """The batch of a multi-stride case on a card of `cus` CUs: two whole grid strides, three more
    blocks and one wave, and 8 bits of the next wave (u8 values), so that a third stride runs in
    the first blocks and ends on a partly filled wave.  per_cu = 1 for these keys: blocks = cus."""
    assert case.nbytes == 1
    d = enc_dispatch(case.tau, case.pc, key_top1(case.rows()), case.bounds(), 1, 1 << 24, cus,
                     masks_aligned=case.off % 16 == 0)
    step = d["blocks"] * K_ENC_BLOCK
    return ((STRIDES - 1) * step + 3 * K_ENC_BLOCK + 64 + 8) // 8


def _tab(pc, gc, top1=False):
    return f"encrypt_table_kernel<{pc},{gc}{',TOP1' if top1 else ''}>"


def _zero_fill(pc, nbits=8):
    """per-bit capacities pc .. pc + 3, all above or at the key's: `for (l = PC; l < cap; ++l) dst[l] = 0`"""
    return tuple(64 * (pc + i % 4) - 1 for i in range(nbits))


U = (("uniform_cap", True),)
NU = (("uniform_cap", False),)

ENC_CASES = {
    # --- encrypt_table_kernel<PC,32,TOP1>: tau = 128, every top limb 0 or 1, aligned masks.
    # enc_lookup2<PL = PC - 1>: the one-pair table at PC = 2, 3, odd PL at even PC, the largest PC
    "top1_pc2": EncCase(128, 2, "top1", _tab(2, 32, True), flags=U + (("odd_lookup", True),)),
    "top1_pc3": EncCase(128, 3, "top1", _tab(3, 32, True), flags=U + (("odd_lookup", False),)),
    "top1_pc4": EncCase(128, 4, "top1", _tab(4, 32, True), flags=U + (("odd_lookup", True),)),
    "top1_pc9": EncCase(128, 9, "top1", _tab(9, 32, True), flags=U + (("odd_lookup", False),)),
    "top1_pc17": EncCase(128, 17, "top1", _tab(17, 32, True), flags=U + (("odd_lookup", False),)),
    "top1_topcol0_pc6": EncCase(128, 6, "top0", _tab(6, 32, True), flags=U),
    # --- encrypt_table_kernel<PC,32>: tau = 128, a top limb above 1
    "gc32_pc5": EncCase(128, 5, "wide", _tab(5, 32), flags=U + (("odd_lookup", True),)),
    "gc32_pc8": EncCase(128, 8, "wide", _tab(8, 32), flags=U + (("odd_lookup", False),)),
    # the same call with the masks 8 bytes off a 16-byte boundary: `<PC,0>` with mb = 16
    "gc0_pc5_tau128_masks_off8": EncCase(128, 5, "wide", _tab(5, 0), off=8,
                                         flags=U + (("mask_words", True), ("mb", 16))),
    "gc0_pc4_top1key_masks_off8": EncCase(128, 4, "top1", _tab(4, 0), off=8, flags=U),
    # --- encrypt_table_kernel<PC,0>: any tau.  mb & 3, G not a multiple of 8, rows past tau in
    # the last nibble group, PC = 1 and even PC
    "gc0_tau1_pc1": EncCase(1, 1, "wide", _tab(1, 0), flags=U + (("mask_words", False),)),
    "gc0_tau3_pc2": EncCase(3, 2, "wide", _tab(2, 0), flags=U + (("mask_words", False),)),
    "gc0_tau4_pc3": EncCase(4, 3, "wide", _tab(3, 0), flags=U + (("mask_words", False),)),
    "gc0_tau5_pc4": EncCase(5, 4, "wide", _tab(4, 0), flags=U + (("mask_words", False),)),
    "gc0_tau33_pc5": EncCase(33, 5, "wide", _tab(5, 0), flags=U + (("mb", 5),)),
    "gc0_tau40_pc6": EncCase(40, 6, "wide", _tab(6, 0), flags=U + (("mb", 5),)),
    "gc0_tau64_pc1": EncCase(64, 1, "wide", _tab(1, 0), flags=U + (("mask_words", True),)),
    "gc0_tau100_pc7_top1key": EncCase(100, 7, "top1", _tab(7, 0), flags=U + (("mb", 13),)),
    "gc0_tau130_pc3": EncCase(130, 3, "wide", _tab(3, 0), flags=U + (("mb", 17),)),
    # --- the lane-per-bit fallback, by table size (the table is not built) and its neighbour
    "gc0_tau1536_pc2_last_table": EncCase(1536, 2, "wide", _tab(2, 0), n=9, nbytes=1,
                                          flags=U + (("table", K_ENC_TABLE_BYTES),)),
    "fallback_table_tau1537_pc2": EncCase(1537, 2, "wide", "encrypt_kernel<2>", n=9, nbytes=1,
                                          flags=U + (("fallback", "table"), ("mask_words", False))),
    "fallback_table_tau2048_pc2": EncCase(2048, 2, "wide", "encrypt_kernel<2>", n=9, nbytes=1,
                                          flags=U + (("fallback", "table"), ("mask_words", True))),
    # --- the fallback with the table built but table + stage over 160 KiB, and its neighbour
    "fallback_lds_pc16_tau192": EncCase(192, 16, "wide", "encrypt_kernel<16>",
                                        flags=U + (("fallback", "lds"),)),
    "fallback_lds_pc17_tau168": EncCase(168, 17, "wide", "encrypt_kernel<17>",
                                        flags=U + (("fallback", "lds"),)),
    "gc0_pc17_tau160_last_lds": EncCase(160, 17, "wide", _tab(17, 0), flags=U),
    # --- output shapes: n * nbits < 64, a full wave + 8 bits, 3-byte values (lognbits = -1),
    # 16-byte values; on table variants and on the fallback
    "top1_pc5_n1_u8": EncCase(128, 5, "top1", _tab(5, 32, True), nbytes=1, n=1, flags=U),
    "top1_pc5_n9_u8": EncCase(128, 5, "top1", _tab(5, 32, True), nbytes=1, n=9, flags=U),
    "top1_pc5_n7_3byte": EncCase(128, 5, "top1", _tab(5, 32, True), nbytes=3, n=7,
                                 flags=U + (("lognbits", -1),)),
    "top1_pc5_n5_16byte": EncCase(128, 5, "top1", _tab(5, 32, True), nbytes=16, n=5,
                                  flags=U + (("lognbits", 7),)),
    "gc32_pc5_n7_3byte": EncCase(128, 5, "wide", _tab(5, 32), nbytes=3, n=7,
                                 flags=U + (("lognbits", -1),)),
    "gc0_tau40_pc6_n1_u8": EncCase(40, 6, "wide", _tab(6, 0), nbytes=1, n=1, flags=U),
    "gc0_tau40_pc6_n9_u8": EncCase(40, 6, "wide", _tab(6, 0), nbytes=1, n=9, flags=U),
    "gc0_tau40_pc6_n7_3byte": EncCase(40, 6, "wide", _tab(6, 0), nbytes=3, n=7,
                                      flags=U + (("lognbits", -1),)),
    "gc0_tau40_pc6_n5_16byte": EncCase(40, 6, "wide", _tab(6, 0), nbytes=16, n=5, flags=U),
    "fallback_lds_n1_u8": EncCase(192, 16, "wide", "encrypt_kernel<16>", nbytes=1, n=1, flags=U),
    "fallback_lds_n9_u8": EncCase(192, 16, "wide", "encrypt_kernel<16>", nbytes=1, n=9, flags=U),
    "fallback_lds_n7_3byte": EncCase(192, 16, "wide", "encrypt_kernel<16>", nbytes=3, n=7,
                                     flags=U + (("lognbits", -1),)),
    "fallback_lds_n5_16byte": EncCase(192, 16, "wide", "encrypt_kernel<16>", nbytes=16, n=5, flags=U),
    # --- non-uniform output bounds: per-bit capacities above PC (zero fill) ...
    "top1_pc3_zero_fill": EncCase(128, 3, "top1", _tab(3, 32, True), nbytes=1, n=37,
                                  bound=_zero_fill(3), flags=NU),
    "gc32_pc5_zero_fill": EncCase(128, 5, "wide", _tab(5, 32), nbytes=1, n=37,
                                  bound=_zero_fill(5), flags=NU),
    "gc0_tau33_pc5_zero_fill": EncCase(33, 5, "wide", _tab(5, 0), nbytes=1, n=37,
                                       bound=_zero_fill(5), flags=NU),
    "fallback_lds_zero_fill": EncCase(192, 16, "wide", "encrypt_kernel<16>", nbytes=1, n=37,
                                      bound=_zero_fill(16), flags=NU),
    # ... and rows padded beyond the output's capacity (the dropped limbs are zero: no flag)
    "top1_pc5_rows_padded_b100": EncCase(128, 5, "low100", _tab(5, 32, True), nbytes=1, n=37,
                                         bound=100, flags=NU),
    "gc0_tau40_pc5_rows_padded_b100": EncCase(40, 5, "low100", _tab(5, 0), nbytes=1, n=37,
                                              bound=100, flags=NU),
    "fallback_table_rows_padded_b40": EncCase(1537, 2, "low40", "encrypt_kernel<2>", nbytes=1,
                                              n=9, bound=40, flags=NU + (("fallback", "table"),)),
    # --- more than one grid stride (per_cu = 1; n from the CU count, stride_n)
    "gc0_tau256_pc9_strides": EncCase(256, 9, "wide", _tab(9, 0), nbytes=1, n=None,
                                      flags=U + (("per_cu", 1), ("strides", STRIDES),
                                                 ("partial_wave", True))),
    "gc32_pc13_strides": EncCase(128, 13, "wide", _tab(13, 32), nbytes=1, n=None,
                                 flags=U + (("per_cu", 1), ("strides", STRIDES),
                                            ("partial_wave", True))),
    "top1_pc17_strides": EncCase(128, 17, "top1", _tab(17, 32, True), nbytes=1, n=None,
                                 flags=U + (("per_cu", 1), ("strides", STRIDES),
                                            ("partial_wave", True))),
    # --- refusals
    "unsupported_pc18": EncCase(8, 18, "wide", "unsupported", nbytes=1, n=9, status="unsupported"),
    "invalid_bound_below_maxdeg": EncCase(40, 6, "wide", _tab(6, 0), nbytes=1, n=9, bound=382,
                                          status="invalid"),
}

# every variant the tier must name: a case name containing the key and a restated kernel with the
# prefix (test_cipher_paths.py::test_every_variant_has_a_case)
ENC_VARIANTS = {
    "top1_": ("encrypt_table_kernel<", ",32,TOP1>"),
    "gc32_": ("encrypt_table_kernel<", ",32>"),
    "gc0_": ("encrypt_table_kernel<", ",0>"),
    "fallback_table_": ("encrypt_kernel<", ">"),
    "fallback_lds_": ("encrypt_kernel<", ">"),
}


def enc_inputs(name, n):
    """(data (n, nbytes) uint8, masks (n, nbits, mb) uint8) of a case, seeded by its name."""
    c = ENC_CASES[name]
    rng = np.random.default_rng([SEED, n] + [ord(ch) for ch in name])
    data = rng.integers(0, 256, size=(n, c.nbytes), dtype=np.uint8)
    masks = rng.integers(0, 256, size=(n, 8 * c.nbytes, (c.tau + 7) // 8), dtype=np.uint8)
    return data, masks


# ------------------------------------------------------------------ mask draw cases
DRAW_SEED = 2718
DRAW_LENGTHS = (0, 1, 63, 64, 65, 1000, 16383, 16384, 16385, (1 << 20) + 5)
DRAW_MISALIGN = (1, 8)       # destination offsets of the 16385-byte draws
DRAW_MISALIGN_LEN = 16385
ENGINE_MASKS = dict(tau=33, pc=2, kind="wide", nbytes=1, n=(9, 9, 37))  # mb = 5: 360, 360, 1480 bytes


def draw_windows(length):
    """[lo, hi) byte windows of a draw to compare: everything up to 32 KiB + 64; for a longer draw
    the first block, the two 64-byte ChaCha20 blocks around every 16384-byte edge (where
    rand_fill_kernel's block of 256 threads ends), the last full block and the partial one."""
    if length <= 2 * RAND_BLOCK_BYTES + 64:
        return [(0, length)]
    w = [(0, 64)]
    for edge in range(RAND_BLOCK_BYTES, length, RAND_BLOCK_BYTES):
        w.append((edge - 64, min(edge + 64, length)))
    last = length // 64 * 64
    w.append((max(last - 64, 0), length))
    return w
