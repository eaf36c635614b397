"""The MFMA carry chain's bit loop (adder_mfma.hip) on the paths its address bookkeeping takes:
ring wraps and all four ring phases, a chain that restarts after tiles have run, odd and even
window depths with a short carry (the tiles' degree tracking), and each chunk-count instance.

Every case is bit-exact against the CPU oracle (degrees and limbs) plus decrypt parity; there is
no tolerance.  Each case also replays the chain on the oracle's input polynomials with the model's
integers and asserts that the inputs reach the path the case is named for, so a case that no
longer reaches its path fails instead of passing idly.  `reference(case)` needs no GPU.
"""
import functools

import numpy as np
import pytest

from helpers import as_bytes, assert_batches_equal, bit_ints, fresh_bound, keys, masks, plain

pytestmark = pytest.mark.gpu

SEED = 31


@pytest.fixture(scope="module")
def H():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import homomorph
    homomorph.lib()  # loud failure if the engine is not built
    return homomorph


# ------------------------------------------------------------------ inputs
def _even_odd(m, odd):
    """Masks with the wanted popcount parity (bit 0 of byte 0 flipped where needed): an odd subset
    of public-key rows has degree d + dp exactly, an even one a lower degree (the tops cancel)."""
    par = np.unpackbits(m, axis=-1).sum(axis=-1) & 1
    m = m.copy()
    m[..., 0] ^= (par != int(odd)).astype(np.uint8)
    return m


def _case(name):
    """dict(params, dtype, n, a, b, ma, mb, ba, bb): plaintexts, subset masks, input bounds."""
    if name in ("wrap_u16", "wrap_u8", "nc7_u16", "nc25_u8"):
        params, dtype, n = {"wrap_u16": ((128, 128, 1, 128), np.uint16, 5),
                            "wrap_u8": ((128, 128, 1, 128), np.uint8, 3),
                            "nc7_u16": ((64, 64, 1, 64), np.uint16, 6),
                            "nc25_u8": ((256, 256, 1, 256), np.uint8, 3)}[name]
        nbits = 8 * np.dtype(dtype).itemsize
        a, b = plain(n, dtype, 41), plain(n, dtype, 42)
        ma, mb = masks(n, nbits, params[3], 43), masks(n, nbits, params[3], 44)
        ba = bb = fresh_bound(params[0], params[1], nbits)
    elif name == "restart_u16":
        # bits 6 and 11 of both operands: plaintext 0 under an all-zero mask, i.e. the null
        # polynomial, so x_i = P_i = ab_i = 0 there and the carry goes null after tiles have run
        params, dtype, n, nbits = (128, 128, 1, 128), np.uint16, 4, 16
        keep = np.uint16(~((1 << 6) | (1 << 11)) & 0xFFFF)
        a, b = plain(n, dtype, 51) & keep, plain(n, dtype, 52) & keep
        ma, mb = masks(n, nbits, 128, 53), masks(n, nbits, 128, 54)
        for m in (ma, mb):
            m[:, 6, :] = 0
            m[:, 11, :] = 0
        ba = bb = fresh_bound(128, 128, nbits)
    elif name == "short_carry_u8":
        # skewed capacities; per bit (LSB first), with d + dp = 128:
        #   1, 5  a_i an even subset of the key's rows (their tops cancel: a lower degree)
        #   2, 6  both odd subsets: P_i at its full degree, 12 words (even)
        #   3     a_i = b_i = 1 (zero masks): x = P = 0, ab = 1, so carry_4 = 1
        #   4     the same subset in both, plaintext bits 1 and 0: x_i = 1, so deg P_i + deg carry
        #         = deg ab_i: a short carry, the tiles track the degree; P_i = 1 + ab_i has 9 words
        #         (odd); carry_5 = 1 again
        params, dtype, n, nbits = (64, 64, 1, 64), np.uint8, 4, 8
        rng = np.random.default_rng(61)
        ba = rng.integers(128, 257, size=nbits).astype(np.uint32)
        bb = rng.integers(128, 257, size=nbits).astype(np.uint32)
        a = (plain(n, dtype, 62) & np.uint8(0b11100111)) | np.uint8(0b00011000)
        b = (plain(n, dtype, 63) & np.uint8(0b11100111)) | np.uint8(0b00001000)
        ma, mb = _even_odd(masks(n, nbits, 64, 64), True), _even_odd(masks(n, nbits, 64, 65), True)
        for i in (1, 5):
            ma[:, i, :] = _even_odd(ma[:, i, :], False)
        ma[:, 3, :] = 0
        mb[:, 3, :] = 0
        mb[:, 4, :] = ma[:, 4, :]
    else:
        raise KeyError(name)
    return dict(params=params, dtype=dtype, n=n, a=a, b=b, ma=ma, mb=mb,
                ba=np.asarray(ba, dtype=np.uint32), bb=np.asarray(bb, dtype=np.uint32))


# ------------------------------------------------------------------ CPU side
def _words(p):
    return (p.bit_length() + 31) // 32


def chain_trace(abits, bbits, model):
    """The kernel's per-bit quantities for one value, from its input polynomials: words of P_i
    (np), of ab_i and of carry_i (nc), the tiles bit i runs (0: the copy-ab branch) and whether
    they track the degree (deg P_i + deg carry_i <= deg ab_i)."""
    rows, c = [], 0
    for i in range(len(abits) - 1):
        x = abits[i] ^ bbits[i]
        ab = model.clmul_fast(abits[i], bbits[i])
        p = model.clmul_fast(x, ab ^ 1)
        npw, nab, nc = _words(p), _words(ab), _words(c)
        tiles = 0 if npw == 0 or nc == 0 else (max(nc + npw, nab) + 31) // 32
        track = tiles > 0 and (p.bit_length() - 1) + (c.bit_length() - 1) <= ab.bit_length() - 1
        rows.append(dict(i=i, np=npw, nab=nab, nc=nc, tiles=tiles, track=track))
        c = ab ^ model.clmul_fast(p, c)
    return rows


@functools.lru_cache(maxsize=None)
def reference(name):
    """Inputs, the oracle's add and the chain traces of one case (computed once, shared)."""
    import homomorph as H
    from oracle import gf2_model as model
    from oracle import oracle_py as oracle
    oracle.build()
    c = _case(name)
    nbits = 8 * np.dtype(c["dtype"]).itemsize
    sk, pk, _ = keys(*c["params"], SEED)
    la, da = oracle.encrypt_batch(pk, as_bytes(c["a"]), c["ma"], c["ba"])
    lb, db = oracle.encrypt_batch(pk, as_bytes(c["b"]), c["mb"], c["bb"])
    ob = H.add_out_bounds(c["ba"], c["bb"])
    rl, rd = oracle.add_batch(la, da, c["ba"], lb, db, c["bb"], nbits, c["n"], ob)
    rdec = oracle.decrypt_batch(sk, rl, rd, ob, nbits, c["n"]).view(c["dtype"]).reshape(-1)
    traces = [chain_trace(bit_ints(la, da, c["ba"], e), bit_ints(lb, db, c["bb"], e), model)
              for e in range(c["n"])]
    for v in (rl, rd, rdec):
        v.setflags(write=False)
    return dict(case=c, ob=ob, rl=rl, rd=rd, rdec=rdec, traces=traces)


def check_paths(name, traces):
    """The path each case is named for, asserted from the oracle's polynomials."""
    rows = [r for t in traces for r in t]
    ran = [r for r in rows if r["tiles"] > 0]
    if name in ("wrap_u16", "wrap_u8"):
        # the carry passes the ring's 128 words (u16: nearly three times), and the bits' tile
        # counts cover every ring phase
        assert max(r["nc"] for r in rows) > (320 if name == "wrap_u16" else 128)
        # (carry_i has about 17 + 24 (i - 1) words at d + dp = 256: 2 .. 11 tiles over a u16's
        # bits, 2 .. 5 over a u8's)
        want = set(range(2, 12)) if name == "wrap_u16" else set(range(2, 6))
        assert want <= {r["tiles"] for r in ran}, sorted({r["tiles"] for r in ran})
    elif name == "restart_u16":
        for t in traces:
            for i in (6, 11):
                # tiles ran on the bit before; bit i itself takes the copy branch with a live
                # carry (np = 0, nc > 0), and the next bit starts from a null carry
                assert t[i - 1]["tiles"] > 0 and t[i]["np"] == 0 and t[i]["nc"] > 0
                assert t[i + 1]["nc"] == 0 and t[i + 1]["tiles"] == 0
            assert t[i + 2]["tiles"] > 0  # ... and the chain runs again
    elif name == "short_carry_u8":
        for t in traces:
            assert {r["np"] & 1 for r in t if r["tiles"] > 0} == {0, 1}, t
            assert t[3]["np"] == 0 and t[4]["nc"] == 1  # carry_4 = 1
            assert t[4]["tiles"] > 0 and t[4]["track"] and t[5]["nc"] == 1
            assert t[5]["tiles"] > 0 and not t[5]["track"] and t[5]["np"] % 2 == 0
    elif name == "nc7_u16":
        assert 8 <= max(r["np"] for r in ran) <= 13 and max(r["tiles"] for r in ran) >= 5
    elif name == "nc25_u8":
        assert 26 <= max(r["np"] for r in ran) <= 49 and max(r["tiles"] for r in ran) >= 5


# ------------------------------------------------------------------ GPU side
def _run(H, name, chain):
    ref = reference(name)
    c = ref["case"]
    check_paths(name, ref["traces"])
    ctx = H.Context(H.Parameters(*c["params"]))
    ctx.seed_rng(SEED)
    ctx.generate_secret_key()
    ctx.generate_public_key()
    ctx.set_add_options(chain)
    ca = ctx.encrypt(c["a"], masks=c["ma"], bound=c["ba"])
    cb = ctx.encrypt(c["b"], masks=c["mb"], bound=c["bb"])
    cs = ctx.apply2(H.HomomorphicAddition, ca, cb)
    dec = ctx.decrypt(cs)
    ctx.synchronize()
    assert np.array_equal(cs.bound, ref["ob"])
    gl, gd = cs.to_host()
    assert_batches_equal(gl, gd, ref["rl"], ref["rd"], ref["ob"], c["n"], f"{name}/{chain}")
    assert np.array_equal(dec, ref["rdec"])


@pytest.mark.parametrize("chain", ["mfma", "valu"])
@pytest.mark.parametrize("name", ["wrap_u16", "wrap_u8"])
def test_ring_wrap_and_tile_phases(H, name, chain):
    """A ragged last block (n = 5 and 3 at 4 waves per block), carries past the ring's 128 words,
    2 .. 11 tiles per bit: the MFMA chain and the VALU chain both equal the oracle."""
    _run(H, name, chain)


def test_chain_restart_after_tiles(H):
    """Null P_i and ab_i on two middle bits: the carry goes null after tiles have run (the
    tw >= 0 -> copy ab -> tw = -1 path) and the chain restarts."""
    _run(H, "restart_u16", "mfma")


def test_odd_even_depth_short_carry(H):
    """Window depths D = np of both parities under skewed capacities, and a short carry (carry =
    1 under x_i = 1) whose tiles track the degree."""
    _run(H, "short_carry_u8", "mfma")


@pytest.mark.parametrize("name", ["nc7_u16", "nc25_u8"])
def test_each_instance(H, name):
    """The 7-chunk (d + dp = 128) and 25-chunk (d + dp = 512) instances of the chain."""
    _run(H, name, "mfma")
