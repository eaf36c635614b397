"""CPU: the case table of the cipher-paths tier (tests/cipher_paths.py) held against the restated
dispatch of csrc/cipher.hip, before test_gpu_cipher_paths.py runs the engine on it.

Every encryption case lands on the kernel variant and the branch flags it is named for; the
multi-stride cases at the CU counts of three cards; the table-size and LDS-size edges as last fits
/ first does not; the keys are of the top-limb class their cases need.  The synthetic decryption
operands reach the top coefficient of every capacity-defining bound, on the kernel and branch of
their names, and the model's decryption equals the C oracle's on them.
"""
import re

import numpy as np
import pytest

import cipher_paths as cp
import synth
from helpers import seeded_random_bytes


# ------------------------------------------------------------------ encryption
@pytest.mark.parametrize("name", list(cp.ENC_CASES))
def test_enc_case_reaches_its_path(name):
    c = cp.ENC_CASES[name]
    d = c.dispatch(cus=256)
    assert d["kernel"] == c.kernel, (name, d)
    for k, v in c.flags:
        assert d[k] == v, (name, k, d)
    if c.status == "unsupported":
        return
    # the name says which variant it is
    key = next(k for k in cp.ENC_VARIANTS if name.startswith(k)) if c.status == "ok" else None
    if key:
        pre, post = cp.ENC_VARIANTS[key]
        assert d["kernel"].startswith(pre) and d["kernel"].endswith(post)
        if key.startswith("fallback_"):
            assert d["fallback"] == key.split("_")[1]
    rows, bound = c.rows(), c.bounds()
    assert rows.shape == (c.tau, c.pc)
    if c.status == "invalid":  # `if (out->bound[i] < c->pk_maxdeg) return HM_ERR_INVALID_ARGUMENT`
        assert int(bound.min()) == cp.key_maxdeg(rows) - 1
        return
    assert int(bound.min()) >= cp.key_maxdeg(rows)
    # HM_ERR_CAPACITY only where a nonzero limb is dropped: never here
    assert cp.key_maxdeg(rows) // 64 + 1 <= int(cp.caps(bound).min())
    # the mask buffer of a misaligned case keeps 4-byte alignment (word reads at mb & 3 == 0)
    assert c.off % 4 == 0


def test_every_variant_has_a_case():
    """The three table forms with and without TOP1, the fallback by table size and by LDS size."""
    for key, (pre, post) in cp.ENC_VARIANTS.items():
        hits = [n for n, c in cp.ENC_CASES.items() if n.startswith(key) and c.status == "ok"]
        assert hits, key
        for n in hits:
            k = cp.ENC_CASES[n].dispatch()["kernel"]
            assert k.startswith(pre) and k.endswith(post), (n, k)
    kernels = {c.dispatch()["kernel"] for c in cp.ENC_CASES.values()}
    assert {cp._tab(pc, 32, True) for pc in (2, 3, 4, 5, 6, 9, 17)} <= kernels
    assert {cp._tab(5, 32), cp._tab(8, 32), cp._tab(13, 32)} <= kernels
    assert {cp._tab(pc, 0) for pc in (1, 2, 3, 4, 5, 6, 7, 9, 17)} <= kernels
    assert {"encrypt_kernel<2>", "encrypt_kernel<16>", "encrypt_kernel<17>"} <= kernels
    # every output shape on a table variant and on the fallback
    for shape in ("n1_u8", "n9_u8", "n7_3byte", "n5_16byte", "zero_fill", "rows_padded"):
        names = [n for n in cp.ENC_CASES if shape in n]
        assert any(n.startswith("fallback") for n in names) and any(
            n.startswith(("top1", "gc32", "gc0")) for n in names), shape
    # each flag value of the in-kernel branches appears with each table form that has the branch
    # (uniform_cap or per-bit stores, shift or divide by nbits)
    seen = set()
    for c in cp.ENC_CASES.values():
        if c.status == "ok":
            d = c.dispatch()
            seen.add((re.sub(r"<\d+", "<PC", d["kernel"]), d["uniform_cap"], d["lognbits"] >= 0))
    for form in ("encrypt_table_kernel<PC,32,TOP1>", "encrypt_table_kernel<PC,32>",
                 "encrypt_table_kernel<PC,0>", "encrypt_kernel<PC>"):
        assert {(form, True, True), (form, False, True), (form, True, False)} <= seen, form


@pytest.mark.parametrize("name", [n for n, c in cp.ENC_CASES.items() if c.n is None])
@pytest.mark.parametrize("cus", [256, 304, 64])
def test_stride_cases_on_three_cards(name, cus):
    """`blocks = min(want, cus * per_cu)` with per_cu = 1: the batch derived from the CU count
    takes three grid strides and ends on a partly filled wave, whatever the card."""
    c = cp.ENC_CASES[name]
    n = cp.stride_n(c, cus)
    d = c.dispatch(cus, n)
    assert d["kernel"] == c.kernel and d["per_cu"] == 1 and d["blocks"] == cus
    assert d["strides"] == cp.STRIDES >= 3 and d["partial_wave"] and d["uniform_cap"]
    total, step = 8 * n, cus * cp.K_ENC_BLOCK
    assert 2 * step < total < 3 * step and total % 64 == 8
    assert (total - 2 * step) // cp.K_ENC_BLOCK == 3  # three whole blocks take a third pass
    # one value fewer per stride would not: the count is not padded
    assert c.dispatch(cus, 2 * step // 8)["strides"] == 2


def test_table_and_lds_edges():
    """The hand-derived edges of launch_enc_pc, as last fits / first does not."""
    b = lambda pc: np.full(8, 64 * pc - 1, dtype=np.uint32)  # noqa: E731
    k = lambda tau, pc: cp.enc_dispatch(tau, pc, False, b(pc), 1, 9, 256)  # noqa: E731
    # table size: tab = ceil(tau / 4) * ceil(PC / 2) * 256 <= 96 KiB
    assert cp.table_bytes(1536, 2) == cp.K_ENC_TABLE_BYTES and cp.table_bytes(1537, 2) > cp.K_ENC_TABLE_BYTES
    assert k(1536, 2)["kernel"] == "encrypt_table_kernel<2,0>"
    assert k(1537, 2)["kernel"] == "encrypt_kernel<2>" and k(1537, 2)["fallback"] == "table"
    assert k(2048, 2)["fallback"] == "table"
    assert cp.table_bytes(256, 9) == 80 * 1024  # engine.h: "tau = 256 at d + dp = 512: 80 KB"
    # LDS size: the table fits, table + stage + bounds does not
    for pc, fits, not_ in ((16, 188, 189), (17, 160, 161)):
        assert cp.table_bytes(not_ + 3, pc) <= cp.K_ENC_TABLE_BYTES
        assert cp.enc_lds(fits, pc) <= cp.LDS_BYTES < cp.enc_lds(not_, pc)
        assert k(fits, pc)["kernel"] == f"encrypt_table_kernel<{pc},0>"
        assert k(not_, pc)["kernel"] == f"encrypt_kernel<{pc}>" and k(not_, pc)["fallback"] == "lds"
    assert k(192, 16)["fallback"] == "lds" and k(168, 17)["fallback"] == "lds"
    assert cp.enc_lds(160, 17) == 162816 and cp.enc_lds(168, 17) == 167424
    # per_cu = clamp(160 KiB / lds, 1, 4): the bench's key (tau 128, PC 5, TOP1) gets 4
    top = cp.enc_dispatch(128, 5, True, b(5), 1, 1 << 22, 256)
    assert top["kernel"] == "encrypt_table_kernel<5,32,TOP1>" and top["per_cu"] == 4
    assert top["blocks"] == 1024 and top["strides"] == 64
    assert cp.enc_dispatch(128, 18, False, b(18), 1, 9, 256) == dict(kernel="unsupported")


def test_keys_are_of_their_class():
    """TOP1 keys have every top limb in {0, 1} (a mixed topcol, or all zero), the others do not."""
    for name, c in cp.ENC_CASES.items():
        rows = c.rows()
        top = rows[:, c.pc - 1]
        if c.kind == "top1":
            assert set(top.tolist()) == {0, 1} and cp.key_top1(rows) == (c.tau <= 128), name
            assert cp.key_maxdeg(rows) == 64 * (c.pc - 1)
        elif c.kind == "top0":
            assert not top.any() and cp.key_top1(rows), name
        elif c.kind == "wide":
            assert int(top.max()) > 1 and not cp.key_top1(rows), name
            assert cp.key_maxdeg(rows) == 64 * c.pc - 1
        else:
            deg = int(c.kind[3:])
            assert cp.key_maxdeg(rows) == deg and not rows[:, deg // 64 + 1:].any(), name
        if "TOP1" in c.kernel:
            assert cp.key_top1(rows) and c.tau == 128 and c.off == 0, name
    assert cp.make_key(128, 5, "top1") is cp.make_key(128, 5, "top1")  # one key per shape


def test_enc_reference_runs_on_a_loaded_key(oracle, model):
    """The oracle's encrypt_batch on loaded rows of a shape no keygen makes, against the model's
    cipher_bit: per-bit capacities above the rows' (zero fill) and a 5-byte mask."""
    name = "gc0_tau33_pc5_zero_fill"
    c = cp.ENC_CASES[name]
    data, masks = cp.enc_inputs(name, 3)
    limbs, deg = oracle.encrypt_batch(c.rows(), data, masks, c.bounds())
    pk = [model.limbs_to_int(r) for r in c.rows()]
    cap = cp.caps(c.bounds())
    want, wdeg = [], []
    for e in range(3):
        for k in range(8):
            p = model.cipher_bit((int(data[e, 0]) >> k) & 1, pk, bytes(masks[e, k]))
            want += model.int_to_limbs(p, int(cap[k]))
            wdeg.append(model.degree(p))
    assert limbs.tolist() == want and deg.tolist() == wdeg


# ------------------------------------------------------------------ decryption
@pytest.mark.parametrize("name", list(synth.DEC_PATH_CASES))
def test_dec_case_reaches_its_path(oracle, name):
    c = synth.inputs("dec", name)
    la, da, _, _ = synth.packed("dec", name)
    sk, _, _ = oracle.keygen(*synth.DEC_PARAMS, synth.SEED)
    want = oracle.decrypt_batch(sk, la, da, c["ba"], c["nbits"], c["n"])
    assert np.array_equal(synth.dec_reference(name), want)
    if want.size >= 8:
        assert 0 < int(np.unpackbits(want).sum()) < want.size * 8
    d = synth.check_dec_path(name)
    assert d["kernel"] == ("decrypt_bits_kernel" if name.startswith("bits_") else "decrypt_kernel")


def test_existing_dec_cases_in_the_restatement():
    """The four full-bounds decryption cases, through dec_dispatch as well."""
    want = {"b511_ucap": ("decrypt_bits_kernel", 8), "b512": ("decrypt_bits_kernel", 0),
            "per_bit": ("decrypt_kernel", 0), "per_bit_cap32": ("decrypt_bits_kernel", 0)}
    for name, bound in synth.DEC_CASES.items():
        d = cp.dec_dispatch(bound, synth.DEC_N)
        assert (d["kernel"], d["ucap"]) == want[name]
        assert d["ucap"] == synth.check_dec_path(name)["ucap"]


# ------------------------------------------------------------------ mask draw
def test_draw_windows_cover_the_edges():
    for n in cp.DRAW_LENGTHS:
        w = cp.draw_windows(n)
        assert all(0 <= lo <= hi <= n for lo, hi in w)
        covered = np.zeros(n + 1, dtype=bool)
        for lo, hi in w:
            covered[lo:hi] = True
        if n <= 2 * cp.RAND_BLOCK_BYTES + 64:
            assert covered[:n].all()
            continue
        assert covered[:64].all() and covered[n - 69:n].all()  # first block; last full + partial
        for edge in range(cp.RAND_BLOCK_BYTES, n, cp.RAND_BLOCK_BYTES):
            assert covered[edge - 64:min(edge + 64, n)].all()
    # the lengths sit on the kernel's edges: a ChaCha20 block, a block of 256 threads
    assert {63, 64, 65, 16383, 16384, 16385} <= set(cp.DRAW_LENGTHS)
    assert cp.DRAW_LENGTHS[-1] % 64 == 5 and cp.DRAW_MISALIGN_LEN > cp.RAND_BLOCK_BYTES
    e = cp.ENGINE_MASKS
    mb = (e["tau"] + 7) // 8
    assert mb % 4 and all((n * 8 * e["nbytes"] * mb) % 64 for n in e["n"]) and e["n"][2] > e["n"][1]
    # the reference generator indexes draws and bytes as the tests use it
    a = seeded_random_bytes(cp.DRAW_SEED, 3, 200)
    assert np.array_equal(a[70:150], seeded_random_bytes(cp.DRAW_SEED, 3, 80, start=70))
    assert not np.array_equal(a, seeded_random_bytes(cp.DRAW_SEED, 4, 200))
