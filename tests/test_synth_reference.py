"""CPU: the references of the full-bounds tier (tests/synth.py), pinned before the GPU meets them.

For every case of test_gpu_full_bounds.py: the model's result equals the C oracle's on the same
synthetic operands (borrow_model has no second implementation: its ring identities and residues
are checked instead), every output degree is within the engine's static output bounds
(H.*_out_bounds, which the Python restatements of synth.py must equal), and the case's path
assertion holds on the model's integers, so a case that stops reaching its path fails here.

The families of select, min / max, lookup, shift, the bit counts and the array circuits have no C
restatement: each model is pinned by a second evaluation order (or in the residue ring) instead,
and their plans come from the stand-alone plan drivers of tests/sanitize/.
"""
import numpy as np
import pytest

import borrow_model as bm
import synth
from helpers import assert_batches_equal, residue_modulus


@pytest.fixture(scope="module")
def H():
    import homomorph
    homomorph.lib()  # host-only entry points: no GPU needed
    return homomorph


def within(vals, ob):
    for v in vals:
        for p, b in zip(v, ob):
            assert p.bit_length() - 1 <= int(b)


# ------------------------------------------------------------------ the generator itself
def test_schedule_and_kinds():
    """Every kind at every bit position, exact degrees, nothing above the bound."""
    for bound in (0, 1, 31, 40, 63, 64, 255, 700, 1023, 8223):
        b8 = synth.uniform(8, bound)
        vals = synth.operands(b8, 12, 5)
        within(vals, b8)
        for e in range(8):
            for i in range(8):
                k, p = synth.kind_of(e, i), vals[e][i]
                assert k == synth.KINDS[(e + i) % 8]
                if k in ("FULL", "MONO", "ONES", "SPARSE"):
                    assert p.bit_length() - 1 == bound
                if k == "MONO":
                    assert p == 1 << bound
                if k == "ONES":
                    assert p == (1 << (bound + 1)) - 1
                if k == "NULL":
                    assert p == 0
                if k == "UNIT":
                    assert p == 1
                if k == "EDGE":
                    assert p.bit_length() - 1 in synth.edge_degrees(bound)
                if k == "SPARSE" and bound >= 2:
                    assert 1 <= p.bit_count() <= 3
                if k == "LOW" and bound >= 2:
                    assert p.bit_length() - 1 < bound // 2
        for i in range(8):
            assert {synth.kind_of(e, i) for e in range(8)} == set(synth.KINDS)
            assert {synth.kind_of(e, i, 3) for e in range(8)} == set(synth.KINDS)
    assert synth.edge_degrees(700) == [31, 32, 33, 63, 64, 65, 639, 640, 699]
    assert synth.operands(synth.uniform(8, 300), 10, 7) == synth.operands(synth.uniform(8, 300), 10, 7)
    A, B = synth.full_pair(synth.uniform(8, 266), synth.uniform(8, 266), 4, 1)
    assert all(a.bit_length() - 1 == 266 for v in A for a in v)
    assert all(b.bit_length() - 1 == 265 for v in B for b in v[1:])
    assert [v[0].bit_length() - 1 for v in B] == [265, 266, 265, 266]


# ------------------------------------------------------------------ gates
@pytest.mark.parametrize("name", list(synth.GATE_CASES))
def test_gate_reference(H, oracle, name):
    c = synth.inputs("gate", name)
    la, da, lb, db = synth.packed("gate", name)
    assert 8 <= c["n"] <= 16
    for op in synth.GATE_OPS:
        ob, vals, rl, rd = synth.gate_reference(name, op)
        opcls = {"and": H.HomomorphicAndGate, "or": H.HomomorphicOrGate,
                 "xor": H.HomomorphicXorGate, "not": H.HomomorphicNotGate}[op]
        assert np.array_equal(ob, H.gate_out_bounds(opcls, c["ba"], None if op == "not" else c["bb"]))
        within(vals, ob)
        ol, od = oracle.gate_batch(op, la, da, c["ba"], lb, db, c["bb"], 8, c["n"], ob)
        assert_batches_equal(rl, rd, ol, od, ob, c["n"], f"{name} {op}")
    synth.check_gate_path(name)


# ------------------------------------------------------------------ subtraction, comparisons
@pytest.mark.parametrize("name", list(synth.BORROW_CASES))
def test_borrow_reference(H, name):
    c = synth.inputs("borrow", name)
    assert 8 <= c["n"] <= 16
    g = residue_modulus(17)
    mul = synth.model.residue_mul(g)
    RA = [[synth.model.residue_int(p, g) for p in v] for v in c["A"]]  # once: the slow part
    RB = [[synth.model.residue_int(p, g) for p in v] for v in c["B"]]
    ob, vals, _, _ = synth.borrow_reference(name, "sub")
    assert np.array_equal(ob, H.sub_out_bounds(c["ba"], c["bb"]))
    within(vals, ob)
    for a, b, ra, rb, out in zip(c["A"], c["B"], RA, RB, vals):
        w = bm.borrows(a, b, last=False)
        assert [o ^ x ^ y for o, x, y in zip(out, a, b)] == w  # sub_i + a_i + b_i = w_i
        # the borrow recurrence in the residue ring (a ring homomorphism)
        rw = 0
        for i in range(len(a)):
            assert synth.model.residue_int(w[i], g) == rw
            rw = mul(ra[i], rb[i]) ^ rb[i] ^ mul(ra[i] ^ rb[i] ^ 1, rw)
    for signed in (False, True):
        for op in bm.COMPARISONS:
            ob, vals, _, _ = synth.borrow_reference(name, op, signed)
            assert np.array_equal(ob, H.compare_out_bounds(_cmp(H, op), c["ba"], c["bb"]))
            within(vals, ob)
            for ra, rb, out in zip(RA, RB, vals):
                if op in ("eq", "ne"):
                    want = 1
                    for x, y in zip(ra, rb):
                        want = mul(x ^ y ^ 1, want)
                    want ^= op == "ne"
                else:
                    if op in ("gt", "le"):
                        ra, rb = rb, ra
                    want, n = 0, len(ra)
                    for i in range(n):
                        gen = ra[i] if signed and i == n - 1 else rb[i]
                        want = mul(ra[i], rb[i]) ^ gen ^ mul(ra[i] ^ rb[i] ^ 1, want)
                    want ^= op in ("ge", "le")
                assert synth.model.residue_int(out[0], g) == want, (op, signed)
                assert out[1:] == [0] * 7
    synth.check_borrow_path(name)


def _cmp(H, op):
    return {"eq": H.HomomorphicEqual, "ne": H.HomomorphicNotEqual, "lt": H.HomomorphicLessThan,
            "le": H.HomomorphicLessEqual, "gt": H.HomomorphicGreaterThan,
            "ge": H.HomomorphicGreaterEqual}[op]


# ------------------------------------------------------------------ addition
@pytest.mark.parametrize("name", list(synth.ADD_CASES))
def test_add_reference(H, oracle, name):
    c = synth.inputs("add", name)
    la, da, lb, db = synth.packed("add", name)
    ob, vals, rl, rd = synth.add_reference(name)
    assert np.array_equal(ob, H.add_out_bounds(c["ba"], c["bb"]))
    within(vals, ob)
    ol, od = oracle.add_batch(la, da, c["ba"], lb, db, c["bb"], c["nbits"], c["n"], ob)
    assert_batches_equal(rl, rd, ol, od, ob, c["n"], name)
    synth.check_add_path(name)


# ------------------------------------------------------------------ multiplication
@pytest.mark.parametrize("name", list(synth.MUL_CASES))
def test_mul_reference(H, oracle, name):
    from helpers import low_bits
    c = synth.inputs("mul", name)
    _, _, signed, k, _, _ = synth.MUL_CASES[name]
    la, da, lb, db = synth.packed("mul", name)
    ba, bb, nbits = c["ba"], c["bb"], c["nbits"]
    if k:
        la, da, ba = low_bits(la, da, ba, c["n"], k)
        lb, db, bb = low_bits(lb, db, bb, c["n"], k)
        nbits = k
    ob, vals, rl, rd = synth.mul_reference(name)
    assert np.array_equal(ob, H.mul_out_bounds(ba, bb, signed))
    within(vals, ob)
    ol, od = oracle.mul_batch(la, da, ba, lb, db, bb, nbits, c["n"], ob, signed=signed)
    assert_batches_equal(rl, rd, ol, od, ob, c["n"], name)
    synth.check_mul_path(name)


@pytest.mark.parametrize("name", list(synth.MUL_CLASS_CASES))
def test_mul_class_reference(H, oracle, name):
    """The multiplier's product classes at their size edges and the degree ladders: the case's
    path from the planner's census (synth.check_mul_class_path), every output degree within
    hm_mul_out_bounds, and the model pinned to the bit-serial oracle on the first two values and
    the last one (a ladder's widest)."""
    from helpers import low_bits
    c = synth.inputs("mulc", name)
    spec = synth.MUL_CLASS_CASES[name]
    k, signed = spec["k"], spec["signed"]
    ob, vals, rl, rd = synth.mul_class_reference(name)
    nbits = k or c["nbits"]
    assert np.array_equal(ob, H.mul_out_bounds(c["ba"][:nbits], c["bb"][:nbits], signed))
    cen = synth.check_mul_class_path(name)
    assert [col["res_bound"] for col in cen["cols"]] == ob.tolist()
    within(vals, ob)
    pick = sorted({0, 1, c["n"] - 1})
    la, da = bm.pack([c["A"][e] for e in pick], c["ba"])
    lb, db = bm.pack([c["B"][e] for e in pick], c["bb"])
    ba, bb = c["ba"], c["bb"]
    if k:
        la, da, ba = low_bits(la, da, ba, len(pick), k)
        lb, db, bb = low_bits(lb, db, bb, len(pick), k)
    ol, od = oracle.mul_batch(la, da, ba, lb, db, bb, nbits, len(pick), ob, signed=signed)
    ml, md = bm.pack([vals[e] for e in pick], ob)
    assert_batches_equal(ml, md, ol, od, ob, len(pick), name)


# ------------------------------------------------------------------ chunks, staging, K > 32
@pytest.mark.parametrize("name", list(synth.WIDE_CASES))
def test_mul_wide_reference(H, oracle, name):
    """The plans with K > 32 on bound-0 u64 operands (test_gpu_mul_chunks.py): every bit is the
    null or the unit polynomial, so the carry-save circuit is ordinary binary arithmetic, and the
    model is held against it, not only against itself: every output polynomial is 0 or 1 and the
    value they spell is a * b mod 2^K (the signed circuit: the wrapping i64 product, the same 64
    bits).  The model equals the bit-serial oracle on the same operands, the output bounds (all 0)
    are hm_mul_out_bounds', and the path holds in the planner's census."""
    from helpers import low_bits
    K, signed = synth.WIDE_CASES[name]
    c = synth.wide_inputs()
    assert c["n"] == 6 and c["nbits"] == 64 and not c["ba"].any()
    ob, vals, rl, rd = synth.wide_reference(name)
    assert np.array_equal(ob, H.mul_out_bounds(c["ba"][:K], c["bb"][:K], signed)) and not ob.any()
    mask = (1 << K) - 1
    for (a, b), res in zip(synth.wide_values(), vals):
        assert len(res) == K and set(res) <= {0, 1}
        got = sum(p << i for i, p in enumerate(res))
        assert got == (a * b) & mask, (name, hex(a), hex(b))
        if signed:
            sa, sb = a - (a >> 63 << 64), b - (b >> 63 << 64)
            assert -2**63 <= sa < 2**63 and got == (sa * sb) % 2**64
    vs = synth.wide_values()
    assert vs[0][0] == 0 and vs[1] == (2**64 - 1, 2**64 - 1) and vs[4][1] == 0
    assert vs[2][0] ^ vs[2][1] == 2**64 - 1 and vs[5] == (2**63 + 1, 2**63 + 1)
    la, da, ba = low_bits(*c["a"], c["ba"], c["n"], K)
    lb, db, bb = low_bits(*c["b"], c["bb"], c["n"], K)
    ol, od = oracle.mul_batch(la, da, ba, lb, db, bb, K, c["n"], ob, signed=signed)
    assert_batches_equal(rl, rd, ol, od, ob, c["n"], name)
    cen = synth.check_mul_wide_path(name)
    assert [col["res_bound"] for col in cen["cols"]] == ob.tolist()


def test_wide_stage_reference(H, oracle):
    """The K = 33 plan with a_32 at bound 64 (synth.wide_stage_inputs): it builds within 10^5 arena
    words per value on both product settings, its column 32 alone reads the wide bit, and the model
    equals the oracle."""
    from helpers import low_bits
    c = synth.wide_stage_inputs()
    K, i = c["K"], synth.WIDE_STAGE_BIT
    assert np.array_equal(c["ob"], H.mul_out_bounds(c["ba"][:K], c["bb"][:K]))
    assert c["ob"].tolist() == [0] * 32 + [64]
    assert sorted(synth.model.degree(v[i]) for v in c["A"]) == [0, 0, 5, 40, 63, 64]
    for mfma in (True, False):
        cen = synth.wide_census("low33", mfma, c["ba"])
        assert cen["astride"] < 10**5 and [col["res_bound"] for col in cen["cols"]] == c["ob"].tolist()
    la, da, ba = low_bits(*c["a"], c["ba"], c["n"], K)
    lb, db, bb = low_bits(*c["b"], c["bb"], c["n"], K)
    ol, od = oracle.mul_batch(la, da, ba, lb, db, bb, K, c["n"], c["ob"])
    assert_batches_equal(*c["ref"], ol, od, c["ob"], c["n"], "K = 33, a_32 at bound 64")
    for how in synth.CORRUPTIONS:
        e, _ = synth.corruption_site(c["A"], c["ba"], how, [i], first=4)
        assert e >= 4


def test_stage_references_and_corruptions(H, oracle):
    """The staging-validation batch (u8 at 383, 8 scheduled values): its references equal the
    oracle's; every corruption changes exactly one limb or one degree word of a value with index
    >= 3, inside the bit's own limbs, and leaves a batch that load_bit's rules refuse."""
    from helpers import low_bits, offsets
    c = synth.stage_inputs()
    n = c["n"]
    for what, k in (("low4", 4), ("full", 8)):
        ob, vals, rl, rd = synth.stage_reference(what)
        assert np.array_equal(ob, H.mul_out_bounds(c["ba"][:k], c["bb"][:k]))
        within(vals, ob)
        la, da, ba = low_bits(*c["a"], c["ba"], n, k)
        lb, db, bb = low_bits(*c["b"], c["bb"], n, k)
        ol, od = oracle.mul_batch(la, da, ba, lb, db, bb, k, n, ob)
        assert_batches_equal(rl, rd, ol, od, ob, n, what)
    assert synth.mul_census("ppv_12w")["pp_instance"] == "mul_ppv_kernel"  # the plan at 383
    for op in ("and", "not"):
        ob, vals, rl, rd = synth.stage_reference(op)
        ol, od = oracle.gate_batch(op, *c["a"], c["ba"], *c["b"], c["bb"], 8, n, ob)
        assert_batches_equal(rl, rd, ol, od, ob, n, op)
    cap, off = 6, offsets(c["ba"])[0]
    stride = 8 * cap
    for X in ("a", "b"):
        l0, d0 = c[X]
        for how in synth.CORRUPTIONS:
            for bits in (range(4), [5], range(8)):
                e, i = synth.corruption_site(c[X.upper()], c["ba"], how, bits)
                assert e >= synth.STAGE_CHUNK and i in bits
                l1, d1 = synth.corrupt(l0, d0, c["ba"], n, e, i, how)
                dl, dd = np.flatnonzero(l0 != l1), np.flatnonzero(d0 != d1)
                assert len(dl) + len(dd) == 1
                base = e * stride + int(off[i])
                assert all(base <= g < base + cap for g in dl) and all(g == e * 8 + i for g in dd)
                # what load_bit checks, on the corrupted bit
                p = synth.model.limbs_to_int(l1[base: base + cap])
                d = int(d1[e * 8 + i])
                assert d > synth.STAGE_BOUND or p.bit_length() - 1 > d or (d > 0 and not p >> d & 1)


@pytest.mark.parametrize("name", synth.STALE_LADDERS)
def test_stale_arena_references(H, oracle, name):
    """The descending ladders are the ladder's own rows, permuted; the interleaved batch's model
    equals the oracle, and its null and unit blocks are what they are named for."""
    from helpers import low_bits
    c = synth.inputs("mulc", name)
    la, da, lb, db, ob, rl, rd = synth.descending(name)
    _, _, fl, fd = synth.mul_class_reference(name)
    n, k = c["n"], synth.MUL_CLASS_CASES[name]["k"]
    stride = int((ob // 64 + 1).sum())
    assert np.array_equal(rl.reshape(n, stride)[::-1], fl.reshape(n, stride))
    assert np.array_equal(rd.reshape(n, k)[::-1], fd.reshape(n, k))
    pa, pd, _, _ = synth.packed("mulc", name)
    sa = pa.size // n
    assert np.array_equal(la.reshape(n, sa)[::-1], pa.reshape(n, sa))
    t = synth.interleaved(name)
    assert t["n"] == 16 and np.array_equal(t["ob"], ob)
    assert all(p == 0 for v in t["A"][4:6] + t["B"][6:8] for p in v)
    assert all(p == 1 for v in t["A"][12:15] + t["B"][12:14] + t["B"][15:] for p in v)
    for blk in (0, 8):
        assert all(p.bit_length() - 1 == int(b) for v in t["A"][blk:blk + 4] for p, b in zip(v, t["ba"]))
    xa, xd, ba = low_bits(*t["a"], t["ba"], 16, k)
    xb, xe, bb = low_bits(*t["b"], t["bb"], 16, k)
    ol, od = oracle.mul_batch(xa, xd, ba, xb, xe, bb, k, 16, ob)
    assert_batches_equal(*t["ref"], ol, od, ob, 16, name)


def test_chunk_cases_are_the_tier_s():
    """Every chunked case is a case of the full-bounds tier with n = 10, so that chunks of 1, 3 and
    4 give 10 chunks, 3 + 3 + 3 + 1 and 4 + 4 + 2."""
    for family, name in synth.CHUNK_CASES:
        assert synth.inputs(family, name)["n"] == 10
        spec, ref = synth.mul_spec(family, name)
        assert ref(name)[2].size and set(spec) == {"k", "signed", "ka"}


# ------------------------------------------------------------------ decryption
@pytest.mark.parametrize("name", list(synth.DEC_CASES))
def test_dec_reference(oracle, name):
    c = synth.inputs("dec", name)
    la, da, _, _ = synth.packed("dec", name)
    sk, _, _ = oracle.keygen(*synth.DEC_PARAMS, synth.SEED)
    s, _ = synth.model.keygen(*synth.DEC_PARAMS, synth.SEED)
    assert synth.model.limbs_to_int(sk) == s
    want = oracle.decrypt_batch(sk, la, da, c["ba"], 8, c["n"])
    assert np.array_equal(synth.dec_reference(name), want)
    assert 0 < int(np.unpackbits(want).sum()) < want.size * 8  # neither all zeros nor all ones
    synth.check_dec_path(name)


# ------------------------------------------------------------------ select, min / max
@pytest.mark.parametrize("name", list(synth.SELECT_CASES))
def test_select_reference(H, name):
    """select_model pinned by a second evaluation, b_i + c a_i + c b_i over the gate model (two
    products on gf2_model.clmul_fast instead of one on clmul); bounds against hm_select_out_bounds;
    the path, the fills and the plan's slots in synth.check_select_path."""
    c = synth.inputs("select", name)
    assert 8 <= c["n"] <= 12 and len(synth.packed("select", name)) == 6
    ob, vals, _, _ = synth.select_reference(name)
    assert np.array_equal(ob, H.select_out_bounds(c["bc"][0], c["ba"], c["bb"]))
    within(vals, ob)
    for cv, a, b, out in zip(c["C"], c["A"], c["B"], vals):
        cc = [cv[0]] * len(a)
        ca, cb = synth.gate_circuit("and", cc, a), synth.gate_circuit("and", cc, b)
        assert [y ^ p ^ q for y, p, q in zip(b, ca, cb)] == out
        assert cv[1:] == [0] * 7
    synth.check_select_path(name)


@pytest.mark.parametrize("name", list(synth.MINMAX_CASES))
def test_minmax_reference(H, name):
    """select_model's min / max pinned in the residue ring (a ring homomorphism): the borrow
    recurrence run on the operands' residues, then b_i + w a_i + w b_i (min) or a_i + ... (max);
    bounds against hm_minmax_out_bounds; synth.check_minmax_path."""
    c = synth.inputs("minmax", name)
    assert 8 <= c["n"] <= 12
    g = residue_modulus(19)
    mul = synth.model.residue_mul(g)
    res = lambda p: synth.model.residue_int(p, g)  # noqa: E731
    RA = [[res(p) for p in v] for v in c["A"]]
    RB = [[res(p) for p in v] for v in c["B"]]
    n = c["nbits"]
    for signed in (False, True):
        RW = []
        for ra, rb in zip(RA, RB):
            w = 0
            for i in range(n):
                gen = ra[i] if signed and i == n - 1 else rb[i]
                w = mul(ra[i], rb[i]) ^ gen ^ mul(ra[i] ^ rb[i] ^ 1, w)
            RW.append(w)
        for op in ("min", "max"):
            ob, vals, _, _ = synth.minmax_reference(name, op, signed)
            assert np.array_equal(ob, H.minmax_out_bounds(c["ba"], c["bb"]))
            within(vals, ob)
            for ra, rb, w, out in zip(RA, RB, RW, vals):
                keep = rb if op == "min" else ra
                for i in range(n):
                    assert res(out[i]) == keep[i] ^ mul(w, ra[i]) ^ mul(w, rb[i]), (op, signed, i)
    synth.check_minmax_path(name)


# ------------------------------------------------------------------ lookup
@pytest.mark.parametrize("name", list(synth.LOOKUP_CASES))
def test_lookup_reference(H, name):
    """lookup_model pinned by the other doubling order: the reference multiplies the monomials up
    from their lowest bit over all k index bits (lookup_model.monomials); synth.lookup_trace forms
    them on the top bit within the low and the high half, as the kernel does, and accumulates
    MH[t] I_jt on clmul_fast.  Both must give the same polynomials for all three tables; bounds
    against hm_lookup_out_bounds and the plan driver; synth.check_lookup_path."""
    import lookup_model as lm
    c = synth.inputs("lookup", name)
    assert 8 <= c["n"] <= 12
    for which in synth.LOOKUP_TABLES:
        t = synth.lookup_table(name, which)
        ob, vals, _, _ = synth.lookup_reference(name, which)
        assert np.array_equal(ob, H.lookup_out_bounds(c["ba"], t, c["k"]))
        plan, tr = synth.lookup_traces(name, which)
        assert plan["bounds"] == ob.tolist()
        within(vals, ob)
        assert [out for _, _, _, out in tr] == vals, which
    t = synth.lookup_table(name, "random")
    assert lm.lookup_circuit(c["A"][-1], t) == synth.lookup_reference(name, "random")[1][-1]
    masks = lm.coefficient_masks(synth.lookup_table(name, "all"))
    assert masks[0] == (1 << (1 << c["k"])) - 1  # t[0] = 1: every monomial in output bit 0
    assert lm.coefficient_masks(synth.lookup_table(name, "top"))[0] == 1 << ((1 << c["k"]) - 1)
    synth.check_lookup_path(name)


# ------------------------------------------------------------------ shift
@pytest.mark.parametrize("name", list(synth.SHIFT_CASES))
def test_shift_reference(H, name):
    """shift_model (stages ascending) pinned by the kernel's own order: synth.shift_trace runs the
    stages from the widest step down on clmul_fast, skipping null amounts, and shift_circuit(order
    descending) on the last value; bounds against hm_shift_out_bounds and the plan driver;
    synth.check_shift_path in all five modes."""
    import shift_model as shm
    c = synth.inputs("shift", name)
    assert 8 <= c["n"] <= 12
    ops = {"shl": H.HomomorphicShiftLeft, "shr": H.HomomorphicShiftRight,
           "rotl": H.HomomorphicRotateLeft, "rotr": H.HomomorphicRotateRight}
    for op, signed in shm.MODES:
        ob, vals, _, _ = synth.shift_reference(name, op, signed)
        assert np.array_equal(ob, H.shift_out_bounds(ops[op], c["ba"], c["bb"]))
        within(vals, ob)
        assert [t[4] for t in synth.shift_traces(name, op, signed)] == vals, (op, signed)
        down = shm.shift_circuit(op, c["A"][-1], c["B"][-1], signed, order=range(c["L"] - 1, -1, -1))
        assert down == vals[-1]
        synth.check_shift_path(name, op, signed)


# ------------------------------------------------------------------ counts, runs, array
def _esym(us, top, mul):
    """e_0 .. e_top of the literals by halving: e_j(L + R) = sum_l e_l(L) e_{j-l}(R) -- not the
    model's one-literal-at-a-time recurrence."""
    if len(us) == 1:
        return [1, us[0]] + [0] * (top - 1)
    h = len(us) // 2
    lo, hi = _esym(us[:h], top, mul), _esym(us[h:], top, mul)
    out = [0] * (top + 1)
    for a, x in enumerate(lo):
        for b, y in enumerate(hi[:top + 1 - a]):
            if x and y:
                out[a + b] ^= mul(x, y)
    return out


@pytest.mark.parametrize("name", list(synth.COUNT_CASES))
def test_count_reference(H, name):
    """bitcount_model pinned in the residue ring by another evaluation order: the elementary
    symmetric polynomials by halving (counts), the runs' prefixes multiplied from the far end;
    bounds against hm_bitcount_out_bounds and the plan driver; synth.check_count_path per op."""
    import bitcount_model as bcm
    c = synth.inputs("count", name)
    assert 8 <= c["n"] <= 12
    g = residue_modulus(23)
    mul = synth.model.residue_mul(g)
    res = lambda p: synth.model.residue_int(p, g)  # noqa: E731
    RA = [[res(p) for p in v] for v in c["A"]]
    ops = {op: getattr(H, "Homomorphic" + "".join(w.title() for w in op.split("_")))
           for op in bcm.OPS}
    for op in synth.COUNT_CASES[name][1]:
        run, zeros, leading = bcm.OPS[op]
        ob, vals, _, _ = synth.count_reference(name, op)
        assert np.array_equal(ob, H.bitcount_out_bounds(ops[op], c["ba"]))
        within(vals, ob)
        for ra, out in zip(RA, vals):
            u = [x ^ 1 for x in ra] if zeros else list(ra)
            if run:
                v = u[::-1] if leading else u
                want = [0] * 8
                for j in range(1, 9):
                    t = 1
                    for x in reversed(v[:j]):
                        t = mul(x, t)
                    for k in range(4):
                        if j % (1 << k) == 0:
                            want[k] ^= t
            else:
                e = _esym(u, 8, mul)
                want = [e[1 << k] if k < 4 else 0 for k in range(8)]
            assert [res(p) for p in out] == want, op
        assert [t[-1] for t in synth.count_traces(name, op)] == vals, op  # the pruned recurrence
        synth.check_count_path(name, op)


@pytest.mark.parametrize("name", list(synth.ARRAY_CASES))
def test_array_reference(H, name):
    """array_model's tree pinned by array_model.circuit_read_sum (the indicator sum), the write by
    T + ind x + ind T on clmul_fast; bounds against hm_array_*_out_bounds and the plan driver;
    synth.check_array_path."""
    import array_model as am
    c = synth.inputs("array", name)
    assert 8 <= c["n"] <= 12 and len(c["A"]) == c["n"] * c["count"]
    assert len(synth.packed("array", name)) == 6
    fast = synth.model.clmul_fast
    ob, vals, _, _ = synth.array_reference(name, "read")
    assert np.array_equal(ob, H.array_read_out_bounds(c["ba"], c["count"], c["bb"]))
    within(vals, ob)
    for arr, s, out in zip(c["arrays"], c["B"], vals):
        assert am.circuit_read_sum(arr, s, fast) == out
    ob, vals, _, _ = synth.array_reference(name, "write")
    assert np.array_equal(ob, H.array_write_out_bounds(c["ba"], c["bc"], c["count"], c["bb"]))
    within(vals, ob)
    at = 0
    for arr, s, x in zip(c["arrays"], c["B"], c["C"]):
        for v, el in enumerate(arr):
            ind = am.indicator(s, v, c["k"], fast)
            assert [T ^ fast(ind, xj) ^ fast(ind, T) for T, xj in zip(el, x)] == vals[at]
            at += 1
    synth.check_array_path(name)
