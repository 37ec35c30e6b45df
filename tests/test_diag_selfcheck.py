"""CPU checks of what the device diagnostics' tests are built from
(tests/diag_util.py and the operand generators of test_gpu_field_diag.py,
test_gpu_group_diag.py, test_gpu_scalar_diag.py): every operand class lies
inside the bound it claims, tests/bounds_model.py accepts its hull without
Overflow, and the exact references agree with each other.  No GPU."""
import random

import pytest

import bounds_model as bm
import diag_util as du
import test_gpu_field_diag as tf
import test_gpu_group_diag as tg
import test_gpu_scalar_diag as ts
from diag_util import L, P


def test_limb_value_round_trips():
    rng = random.Random(91)
    vals = du.FE_SPECIAL + [rng.randrange(-P, 2 * P) for _ in range(200)]
    for v in vals:
        for l in (du.fe_centered(v), du.fe_centered(v, False) if abs(v) < 2**255 else du.fe_centered(v)):
            assert du.fe_val(l) == v % P
        if abs(v) < 3 * 2**254:
            assert du.fe_int(du.fe_digits(v)) == v
            assert du.fe_int(du.fe_centered(v, False)) == v
        assert du.within(du.fe_centered(v), [-x for x in du.TIGHT], du.TIGHT)
        assert du.from_words(du.canonical_words(v)) == v % P
    for z in du.fe_zero_vectors():
        assert du.fe_val(z) == 0
    for v in [0, 1, P - 1, P, 15 * P, 16 * P - 1] + [rng.randrange(16 * P) for _ in range(100)]:
        for l in du.r16_splits(v, rng, 4):
            assert du.r16_int(l) == v and max(l) < du.R16_IN
    assert all(max(du.r16_random_tight(rng)) <= du.R16_TIGHT for _ in range(100))
    assert [du.s32(x) for x in (0, 1, 2**31 - 1, 2**31, 2**32 - 1)] == [0, 1, 2**31 - 1, -2**31, -1]


def test_edwards_references_agree():
    rng = random.Random(92)
    pts = [du.random_point(rng) for _ in range(8)] + du.TORSION + [du.BASE]
    for a in pts:
        assert du.on_curve(a)
        assert du.ed_dbl(a) == du.ed_add(a, a)
        assert du.ed_add(a, du.ed_neg(a)) == du.IDENT
        assert du.ed_add(a, du.IDENT) == a
    assert du.ed_mul(2, du.ORDER2) == du.IDENT and du.ORDER2 != du.IDENT
    for t in du.ORDER4:
        assert du.ed_mul(2, t) == du.ORDER2
    assert du.ed_mul(4, du.ORDER8) == du.ORDER2 and du.ed_mul(8, du.ORDER8) == du.IDENT
    assert du.ed_mul(L, du.BASE) == du.IDENT
    a, b, c = pts[:3]
    assert du.ed_add(du.ed_add(a, b), c) == du.ed_add(a, du.ed_add(b, c))
    assert du.ed_mul(5, a) == du.ed_add(du.ed_dbl(du.ed_dbl(a)), a)


@pytest.mark.parametrize("op", list(tf.OPS))
def test_fe_classes_are_inside_their_bounds_and_the_model_accepts_them(op):
    bf, bg, _, model = tf.OPS[op]
    for label, pairs in tf.classes_for(op).items():
        fs = [f for f, _ in pairs]
        gs = [g for _, g in pairs if g is not None]
        hi = tf.unsigned_2x() if label == "unsigned" else bf
        lo = [0] * 10 if label == "unsigned" else [-x for x in bf]
        assert all(du.within(f, lo, hi) for f in fs), (op, label)
        assert all(du.within(g, [-x for x in bg], bg) for g in gs), (op, label)
        out = model(du.hull(fs), du.hull(gs) if gs else None)          # raises bm.Overflow if it does not fit
        assert len(out) == 10
    # the whole bound at once, as tests/test_bounds.py feeds it
    full = [(-x, x) for x in bf]
    model(full, [(-x, x) for x in bg] if bg else None)


def test_exponentiation_operands():
    zs = tf.pow_operands()
    assert all(du.within(z, [-x for x in du.TIGHT], du.TIGHT) for z in zs)
    bm.fe_pow22523(du.hull(zs))
    tf.model_invert(du.hull(zs))
    z = zs[6]
    assert du.fe_val([lo for lo, _ in tf.pow_exact(du.point_iv(z))]) == pow(du.fe_val(z), 2**252 - 3, P)


def test_carry_patterns_reach_the_edges():
    """class (d) does what it says: restating the floor chains of a product
    with (1, 0, .., 0) on these column sums, some column (with its incoming
    carry) is exactly 2^w - 1, 2^w, -1; and of fe_carry's centered chain,
    some column is exactly at the rounding boundary +-2^(w-1)"""
    floor_hits, centered_hits = set(), set()
    for g in tf.carry_patterns():
        c = 0
        for k in range(5):
            t = g[k] + c
            floor_hits.add(("A", k, t - (1 << du.W[k])))
            c = t >> du.W[k]
        c = 0
        for k in range(5, 10):
            t = g[k] + c
            floor_hits.add(("B", k, t - (1 << du.W[k])))
            c = t >> du.W[k]
        floor_hits.add(("wrap", 0, 19 * c + (g[0] & ((1 << 26) - 1)) - (1 << 26)))
        c = 0
        for k in range(10):     # a plain centered chain (the device's two chains carry limbs 0 and 4 twice)
            t = g[k] + c
            centered_hits.add((k, t - (1 << (du.W[k] - 1))))
            centered_hits.add((k, t + (1 << (du.W[k] - 1))))
            c = (t + (1 << (du.W[k] - 1))) >> du.W[k]
    for k in range(10):
        ch = "A" if k < 5 else "B"
        assert {(ch, k, -1), (ch, k, 0)} <= floor_hits, k                       # 2^w - 1 and 2^w
        assert (ch, k, -1 - (1 << du.W[k])) in floor_hits, k                    # -1
        assert {(k, -1), (k, 0)} <= centered_hits, k                            # 2^(w-1) - 1 and 2^(w-1)
    assert {("wrap", 0, -1), ("wrap", 0, 0)} <= floor_hits


@pytest.mark.parametrize("s,bound,centered", [(1, "B33", False), (1, "B33", True), (2, "TIGHT", False), (2, "TIGHT", True),
                                              (2, "unsigned", False)])
def test_squaring_carry_operands_reach_the_edges(s, bound, centered):
    """class (d) for the squarings' own chains (fe_sqs_u's two floor chains,
    join and wrap; the centered chain of fe_sq / fe_sq2 / fe_sq_sh): every
    column that takes a carry is put exactly on both of its edges, within
    the operation's input bound"""
    hi = tf.unsigned_2x() if bound == "unsigned" else getattr(du, bound)
    fs, reached, wanted = tf.sq_carry_operands(s, hi, centered)
    assert reached == wanted, sorted(wanted - reached)
    assert len(wanted) == (18 if centered else 20)
    assert all(du.within(f, [0] * 10, hi) for f in fs)
    totals = tf.centered_totals if centered else tf.floor_totals
    hit = {(k, t) for f in fs for k, t in totals(tf.sq_columns(f, s)).items()}
    assert wanted <= hit
    for f in fs:        # the restated columns are the square's
        col = tf.sq_columns(f, s)
        assert sum(c << du.OFF[k] for k, c in enumerate(col)) % P == s * du.fe_val(f) ** 2 % P


def test_ge16_operands_reach_the_tight_bound():
    """the 16-lane steps' p3 operands include limbs of exactly 2^16 + 63 in
    lanes 0, 1 and 15 of every row, on points of the curve"""
    rng = random.Random(96)
    for lx in (False, True):
        _, rows = tg.ge16_dbl_rows(rng, lx)
        _check_rows_at_bound([r[:64] for r in rows])
    for neg in (False, True):
        _, rows = tg.ge16_add_rows(rng, neg)
        assert all(0 <= min(r) and max(r[:64]) < 2**17 and max(r[64:]) < du.R16_IN for r in rows)
        if not neg:
            _check_rows_at_bound([r[:64] for r in rows])
            assert any(max(r[64:80]) > 2**17 + 2**16 for r in rows)      # Y + 4p - X from limbs above 0xffff
        else:   # rows 0 and 3 are 4p - tight: down to 4p's limb - (2^16 + 63)
            assert any(r[0] == tg.P4[0] - du.R16_TIGHT for r in rows) and any(r[48 + 15] == tg.P4[15] - du.R16_TIGHT for r in rows)
    cases, rows = tg.ge16_qc_rows(rng)
    _check_rows_at_bound(rows)
    for (pt, z), r in zip(cases, rows):
        assert [du.r16_val(r[16 * q:16 * q + 16]) for q in range(4)] == tg.p3_vals(pt, z)


def _check_rows_at_bound(rows):
    assert all(0 <= min(r) and max(r) <= du.R16_TIGHT for r in rows)
    for q in range(4):
        for c in (0, 1, 15):
            assert any(r[16 * q + c] == du.R16_TIGHT for r in rows), (q, c)
    assert any(r[16 * q:16 * q + 16] == [du.R16_TIGHT] * 16 for r in rows for q in range(4))


def test_r16_operands():
    rng = random.Random(93)
    assert all(0 <= min(x) and max(x) < du.R16_IN for x in tf.r16_operands(rng))
    xs = tf.iszero_cases()
    assert all(0 <= min(x) and max(x) < du.R16_IN for x in xs)
    ks = {du.r16_int(x) // P for x in xs if du.r16_int(x) % P == 0}
    assert set(range(16)) <= ks
    near = {du.r16_int(x) % P for x in xs}
    assert {1, P - 1} <= near


def test_group_operand_representations():
    rng = random.Random(94)
    vals = [0, 1, P - 1, du.SQRTM1] + [rng.randrange(P) for _ in range(200)]
    for v in vals:
        assert du.within(tg.rep_tight(v, rng), [-x for x in du.TIGHT], du.TIGHT)
        u = tg.rep_unsigned(v, rng)
        assert du.within(u, [0] * 10, tf.unsigned_2x()) and du.fe_val(u) == v
        w = tg.rep_wide3(v, rng)
        assert du.within(w, [-x for x in du.bound(3.04)], du.bound(3.04)) and du.fe_val(w) == v
        y = tg.rep_y4(v, rng)
        assert du.within(y, [0] * 10, du.bound(4.01)) and du.fe_val(y) == v
        for kind in (0, 1, 2):
            l = tg.r16_rep(v, rng, kind)
            assert du.r16_val(l) == v and max(l) <= du.R16_TIGHT
    for a, b in tg.pairs()[:20]:
        z = rng.randrange(1, P)
        X, Y, Z, T = tg.p3_vals(a, z)
        assert tg.affine_p3([X, Y, Z, T]) == a
        for kind in (0, 1):
            q = tg.qc16(b, z, rng, kind)
            assert max(max(r) for r in q) < du.R16_IN and min(min(r) for r in q) >= 0
            c = tg.cached_vals(b, z)
            assert [du.r16_val(r) for r in q] == [c[1], c[0], c[3], c[2]]
    # the pairs hold what the issue lists
    ps = tg.pairs()
    assert any(du.ed_add(a, b) == du.IDENT and a != du.IDENT for a, b in ps)           # P with -P
    assert any(a == b and a not in du.TORSION for a, b in ps)                          # P with P
    assert any(du.ed_add(a, du.ed_neg(b)) in du.TORSION[1:] and a not in du.TORSION for a, b in ps)
    for t in du.TORSION + [du.BASE]:
        assert any(a == t for a, _ in ps) and any(b == t for _, b in ps)


def test_scalar_case_lists():
    rng = random.Random(95)
    xs = du.scalar_edges_512(rng, 10)
    assert any(2**252 <= x % L < L for x in xs) and {L - 1, L, L + 1, 2**512 - 1} <= set(xs)
    assert all(x < L for x in du.scalar_edges_lt_l(rng, 10))
    cases = ts.digits160_cases()
    assert all(c < 2**131 and d < 2**(4 * W - 1) and 33 <= W <= ts.WMAX for c, d, W in cases)
    for dbits in (131, 151):
        assert any(d.bit_length() == dbits and d & 1 for _, d, _ in cases)
