"""Device group steps on chosen points and representations
(libfd_ed25519_diag.so): the one-lane steps of fd25519_ge.h, the quad
steps of fd25519_ge4.h and the 16-lane steps of fd25519_r16.h, one step
per kernel, against exact affine Edwards arithmetic.

The verify loops only apply these steps to what they produce themselves.
Here the operands are random points, every torsion point, B, and the pairs
P / -P, P / P and P / P + torsion, under several projective scalings, with
coordinates given as limb vectors up to the bound the headers state for
that operand position (fd25519_ge.h:34-44, 85-90, 110-113, 131-140):
unsigned-form products in [0, 2x], table entries up to 3.04x, completed
points' X, Z, T within 3x and Y in [-1x, 4x], tight otherwise; r16 limbs
tight (up to 2^16 + 63) and, for the qc operand, below 2^19.  Digits of a
given value never sit exactly on such a bound, so the coordinate that the
projective scaling leaves free is given as a limb vector at the bound
(at_bound, p3_bound16) and the others follow from its value.

Per case: the output converted to affine equals the exact result; a p3
output has T Z = X Y; every output limb lies in the interval
tests/bounds_model.py derives from the hull of the class (ge), or within
the bound the header states for it (ge4, ge16); and the one-lane, quad and
16-lane forms of the same step give the same affine point."""
import random

import pytest

import bounds_model as bm
import diag_util as du
from diag_util import D2, P, Diag, s32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def diag():
    return Diag()


def inv(v):
    assert v % P
    return pow(v, P - 2, P)


# ---- coordinate representations (radix 2^25.5) -------------------------------

def rep_tight(v, rng):
    return du.fe_centered(v % P)


def rep_unsigned(v, rng):
    """what a _u product returns: the digits, limbs 1 and 6 up to 2^10 above
    2^w (the joins' carries, fd25519_fe.h:231-234)"""
    c1, c6 = rng.choice((0, 0, 1, 1023)), rng.choice((0, 0, 1, 1023))
    l = du.fe_digits((v - (c1 << du.OFF[1]) - (c6 << du.OFF[6])) % P)
    l[1] += c1
    l[6] += c6
    return l


def rep_wide3(v, rng):
    """within 3x (+1): centered digits plus / minus (2^w at limb i, -1 at limb i+1)"""
    l = du.fe_centered(v % P)
    for i in range(9):
        s = rng.choice((-1, 0, 1))
        l[i] += s << du.W[i]
        l[i + 1] -= s
    return l


def rep_y4(v, rng):
    """a completed point's Y: the sum of two unsigned forms, in [0, 4x]"""
    a = rng.randrange(P)
    return [x + y for x, y in zip(rep_unsigned(a, rng), rep_unsigned(v - a, rng))]


def at_bound(mult, rng, lo_mult=None):
    """every limb exactly at the stated bound: +mult units, or (at random,
    limb by limb) the lower bound, -mult unless given.  Canonical or
    centered digits never sit there, so such a vector is given to the
    coordinate the projective scaling leaves free (Z, or a cached entry's
    2Z) and the other coordinates follow from its value."""
    hi, lo = du.bound(mult), du.bound(-mult if lo_mult is None else lo_mult)
    while True:
        v = [rng.choice((a, a, b)) for a, b in zip(hi, lo)]
        if du.fe_val(v):
            return v


def mk(vals, reps, rng):
    """limb vectors for the coordinate values, one representation each"""
    return [r(v, rng) for v, r in zip(vals, reps)]


SCALINGS = (1, 2, P - 1, None, None)      # Z; None: random


def zs(rng):
    return [z if z is not None else rng.randrange(1, P) for z in SCALINGS]


def p3_vals(pt, z):
    x, y = pt
    return [x * z % P, y * z % P, z % P, x * y * z % P]


def cached_vals(pt, z, nt=False):
    X, Y, Z, T = p3_vals(pt, z)
    t2d = D2 * T % P
    return [(Y + X) % P, (Y - X) % P, 2 * Z % P, (-t2d if nt else t2d) % P]


def val4(o, n=4):
    return [du.fe_val([s32(v) for v in o[10 * q:10 * q + 10]]) for q in range(n)]


def limbs4(o, n=4):
    return [[s32(v) for v in o[10 * q:10 * q + 10]] for q in range(n)]


def affine_p1p1(v):
    X, Y, Z, T = v
    return (X * inv(Z) % P, Y * inv(T) % P)


def affine_p3(v, has_t=True):
    X, Y, Z = v[:3]
    if has_t:
        assert v[3] * Z % P == X * Y % P
    return (X * inv(Z) % P, Y * inv(Z) % P)


def hull_pt(rows, names):
    """rows: per case, one limb vector per field -> bounds_model's point of hulls"""
    return {n: du.hull([r[i] for r in rows]) for i, n in enumerate(names)}


def assert_inside(out_limbs, model_pt, names, ctx):
    for i, n in enumerate(names):
        assert du.inside(out_limbs[i], model_pt[n]), (ctx, n, out_limbs[i], model_pt[n])


P3N = ("X", "Y", "Z", "T")
CN = ("YplusX", "YminusX", "Z2", "T2d")
PN = ("yplusx", "yminusx", "xy2d")


def pairs():
    return du.point_pairs(random.Random(71))


def singles():
    return [a for a, _ in pairs()]


# ---- ge: one lane -----------------------------------------------------------------

@pytest.mark.parametrize("op", ["p2_dbl", "p3_dbl"])
def test_ge_dbl(diag, op):
    rng = random.Random(72)
    cases, rows = [], []
    for pt in singles():
        for z in zs(rng):
            for reps in ((rep_unsigned,) * 4, (rep_tight,) * 4, (rep_tight, rep_unsigned, rep_unsigned, rep_tight),
                         (rep_unsigned, rep_tight, rep_tight, rep_unsigned)):
                cases.append(pt)
                rows.append(mk(p3_vals(pt, z), reps, rng))
        # Z exactly at its bound: 2x (fd25519_ge.h:85 "|X|, |Y|, |Z| <= 2x"), and the tight 1.01x at either sign
        for zl, reps in ((at_bound(2.0, rng, 0), (rep_unsigned,) * 4), (at_bound(1.01, rng), (rep_tight,) * 4)):
            r = mk(p3_vals(pt, du.fe_val(zl)), reps, rng)
            r[2] = zl
            cases.append(pt)
            rows.append(r)
    out = diag.run("ge", op, [sum(r, []) for r in rows])
    model = bm.p2_dbl(hull_pt(rows, P3N))
    for pt, r, o in zip(cases, rows, out):
        assert affine_p1p1(val4(o)) == du.ed_dbl(pt) == du.ed_add(pt, pt), (op, pt, r)
        assert_inside(limbs4(o), model, P3N, (op, pt))
    print(f"ge_{op}: {len(cases)} cases")


@pytest.mark.parametrize("nt", [False, True])
def test_ge_add(diag, nt):
    rng = random.Random(73)
    cases, prow, qrow = [], [], []
    for a, b in pairs():
        for z1, z2 in zip(zs(rng), reversed(zs(rng))):
            for pr, qr in (((rep_unsigned,) * 4, (rep_wide3, rep_wide3, rep_wide3, rep_unsigned)),
                           ((rep_tight,) * 4, (rep_tight,) * 4),
                           ((rep_unsigned, rep_tight, rep_unsigned, rep_tight), (rep_wide3, rep_tight, rep_wide3, rep_wide3))):
                cases.append((a, b))
                prow.append(mk(p3_vals(a, z1), pr, rng))
                qrow.append(mk(cached_vals(b, z2, nt), qr, rng))
        # the entry's 2Z exactly at the table bound 3.04x (tests/test_bounds.py), P's Z at the unsigned 2x
        z2l, z1l = at_bound(3.04, rng), at_bound(2.0, rng, 0)
        p = mk(p3_vals(a, du.fe_val(z1l)), (rep_unsigned,) * 4, rng)
        q = mk(cached_vals(b, du.fe_val(z2l) * inv(2) % P, nt), (rep_wide3, rep_wide3, rep_wide3, rep_unsigned), rng)
        p[2], q[2] = z1l, z2l
        cases.append((a, b))
        prow.append(p)
        qrow.append(q)
    out = diag.run("ge", "add_nt" if nt else "add", [sum(p + q, []) for p, q in zip(prow, qrow)])
    model = bm.ge_add(hull_pt(prow, P3N), hull_pt(qrow, CN), nt)
    for (a, b), o in zip(cases, out):
        assert affine_p1p1(val4(o)) == du.ed_add(a, b), (nt, a, b)
        assert_inside(limbs4(o), model, P3N, (nt, a, b))
    print(f"ge_add<{nt}>: {len(cases)} cases")


def test_ge_madd(diag):
    rng = random.Random(74)
    cases, prow, qrow = [], [], []
    for a, b in pairs():
        for z in zs(rng):
            for pr in ((rep_unsigned, rep_unsigned, rep_tight, rep_unsigned), (rep_tight,) * 4):
                cases.append((a, b))
                prow.append(mk(p3_vals(a, z), pr, rng))
                qrow.append(mk(cached_vals(b, 1)[:2] + [D2 * b[0] * b[1] % P], (rep_tight,) * 3, rng))
        zl = at_bound(1.01, rng)        # P's centered Z exactly at the tight bound
        p = mk(p3_vals(a, du.fe_val(zl)), (rep_unsigned, rep_unsigned, rep_tight, rep_unsigned), rng)
        p[2] = zl
        cases.append((a, b))
        prow.append(p)
        qrow.append(mk(cached_vals(b, 1)[:2] + [D2 * b[0] * b[1] % P], (rep_tight,) * 3, rng))
    out = diag.run("ge", "madd", [sum(p, []) + sum(q, []) for p, q in zip(prow, qrow)])
    model = bm.ge_madd(hull_pt(prow, P3N), hull_pt(qrow, PN))
    for (a, b), o in zip(cases, out):
        assert affine_p1p1(val4(o)) == du.ed_add(a, b), (a, b)
        assert_inside(limbs4(o), model, P3N, (a, b))
    print(f"ge_madd: {len(cases)} cases")


@pytest.mark.parametrize("uxy", [False, True])
def test_ge_p3_to_cached(diag, uxy):
    rng = random.Random(75)
    reps = (rep_unsigned, rep_unsigned, rep_tight, rep_unsigned) if uxy else (rep_tight,) * 4
    cases, rows = [], []
    for pt in singles():
        for z in zs(rng):
            cases.append((pt, z))
            rows.append(mk(p3_vals(pt, z), reps, rng))
        zl = at_bound(1.01, rng)        # Z exactly at the tight bound: 2Z at 2.02x
        r = mk(p3_vals(pt, du.fe_val(zl)), reps, rng)
        r[2] = zl
        cases.append((pt, du.fe_val(zl)))
        rows.append(r)
    out = diag.run("ge", "to_cached_uxy" if uxy else "to_cached", [sum(r, []) for r in rows])
    model = bm.p3_to_cached(hull_pt(rows, P3N), uxy)
    for (pt, z), o in zip(cases, out):
        assert val4(o) == cached_vals(pt, z), (uxy, pt, z)
        assert_inside(limbs4(o), model, CN, (uxy, pt))
    print(f"ge_p3_to_cached<{uxy}>: {len(cases)} cases")


@pytest.mark.parametrize("op", ["p1p1_to_p2", "p1p1_to_p3", "p1p1_to_p3_u", "p1p1_to_p3_uxyt"])
def test_ge_p1p1_conversions(diag, op):
    rng = random.Random(76)
    cases, rows = [], []
    for pt in singles():
        for zc, tc in zip(zs(rng), reversed(zs(rng))):
            for reps in ((rep_wide3, rep_y4, rep_wide3, rep_wide3), (rep_tight,) * 4,
                         (rep_wide3, rep_unsigned, rep_tight, rep_wide3)):
                cases.append(pt)
                rows.append(mk([pt[0] * zc % P, pt[1] * tc % P, zc, tc], reps, rng))
        # Z and T, both free scalings of a completed point, exactly at 3x (fd25519_ge.h:37-38)
        zl, tl = at_bound(3.0, rng), at_bound(3.0, rng)
        r = mk([pt[0] * du.fe_val(zl) % P, pt[1] * du.fe_val(tl) % P, 0, 0], (rep_wide3, rep_y4, rep_tight, rep_tight), rng)
        r[2], r[3] = zl, tl
        cases.append(pt)
        rows.append(r)
    out = diag.run("ge", op, [sum(r, []) for r in rows])
    h = hull_pt(rows, P3N)
    model = bm.p1p1_to_p2(h) if op == "p1p1_to_p2" else bm.p1p1_to_p3(h, op != "p1p1_to_p3", op == "p1p1_to_p3_u")
    for pt, o in zip(cases, out):
        n = 3 if op == "p1p1_to_p2" else 4
        assert affine_p3(val4(o, n), n == 4) == pt, (op, pt)
        assert_inside(limbs4(o, n), model, P3N[:n], (op, pt))
        if n == 3:
            assert not any(o[30:40])
    print(f"ge_{op}: {len(cases)} cases")


def test_ge_cneg(diag):
    rng = random.Random(77)
    rows = [du.fe_random(rng, 4, du.B33) for _ in range(100)] + [[v] * 4 for v in du.fe_extremes(du.B33)]
    for neg in (0, 1):
        out = diag.run("ge", "cached_cneg", [sum(r, []) + [neg] for r in rows])
        for r, o in zip(rows, out):
            want = [r[1], r[0], r[2], [-x for x in r[3]]] if neg else r
            assert limbs4(o) == want, (neg, r)
        out = diag.run("ge", "precomp_cneg", [sum(r, []) + [neg] for r in rows])
        for r, o in zip(rows, out):
            want = [r[1], r[0], [-x for x in r[2]]] if neg else r[:3]
            assert limbs4(o, 3) == want and not any(o[30:40]), (neg, r)
    print(f"ge_cached_cneg / ge_precomp_cneg: {4 * len(rows)} cases")


# ---- ge4: one quad ------------------------------------------------------------------

def within_units(limbs, lo, hi):
    return all(lo * (1 << (w - 1)) <= l <= hi * (1 << (w - 1)) for l, w in zip(limbs, du.W))


def qc_limbs(p3):
    """the quad's qc of tight p3 limbs, formed limb by limb as ge4_to_qc does
    (sums of two tight values, <= 2.02x); 2dT a tight product"""
    X, Y, Z, T = p3
    return [[y - x for x, y in zip(X, Y)], [y + x for x, y in zip(X, Y)], du.fe_centered(D2 * du.fe_val(T) % P),
            [2 * z for z in Z]]


def ge4_cases(rng, two):
    cases, rows = [], []
    for a, b in pairs() if two else [(a, a) for a in singles()]:
        for z1, z2 in zip(zs(rng), reversed(zs(rng))):
            p = mk(p3_vals(a, z1), (rep_tight,) * 4, rng)
            q = qc_limbs(mk(p3_vals(b, z2), (rep_tight,) * 4, rng))
            cases.append((a, b))
            rows.append((p, q))
    return cases, rows


def test_ge4_dbl_add(diag):
    rng = random.Random(78)
    cases, rows = ge4_cases(rng, False)
    out = diag.run("ge4", "dbl", [sum(p, []) for p, _ in rows])
    for (a, _), o in zip(cases, out):
        assert affine_p1p1(val4(o)) == du.ed_dbl(a), a
        assert all(within_units(l, -3.03, 3.03) for l in limbs4(o)), (a, limbs4(o))   # fd25519_ge4.h:19-21
    nd = len(cases)
    cases, rows = ge4_cases(rng, True)
    ins = [sum(p + q, []) for p, q in rows]
    out = diag.run("ge4", "add", ins)
    for (a, b), o in zip(cases, out):
        assert affine_p1p1(val4(o)) == du.ed_add(a, b), (a, b)
        assert all(within_units(l, -3.03, 3.03) for l in limbs4(o)), (a, b, limbs4(o))
    # quads at the end of a wave's last block: counts that are no multiple of 16
    for n in (1, 3, 17):
        o2 = diag.run("ge4", "add", ins[:n])
        assert (o2 == out[:n]).all()
    print(f"ge4_dbl: {nd} cases, ge4_add: {len(cases)} cases")


def test_ge4_conversions(diag):
    rng = random.Random(79)
    cases, rows = [], []
    for pt in singles():
        for zc, tc in zip(zs(rng), reversed(zs(rng))):
            for reps in ((rep_wide3,) * 4, (rep_tight,) * 4):
                cases.append(pt)
                rows.append(mk([pt[0] * zc % P, pt[1] * tc % P, zc, tc], reps, rng))
    out = diag.run("ge4", "to_p3", [sum(r, []) for r in rows])
    for pt, o in zip(cases, out):
        assert affine_p3(val4(o)) == pt, pt
        assert all(within_units(l, -1.01, 1.01) for l in limbs4(o)), pt
    n3 = len(cases)
    cases, rows = [], []
    for pt in singles():
        for z in zs(rng):
            cases.append((pt, z))
            rows.append(mk(p3_vals(pt, z), (rep_tight,) * 4, rng))
    out = diag.run("ge4", "to_qc", [sum(r, []) for r in rows])
    for (pt, z), r, o in zip(cases, rows, out):
        c = cached_vals(pt, z)
        assert val4(o) == [c[1], c[0], c[3], c[2]], (pt, z)            # (Y-X, Y+X, 2dT, 2Z)
        want = qc_limbs(r)
        got = limbs4(o)
        assert got[0] == want[0] and got[1] == want[1] and got[3] == want[3], (pt, z)
        assert within_units(got[2], -1.01, 1.01)
    for neg in (0, 1):
        for op, lanes in (("cneg_p3", (0, 3)), ("cneg_p1p1", (0,))):
            out = diag.run("ge4", op, [sum(r, []) + [neg] for r in rows])
            for r, o in zip(rows, out):
                want = [[-x for x in l] if (neg and q in lanes) else l for q, l in enumerate(r)]
                assert limbs4(o) == want, (op, neg)
    print(f"ge4_to_p3: {n3} cases, ge4_to_qc: {len(cases)} cases, ge4_cneg: {4 * len(rows)} cases")


# ---- ge16: one wave -----------------------------------------------------------------

P4 = [2**17 - 76] + [2**17 - 2] * 15


def r16_rep(v, rng, kind):
    """tight limbs of v mod p: its digits, the digits of v + p, or either at random"""
    v %= P
    if kind == 2:
        kind = rng.randrange(2)
    l = du.r16_digits(v + P if kind else v)
    assert max(l) <= du.R16_TIGHT
    return l


def p3_bound16(pt, rng, which, lx=False):
    """(X, Y, Z, T) -- or, lx, (X, Y, Z, X) -- of pt with row `which` a limb
    vector at the tight bound (du.r16_at_bound: lanes 0, 1 and 15 exactly
    2^16 + 63, or every lane): canonical digits never exceed 0xffff, so the
    vector is chosen first and the scaling Z solved from it (Z = row / x,
    / y or / xy); where that coordinate of pt is 0 the bound vector is Z
    itself.  The other rows are digits."""
    x, y = pt
    unit = [x, y, 1, x if lx else x * y % P]
    if unit[which] % P == 0:
        which = 2
    t = du.r16_at_bound(rng)
    z = du.r16_val(t) * inv(unit[which]) % P
    rows = [r16_rep(u * z, rng, 2) for u in unit]
    rows[which] = t
    assert [du.r16_val(r) for r in rows] == [u * z % P for u in unit] and z
    return rows, z


def r16_vals(o):
    return [du.r16_val(o[16 * q:16 * q + 16]) for q in range(4)]


def assert_r16_tight(o, ctx):
    for q in range(4):
        assert all(int(v) <= m for v, m in zip(o[16 * q:16 * q + 16], du.R16_OUT_MAX)), (ctx, q, list(o))


def qc16(pt, z, rng, kind):
    """(Y-X, Y+X, 2dT, 2Z) below 2^19: digits, or formed limb by limb from tight limbs as ge16_to_qc does"""
    X, Y, Z, T = p3_vals(pt, z)
    if kind == 0:
        return [du.r16_digits(v % P) for v in ((Y - X), (Y + X), D2 * T, 2 * Z)]
    if kind == 2:       # from a p3 with a row at the tight bound (z is then solved, not the one given)
        (x, y, zz, _), z = p3_bound16(pt, rng, rng.randrange(3))
        T = p3_vals(pt, z)[3]
    else:
        x, y, zz = (r16_rep(v, rng, 2) for v in (X, Y, Z))
    t = du.r16_splits(D2 * T % P, rng, 2)[1]
    return [[b + o - a for a, b, o in zip(x, y, P4)], [a + b for a, b in zip(x, y)], t, [2 * a for a in zz]]


def ge16_dbl_rows(rng, lx):
    cases, rows = [], []
    for pt in singles():
        for z in zs(rng)[:4]:
            for kind in (0, 1, 2):
                v = p3_vals(pt, z)
                if lx:
                    v[3] = v[0]         # (X, Y, Z, X)
                cases.append(pt)
                rows.append(sum((r16_rep(c, rng, kind) for c in v), []))
        for which in range(4):          # each row in turn at the tight bound
            cases.append(pt)
            rows.append(sum(p3_bound16(pt, rng, which, lx)[0], []))
    return cases, rows


def ge16_add_rows(rng, neg):
    cases, rows = [], []
    for a, b in pairs():
        for z1, z2 in list(zip(zs(rng), reversed(zs(rng))))[:3]:
            for kind in (0, 1):
                cases.append((a, b))
                rows.append(([r16_rep(c, rng, 2) for c in p3_vals(a, z1)], qc16(b, z2, rng, kind)))
        for which in range(4):          # P with each row in turn at the tight bound, qc formed from such a p3
            cases.append((a, b))
            rows.append((p3_bound16(a, rng, which)[0], qc16(b, 1, rng, 2 if which % 2 else 1)))
    out = []
    for p, q in rows:
        if neg:     # the loop hands -P as 4p - tight in rows 0 and 3 (ge16_cneg4)
            p = [[o - x for o, x in zip(P4, p[0])], p[1], p[2], [o - x for o, x in zip(P4, p[3])]]
        out.append(sum(p, []) + sum(q, []))
    return cases, out


def ge16_qc_rows(rng):
    cases, rows = [], []
    for pt in singles():
        for z in zs(rng):
            cases.append((pt, z))
            rows.append(sum((r16_rep(c, rng, 2) for c in p3_vals(pt, z)), []))
        for which in range(4):
            r, z = p3_bound16(pt, rng, which)
            cases.append((pt, z))
            rows.append(sum(r, []))
    return cases, rows


def test_ge16_dbl2(diag):
    rng = random.Random(80)
    for op, lx, want_t in (("dbl2_ff", False, False), ("dbl2_tf", True, False), ("dbl2_tt", True, True)):
        cases, rows = ge16_dbl_rows(rng, lx)
        rows.append([du.R16_TIGHT] * 64)     # every limb at the tight bound (no point: the output bound only)
        out = diag.run("ge16", op, rows)
        assert_r16_tight(out[-1], op)
        for pt, o in zip(cases, out):
            v = r16_vals(o)
            assert affine_p3(v, want_t) == du.ed_dbl(pt), (op, pt)
            if not want_t:
                assert v[3] == v[0], (op, pt)
            assert_r16_tight(o, (op, pt))
        print(f"ge16_{op}: {len(rows)} cases")


def test_ge16_add2_and_to_qc(diag):
    rng = random.Random(81)
    for op, want_t, neg in (("add2_t", True, False), ("add2_t_neg", True, True), ("add2_f", False, False),
                            ("add2_f_neg", False, True)):
        cases, rows = ge16_add_rows(rng, neg)
        out = diag.run("ge16", op, rows)
        for (a, b), o in zip(cases, out):
            v = r16_vals(o)
            # neg: given -a (rows 0 and 3 hold -X, -T) the step returns a - b (fd25519_r16.h:215-221)
            want = du.ed_add(a, du.ed_neg(b)) if neg else du.ed_add(a, b)
            assert affine_p3(v, want_t) == want, (op, a, b)
            if not want_t:
                assert v[3] == v[0], (op, a, b)
            assert_r16_tight(o, (op, a, b))
        print(f"ge16_{op}: {len(rows)} cases")
    cases, rows = ge16_qc_rows(rng)
    out = diag.run("ge16", "to_qc", rows)
    for (pt, z), o in zip(cases, out):
        c = cached_vals(pt, z)
        assert r16_vals(o) == [c[1], c[0], c[3], c[2]], (pt, z)
        assert max(int(v) for v in o) < 2**18, (pt, z)                 # fd25519_r16.h:377 "< 2^18"
    print(f"ge16_to_qc: {len(rows)} cases")


# ---- the three forms of one step agree ---------------------------------------------

def test_forms_agree(diag):
    rng = random.Random(82)
    ps = pairs()
    z1, z2 = rng.randrange(1, P), rng.randrange(1, P)
    tight = [(mk(p3_vals(a, z1), (rep_tight,) * 4, rng), mk(p3_vals(b, z2), (rep_tight,) * 4, rng)) for a, b in ps]
    # doubling
    o1 = diag.run("ge", "p2_dbl", [sum(p, []) for p, _ in tight])
    o4 = diag.run("ge4", "dbl", [sum(p, []) for p, _ in tight])
    o16 = diag.run("ge16", "dbl2_ff", [sum((r16_rep(c, rng, 2) for c in p3_vals(a, z1)), []) for a, _ in ps])
    for (a, _), x1, x4, x16 in zip(ps, o1, o4, o16):
        assert affine_p1p1(val4(x1)) == affine_p1p1(val4(x4)) == affine_p3(r16_vals(x16), False) == du.ed_dbl(a), a
    # addition
    o1 = diag.run("ge", "add", [sum(p + mk(cached_vals(b, z2), (rep_tight,) * 4, rng), []) for (p, _), (_, b) in zip(tight, ps)])
    o4 = diag.run("ge4", "add", [sum(p + qc_limbs(q), []) for p, q in tight])
    o16 = diag.run("ge16", "add2_t", [sum((r16_rep(c, rng, 2) for c in p3_vals(a, z1)), []) + sum(qc16(b, z2, rng, 1), [])
                                      for a, b in ps])
    for (a, b), x1, x4, x16 in zip(ps, o1, o4, o16):
        assert affine_p1p1(val4(x1)) == affine_p1p1(val4(x4)) == affine_p3(r16_vals(x16)) == du.ed_add(a, b), (a, b)
    print(f"forms agree: {2 * len(ps)} cases in three forms")
