"""The one-lane dsm loop's joint lane table on chosen digit pairs: the
product's dsm phase alone (Engine.diag_dsm) on one batch of crafted
half-size cases, every code compared with the discrete-logarithm model
(dsm_model.case_expect).  Exact.

The loop reads c and |d| in signed 2-bit windows and adds, per window, the
entry of the pair's class (tests/dsm_joint_model.py).  For every class the
recoding can produce, (c, d) is written digit by digit so that the class
sits in a chosen window -- the top one, one that holds both base digits,
one that holds a single base digit (60 with the wide tables, 56 with the
compact ones; the other then holds none), one that holds none, and window
0 -- and R is solved so that the sum is the identity: SUCCESS; the same
scalars with that one digit pair moved to a neighbouring class must give
ERR_MSG.  These lanes all run 66 windows and fill waves of their own (so
"top" is the loop's first window); the last waves mix lanes of 67..76
windows with 66-window lanes, runs of zero digit pairs (the shared identity
entry, also as the top window's entry), and lanes whose code the checks
before the equation decide."""
import random

import numpy as np
import pytest

import dsm_joint_model as jm
import dsm_model as dm
from diag_util import L

pytestmark = pytest.mark.gpu

MAX_CHUNK = 8192
TOP = jm.W2_MIN - 1
WINDOWS = (TOP, 60, 56, 24, 5, 0)   # top; one base digit (wide / compact); both; none; window 0


def value(digits):
    """most significant first"""
    v = 0
    for e in digits:
        v = 4 * v + e
    return v


def usable(cdig, ddig):
    """the digit strings are the recoding of a c < 2^131 and a |d| > 0 that asks for 66 windows"""
    c, d = value(cdig), value(ddig)
    return 0 <= c < 2**131 and 0 < d and jm.w2_of(d) == jm.W2_MIN and jm.digits2(c, 66) == cdig and \
        jm.digits2(d, 66) == ddig


def pairs_of(cls, top):
    """the digit pairs of a class: +-(a', r') within the digits' range"""
    lo, hi = (0, 2) if top else (-2, 1)
    return [(a, r) for a, r in (cls, (-cls[0], -cls[1])) if lo <= a <= hi and lo <= r <= hi]


def placements(rng):
    """[(class, window, c digits, d digits, [neighbour digit strings])]"""
    out = []
    for cls, where in sorted(jm.possible_classes().items()):
        if cls == (0, 0):
            continue
        for w in WINDOWS:
            top = w == TOP
            if top and "top" not in where:
                continue
            for _ in range(200):
                cdig = [rng.randrange(0, 2)] + [rng.randrange(-2, 2) for _ in range(65)]
                ddig = [rng.randrange(0, 2)] + [rng.randrange(-2, 2) for _ in range(64)] + [rng.choice((-1, 1))]
                a, r = rng.choice(pairs_of(cls, top))
                cdig[TOP - w], ddig[TOP - w] = a, r
                if usable(cdig, ddig):
                    break
            else:
                raise AssertionError((cls, w))
            assert jm.windows(value(cdig), value(ddig))[TOP - w][1:] == cls
            near = []
            for a2, r2 in ((a + 1, r), (a - 1, r), (a, r + 1), (a, r - 1)):
                c2, d2 = list(cdig), list(ddig)
                c2[TOP - w], d2[TOP - w] = a2, r2
                lo, hi = (0, 2) if top else (-2, 1)
                if lo <= a2 <= hi and lo <= r2 <= hi and usable(c2, d2):
                    assert jm.windows(value(c2), value(d2))[TOP - w][1:] != cls
                    near.append((c2, d2))
            assert near
            out.append((cls, w, cdig, ddig, near))
    return out


def solved(rng, c, d, **kw):
    """a case whose sum is the identity: r (and R's torsion part) solved"""
    A = (rng.randrange(1, L), rng.randrange(8))
    tr = dm.solve_tr(c, d, A[1])
    if tr is None:
        A, tr = (A[0], 0), 0
    sp = rng.randrange(L)
    return dm.half_case(c, d, sp, A, (dm.solve_r(c, d, sp, A), tr), **kw)


def build_batch():
    rng = random.Random(12)
    cases, kinds = [], []

    def emit(cs, kind):
        cases.append(cs)
        kinds.append(kind)

    # 1. every class in every kind of window, with its neighbours: 66-window lanes only
    for i, (cls, w, cdig, ddig, near) in enumerate(placements(rng)):
        sign = 1 if i % 2 else -1   # HF_DNEG set and clear
        v = solved(rng, value(cdig), sign * value(ddig))
        emit(v, ("class", cls, w))
        for c2, d2 in near:
            emit(dm.half_case(value(c2), sign * value(d2), v["sp"], v["A"], v["R"]), ("near", cls, w))
    while len(cases) % 64:   # whole waves of 66-window lanes
        emit(solved(rng, rng.getrandbits(131), (rng.getrandbits(130) | 1) * rng.choice((1, -1))), ("fill",))
    head = len(cases)
    # 2. longer |d|: every window count 67..76, each among 66-window lanes
    for w2 in range(jm.W2_MIN + 1, jm.W2_MAX + 1):
        for dmag in ((1 << (2 * w2 - 3)) | 1, (1 << (2 * w2 - 1)) - 1):
            if dmag.bit_length() > 151:
                dmag = (1 << 151) - 1
            assert jm.w2_of(dmag) == w2
            sign = rng.choice((1, -1))
            v = solved(rng, rng.getrandbits(131), sign * dmag)
            emit(v, ("long", w2))
            emit(dm.half_case(v["c"], -sign * dmag, v["sp"], v["A"], v["R"], dneg=int(sign > 0)), ("long-sign", w2))
        emit(solved(rng, rng.getrandbits(131), (rng.getrandbits(131) | 1) * rng.choice((1, -1))), ("short",))
    # 3. runs of zero digit pairs: the identity entry, in the top window too
    for c, d in ((0, 1), (1, 1), (0, -1), (1, -(2**130) - 1), (2**130, 2**130 + 1), (1 << 64, -(1 << 64) - 1),
                 (2**131 - 1, 1), (0, 2**150 + 1), (5 << 120, 3 << 40 | 1)):
        v = solved(rng, c, d)
        emit(v, ("zeros",))
        emit(dm.half_case(c, d, (v["sp"] + 1) % L, v["A"], v["R"]), ("zeros-sp",))
    # 4. lanes decided before the equation, over an identity and a non-identity sum
    ok = cases[0]
    bad = dict(ok, sp=(ok["sp"] + 1) % L)
    for base in (ok, bad):
        for sflag, af, rf in ((0, 0, 0), (1, 1, 0), (1, 0, 1), (1, 2, 0), (1, 0, 2), (1, 3, 3), (0, 1, 2)):
            emit(dict(base, sflag=sflag, af=af, rf=rf), ("pre",))
    return cases, kinds, head


@pytest.fixture(scope="module")
def batch():
    cases, kinds, head = build_batch()
    assert len(cases) <= 512 and head % 64 == 0
    return dict(cases=cases, kinds=kinds, head=head, arrays=dm.pack_nonsplit(cases))


@pytest.mark.parametrize("codes", ["avx512", "portable"])
@pytest.mark.parametrize("tables", ["wide", "compact"])
def test_joint_table_classes(batch, tables, codes):
    from firedancer_amd import ed25519
    cases, kinds, a = batch["cases"], batch["kinds"], batch["arrays"]
    exp = np.array([dm.case_expect(c, codes == "portable") for c in cases], np.int8)
    # what the batch holds, before it is run
    for cs, kd, e in zip(cases, kinds, exp):
        if kd[0] in ("class", "long", "short", "zeros", "fill"):
            assert e == dm.SUCCESS, (kd, cs)
        elif kd[0] in ("near", "long-sign", "zeros-sp"):
            assert e == dm.ERR_MSG, (kd, cs)
        if kd[0] in ("class", "near", "fill"):
            assert jm.w2_of(cs["dm"]) == jm.W2_MIN
    placed = {(kd[1], kd[2]) for kd in kinds if kd[0] == "class"}
    classes = {c: w for c, w in jm.possible_classes().items() if c != (0, 0)}
    assert placed == {(c, w) for c, where in classes.items() for w in WINDOWS if w != TOP or "top" in where}
    assert {kd[1] for kd in kinds if kd[0] == "long"} == set(range(67, 77))
    assert {cs["dneg"] for cs, kd in zip(cases, kinds) if kd[0] == "class"} == {0, 1}
    assert set(exp[[kd[0] == "pre" for kd in kinds]].tolist()) >= {dm.ERR_SIG, dm.ERR_PUBKEY}
    eng = ed25519.Engine(0, max_chunk=MAX_CHUNK, dsm="wide", compact=tables == "compact", codes=codes)
    try:
        got = eng.diag_dsm(dm.FORMS["wide"], a["sflag"], a["hflag"], a["pflag"], a["pts"], a["hs"], a["k"], a["S"])
    finally:
        eng.close()
    bad = np.nonzero(got != exp)[0]
    assert not len(bad), (len(bad), len(exp), [(int(i), kinds[i], int(got[i]), int(exp[i]), cases[i]) for i in bad[:4]])
