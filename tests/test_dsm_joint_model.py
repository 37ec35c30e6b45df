"""The joint 12-slot lane table over 2-bit windows (dsm_half_one), without a
GPU: the recoding, class, slot and sign restated in Python integers
(tests/dsm_joint_model.py) give [c]A' + [|d|]R' in dsm_model's group
arithmetic; every slot is in 0..11; the classes the recoding can produce
are the ones the device builds; and, over integer intervals
(tests/bounds_model.py), every new table entry has its stated bound and
every new product's operands and sums fit int32 / int64."""
import os
import random
import re

import pytest

import bounds_model as bm
import dsm_joint_model as jm
import dsm_model as dm
from diag_util import L

KERNELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "firedancer_amd", "csrc",
                       "fd_ed25519_kernels.hip")


def pat4(digit, n):
    """the base-4 digit repeated n times"""
    return sum(digit << (2 * i) for i in range(n))


C_EDGE = [0, 1, 2**131 - 1]
D_EDGE = [1, 2**130 - 1, 2**130 + 1, 2**131, 2**150 + 1]
D_LENGTHS = [v for b in range(129, 152) for v in ((1 << (b - 1)) | 1, (1 << b) - 1)]
# digit strings that carry through every window: 3 -> -1 carry 1, 2 -> -2 carry 1
CARRY = [pat4(3, 65) + (1 << 130), pat4(2, 65), pat4(2, 65) | 1, pat4(3, 64) << 2, (pat4(2, 64) << 2) | 3]


def scalar_pairs():
    rng = random.Random(5)
    out = [(c, d) for c in C_EDGE for d in D_EDGE]
    out += [(rng.getrandbits(131), d) for d in D_LENGTHS]
    out += [(c, d) for c in CARRY for d in CARRY if d % 2] + [(c, pat4(3, 75) >> 1) for c in CARRY]
    out += [(rng.getrandbits(131), rng.getrandbits(rng.choice((131, 131, 151))) | 1) for _ in range(60)]
    return out


def test_digits_are_the_scalar_and_in_range():
    for c, d in scalar_pairs():
        w2 = jm.w2_of(d)
        assert w2 == max(66, -(-(d.bit_length() + 1) // 2)) and 66 <= w2 <= 76
        for x in (c, d):
            for w in {w2, 76}:   # a lane of a wave whose longest |d| asks for more windows
                dg = jm.digits2(x, w)
                assert len(dg) == w and 0 <= dg[0] <= 2 and all(-2 <= e <= 1 for e in dg[1:])
                assert sum(e << (2 * (w - 1 - i)) for i, e in enumerate(dg)) == x
    assert jm.w2_of(2**131 - 1) == 66 and jm.w2_of(2**131) == 67 and jm.w2_of(2**151 - 1) == 76


def test_joint_sum_is_the_double_scalar_product():
    rng = random.Random(6)
    pts = [dm.dl_point(rng.randrange(1, L), t) for t in (0, 3, 4, 7)] + [dm.dl_point(1, 0), dm.dl_point(0, 1)]
    for i, (c, d) in enumerate(scalar_pairs()):
        A1 = dm.xneg(dm.xpt(pts[i % len(pts)]))
        R1 = dm.xpt(pts[(i // 2 + 1) % len(pts)])
        R1 = dm.xneg(R1) if i % 3 else R1
        want = dm.xaffine(dm.xmul2(c, A1, d, R1))
        assert dm.xaffine(jm.joint_sum(c, d, A1, R1)) == want, (c, d)
        if i % 5 == 0:   # ... in a wave that runs more windows than this lane needs
            assert dm.xaffine(jm.joint_sum(c, d, A1, R1, 76)) == want, (c, d)


def test_slots_and_reachable_classes():
    """every lookup is slot 0..11 (or the identity); the classes met by
    real recodings are exactly those the digit ranges admit -- all but
    (2, -2) -- and the device builds exactly their slots"""
    admit = jm.possible_classes()
    assert set(admit) == {(a, r) for a in range(3) for r in range(-2, 3) if (a, r) > (0, -1)} - {(2, -2)}
    seen = {}
    rng = random.Random(8)
    pairs = scalar_pairs() + [(rng.getrandbits(131), rng.getrandbits(131) | 1) for _ in range(300)]
    pairs += [(2**131 - 1 - rng.getrandbits(120), 2**131 - 1 - 2 * rng.getrandbits(120)) for _ in range(200)]
    for c, d in pairs:
        for i, (s, a, r) in enumerate(jm.windows(c, d)):
            assert (a, r) == (0, 0) or 0 <= jm.slot(a, r) <= 11
            assert s in (0, 1) and (a, r) >= (0, 0)
            seen.setdefault((a, r), set()).add("top" if i == 0 else "low")
    assert seen == admit, (seen, admit)
    reachable = {jm.slot(a, r) for (a, r) in admit if (a, r) != (0, 0)}
    assert reachable == set(range(12)) - {jm.slot(2, -2)}
    assert set(jm.build_table(dm.XIDENT, dm.XIDENT)) == reachable
    src = open(KERNELS).read()
    body = src[src.index("void joint_table_build("):src.index("const int4* jtab_entry(")]
    built = {jm.slot(int(a), int(r)) for a, r in re.findall(r"FD_JSLOT\((\d), (-?\d)\)", body)}
    assert built == reachable, sorted(built)


# ---- bounds ---------------------------------------------------------------------

def _within(f, lo_mult, hi_mult):
    for k, (lo, hi) in enumerate(f):
        unit = 1 << (bm.W[k] - 1)
        assert lo >= lo_mult * unit and hi <= hi_mult * unit, (k, lo / unit, hi / unit)


ONE = bm.fe_const([1] + [0] * 9)


def _affine():
    """jtab_affine and its entry: (the point, the stored entry)"""
    x = bm.fe_cneg(bm.decoded_x())
    P = {"X": x, "Y": bm.frombytes(), "Z": ONE, "T": bm.fe_mul(x, bm.frombytes())}
    c1 = bm.p3_to_cached(P, False)
    return P, dict(c1, T2d=bm.fe_neg(c1["T2d"]))


def _stored(P, neg=False):
    """jtab_store: the entry of P, or of -P"""
    c = bm.p3_to_cached(P, True)
    c = dict(c, T2d=bm.fe_neg(c["T2d"]))
    return dict(c, YplusX=c["YminusX"], YminusX=c["YplusX"], T2d=bm.fe_neg(c["T2d"])) if neg else c


def _step(e, q, mneg=False):
    """jtab_step: the entries of E + q and of E - q (mneg: of q - E)"""
    qs, qd = bm.fe_add(q["Y"], q["X"]), bm.fe_sub(q["Y"], q["X"])
    m = bm.fe_mul(e["T2d"], q["T"])
    out = []
    for plus in (False, True):
        u, v = (qs, qd) if plus else (qd, qs)
        a, b = bm.fe_mul_u(e["YplusX"], u), bm.fe_mul_u(e["YminusX"], v)
        ms = m if plus else bm.fe_neg(m)
        s = {"X": bm.fe_sub(a, b), "Y": bm.fe_add(a, b), "Z": bm.fe_sub(e["Z2"], ms), "T": bm.fe_add(e["Z2"], ms)}
        for k in "XZT":   # the completed point's stated bounds (fd25519_ge.h): the conversions' 19-sides
            _within(s[k], -3.04, 3.04)
        _within(s["Y"], -1.01, 4.02)
        out.append(_stored(bm.p1p1_to_p3(s, True, False), mneg and not plus))
    return out[1], out[0]


def joint_entries():
    """joint_table_build over intervals: (the affine entries, the others)"""
    A1, eA = _affine()
    R1, eR = _affine()
    A2 = _stored(bm.p1p1_to_p3(bm.p2_dbl(A1), True, False))
    R2 = _stored(bm.p1p1_to_p3(bm.p2_dbl(R1), True, False))
    new = [A2, R2]
    new += _step(R2, A1, True)
    new += _step(eA, R1)
    p, m = _step(A2, R1)
    new += [p, m, _step(p, R1)[0]]
    return [eA, eR], new


def test_entry_bounds():
    """the affine entries are table_build's first one; every other entry
    has Y+X - p, Y-X within 2.02x, 2Z within 2.02x, -+2dT within 2x"""
    affine, new = joint_entries()
    for e in affine:
        _within(e["YplusX"], -1.01, 3.01)
        _within(e["YminusX"], -1.01, 3.01)
        _within(e["T2d"], -2.001, 0.001)
    assert len(new) == 9
    for e in new:
        _within(e["YplusX"], -2.02, 2.02)
        _within(e["YminusX"], -2.02, 2.02)
        _within(e["Z2"], -2.02, 2.02)
        _within(e["T2d"], -2.001, 2.001)


def joint_loop(max_iter=8):
    """the loop over intervals, fed its own outputs until they stop growing:
    the top window's point taken from its entry, two doublings, one
    addition, the base additions, and the identity test's difference on the
    completed point"""
    affine, new = joint_entries()
    ident = {"YplusX": ONE, "YminusX": ONE, "Z2": bm.fe_const([2] + [0] * 9), "T2d": bm.fe_const([0] * 10)}
    tab = ident
    for e in affine + new:
        tab = bm.ge_hull_c(tab, e)
    tab = bm.cached_cneg(tab)
    bt = bm.base_entry()
    Q = {"X": bm.fe_carry(bm.fe_sub(tab["YplusX"], tab["YminusX"])),
         "Y": bm.fe_carry(bm.fe_add(tab["YplusX"], tab["YminusX"])), "Z": tab["Z2"]}
    for it in range(max_iter):
        P = bm.p1p1_to_p3(bm.p2_dbl(bm.p1p1_to_p2(bm.p2_dbl(Q))), True, True)
        Rt = bm.ge_add(P, tab, True)
        Rb = bm.ge_madd(bm.p1p1_to_p3(Rt, True, False), bt)
        Rb = bm.ge_madd(bm.p1p1_to_p3(Rb, True, False), bt)
        Rt = {k: bm.fe_hull(Rt[k], Rb[k]) for k in Rt}
        bm.fe_carry(Rt["X"])
        bm.fe_carry(bm.fe_sub(Rt["Y"], Rt["T"]))
        Qn = {k: bm.fe_hull(Q[k], v) for k, v in bm.p1p1_to_p2(Rt).items()}
        if Qn == Q:
            return Q, it
        Q = Qn
    return Q, max_iter


def test_loop_fixed_point():
    Q, iters = joint_loop()
    assert iters < 8, "intervals did not converge"
    for k in "XY":
        _within(Q[k], -1.01, 2.001)
    _within(Q["Z"], -2.02, 2.02)


def test_uncarried_top_point_would_overflow_nothing_but_exceeds_the_doubling_bound():
    """why the top window's X and Y are carried: the raw sums reach 4x,
    beyond the 2x ge_p2_dbl states for its input"""
    _, new = joint_entries()
    raw = bm.fe_add(new[0]["YplusX"], new[0]["YminusX"])
    with pytest.raises(AssertionError):
        _within(raw, -2.02, 2.02)
    _within(bm.fe_carry(raw), -1.01, 1.01)
