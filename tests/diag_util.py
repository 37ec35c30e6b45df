"""Loader for the test-only diagnostic library
(firedancer_amd/csrc/diag/fd_ed25519_diag.hip -> _lib/libfd_ed25519_diag.so)
and the exact references its tests compare with: integers mod p and mod L,
affine Edwards arithmetic, limb <-> value conversion for the one-lane
radix-2^25.5 form and the lane-split radix-2^16 form, and the operand
classes (limb vectors at the documented bounds, special values in several
representations, scalar edge lists).  Test infrastructure, no product code.

Everything here is exact: Python integers, no tolerances."""
import ctypes
import os

import numpy as np

import bounds_model as bm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# $FD_ED25519_DIAG_LIB: another build of the unit (as $FD_ED25519_HIP_LIB for the product), e.g. one
# over deliberately broken copies of the headers, to see the tests fail
DIAG_LIB = os.environ.get("FD_ED25519_DIAG_LIB",
                          os.path.join(REPO, "firedancer_amd", "_lib", "libfd_ed25519_diag.so"))

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = (-121665 * pow(121666, P - 2, P)) % P
D2 = 2 * D % P
SQRTM1 = pow(2, (P - 1) // 4, P)

# the op numbers of fd_ed25519_diag.hip's enums, in order
FE_OPS = ("mul", "mul19", "sq", "sq2", "mul_u", "sq_u", "sq2_u", "carry", "ident", "frombytes", "pow22523",
          "invert", "sq_sh")
R16_OPS = ("mul", "sq", "ident", "from_fe", "pow22523")
SC_OPS = ("reduce512", "is_canonical", "recode16", "recode256", "recode65536")
GE_OPS = ("p2_dbl", "p3_dbl", "add", "add_nt", "madd", "to_cached", "to_cached_uxy", "p1p1_to_p2", "p1p1_to_p3",
          "p1p1_to_p3_u", "p1p1_to_p3_uxyt", "cached_cneg", "precomp_cneg")
GE4_OPS = ("dbl", "add", "to_p3", "to_qc", "cneg_p3", "cneg_p1p1")
GE16_OPS = ("dbl2_ff", "dbl2_tf", "dbl2_tt", "add2_t", "add2_t_neg", "add2_f", "add2_f_neg", "to_qc")
FAMILIES = {  # family -> (ops, words in per case, words out per case)
    "fe": (FE_OPS, 20, 20), "r16": (R16_OPS, 32, 32), "sc": (SC_OPS, 16, 64), "digits160": (("digits",), 11, 80),
    "ge": (GE_OPS, 80, 40), "ge4": (GE4_OPS, 80, 40), "ge16": (GE16_OPS, 128, 64),
}
HIP_ERROR_INVALID_VALUE = 1


class Diag:
    """run(family, op, rows): rows is a list of per-case word lists (signed
    or unsigned 32-bit values, shorter rows are zero-padded); returns an
    (n, words out) array of int64 holding the unsigned 32-bit words."""

    def __init__(self, path=DIAG_LIB):
        self.lib = ctypes.CDLL(path)   # a missing library is an error, not a skip
        for fam in FAMILIES:
            f = getattr(self.lib, "fd_ed25519_diag_" + fam)
            f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulong]
            f.restype = ctypes.c_int

    def raw(self, family, opnum, inp, out, n):
        return getattr(self.lib, "fd_ed25519_diag_" + family)(int(opnum), inp.ctypes.data, out.ctypes.data, int(n))

    def run(self, family, op, rows):
        ops, win, wout = FAMILIES[family]
        n = len(rows)
        inp = np.zeros((max(n, 1), win), dtype=np.uint32)
        for i, r in enumerate(rows):
            assert len(r) <= win
            inp[i, :len(r)] = [int(v) & 0xffffffff for v in r]
        out = np.zeros((max(n, 1), wout), dtype=np.uint32)
        rc = self.raw(family, ops.index(op), inp, out, n)
        assert rc == 0, f"fd_ed25519_diag_{family}({op}) returned HIP error {rc}"
        return out[:n].astype(np.int64)


def s32(v):
    """an unsigned 32-bit word read as the int32 the device holds"""
    v = int(v)
    return v - (1 << 32) if v >= (1 << 31) else v


def words(v, n):
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def from_words(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


# ---- radix 2^25.5 ------------------------------------------------------------

W = bm.W
OFF = [sum(W[:i]) for i in range(10)]          # 0, 26, 51, 77, 102, 128, 153, 179, 204, 230


def fe_int(limbs):
    """the integer a limb vector stands for (not reduced)"""
    return sum(int(l) << OFF[i] for i, l in enumerate(limbs))


def fe_val(limbs):
    return fe_int(limbs) % P


def bound(mult):
    """limb magnitudes of `mult` units (2^25 even limbs, 2^24 odd limbs)"""
    return [int(mult * (1 << (w - 1))) for w in W]


B33 = bound(3.3)       # fd25519_fe.h:22 "mul/sq accept inputs <= 3.3x"
TIGHT = bound(1.01)    # fd25519_fe.h:19 "tight ... <= 1.01x"


def within(limbs, lo, hi):
    return all(a <= int(l) <= b for l, a, b in zip(limbs, lo, hi))


def fe_digits(v):
    """plain radix digits of an integer |v| < 1.6 * 2^255 (limb 9 takes what
    is left above bit 230), negated as a whole for v < 0: the integer is v"""
    s, v = (-1, -v) if v < 0 else (1, v)
    out = []
    for i in range(9):
        out.append(s * (v & ((1 << W[i]) - 1)))
        v >>= W[i]
    return out + [s * v]


def fe_centered(v, fold=True):
    """centered digits (limb i in [-2^(w-1), 2^(w-1))); the carry out of limb
    9 is folded into limb 0 as 19 (fold: the value mod p stays, the integer
    moves by a multiple of p) or left in limb 9 (the integer stays)"""
    out = []
    for i in range(10):
        if i == 9 and not fold:
            out.append(v)
            return out
        h = 1 << (W[i] - 1)
        d = ((v + h) % (1 << W[i])) - h
        out.append(d)
        v = (v - d) >> W[i]
    out[0] += 19 * v
    return out


def fe_zero_vectors():
    """limb vectors that stand for 0: (2^w at limb i, -1 at limb i+1), and the
    wrap (2^25 at limb 9, -19 at limb 0) which stands for p"""
    out = []
    for i in range(9):
        z = [0] * 10
        z[i], z[i + 1] = 1 << W[i], -1
        out.append(z)
    z = [0] * 10
    z[9], z[0] = 1 << 25, -19
    out.append(z)
    return out


def fe_reps(v, bnd):
    """representations of the integer v (or, where a fold or the wrap vector
    is used, of v mod p) whose limbs lie within +-bnd: plain digits, centered
    digits (unfolded and folded), and each of those plus / minus a vector
    that stands for 0.  Only what fits the bound is returned; the folded
    centered form always fits a tight bound."""
    base = [fe_digits(v), fe_centered(v, False), fe_centered(v, True)]
    out = []
    for b in base:
        cands = [b] + [[x + s * y for x, y in zip(b, z)] for z in fe_zero_vectors() for s in (1, -1)]
        for c in cands:
            if within(c, [-x for x in bnd], bnd) and c not in out:
                out.append(c)
    assert out and all(fe_val(c) == v % P for c in out)
    return out


FE_SPECIAL = [0, 1, 2, P - 1, P, P + 1, -P, -1, 2**255 - 1, 2**255 - 20, 2**255 - 18, 2**254, 2**254 - 1,
              P + 2**254, -(P + 2**254), 2 * P, (P - 1) // 2, (P + 1) // 2]
"""2p and the values above 1.65 * 2^255 cannot be held as integers by limbs
within 3.3x (their largest integer is about 1.65 * 2^255); fe_reps then gives
forms that stand for them mod p (the folded centered digits)."""


def fe_special_reps(bnd):
    out = []
    for v in FE_SPECIAL:
        if abs(v) < 3 * 2**254:
            out += fe_reps(v, bnd)
        else:
            c = fe_centered(v, True)
            assert within(c, [-x for x in bnd], bnd)
            out.append(c)
    return out


def fe_extremes(bnd, lo=None):
    """class (b): every limb at +bound, at -bound (or the lower bound `lo`),
    alternating, and one limb at either bound with the rest zero"""
    lo = [-x for x in bnd] if lo is None else lo
    out = [list(bnd), list(lo),
           [bnd[i] if i % 2 == 0 else lo[i] for i in range(10)],
           [lo[i] if i % 2 == 0 else bnd[i] for i in range(10)]]
    for i in range(10):
        for v in (bnd[i], lo[i]):
            if v:
                z = [0] * 10
                z[i] = v
                out.append(z)
    return out


def fe_random(rng, n, bnd, lo=None):
    lo = [-x for x in bnd] if lo is None else lo
    return [[rng.randint(lo[i], bnd[i]) for i in range(10)] for _ in range(n)]


def hull(vectors):
    """per-limb (min, max) of a class of limb vectors: bounds_model's input"""
    return [(min(int(v[i]) for v in vectors), max(int(v[i]) for v in vectors)) for i in range(len(vectors[0]))]


def point_iv(limbs):
    return [(int(l), int(l)) for l in limbs]


def inside(limbs, ivs):
    return all(lo <= int(l) <= hi for l, (lo, hi) in zip(limbs, ivs))


def canonical_words(v):
    return words(v % P, 8)


# ---- radix 2^16, 16 lanes ------------------------------------------------------

R16_IN = 2**19                    # fd25519_r16.h:29 "r16_mul / r16_sq take limbs < 2^19"
R16_TIGHT = 2**16 + 63            # the largest tight limb ("tight" = < 2^16 + 64)
# fd25519_r16.h:33-34: round 3 < 2^16 + 38 (lane 0), < 2^16 + 2^6 (lane 1), < 2^16 + 1 elsewhere
R16_OUT_MAX = [2**16 + 38, 2**16 + 2**6] + [2**16] * 14


def r16_int(limbs):
    return sum(int(l) << (16 * c) for c, l in enumerate(limbs))


def r16_val(limbs):
    return r16_int(limbs) % P


def r16_digits(v):
    """16-bit digits of an integer 0 <= v < 2^259; limb 15 takes the rest"""
    out = [(v >> (16 * c)) & 0xffff for c in range(15)]
    return out + [v >> 240]


def r16_splits(v, rng, n):
    """n limb vectors with every limb < 2^19 that stand for the integer v:
    the digits, then units moved down from a limb into the one below it"""
    base = r16_digits(v)
    assert max(base) < R16_IN
    out = [base]
    for _ in range(n - 1):
        l = list(base)
        for c in range(14, -1, -1):
            j = rng.randint(0, min(7 - (l[c] >> 16), l[c + 1]))
            l[c] += j << 16
            l[c + 1] -= j
        assert r16_int(l) == v and 0 <= min(l) and max(l) < R16_IN
        out.append(l)
    return out


def r16_random_tight(rng):
    """a tight limb vector (every limb < 2^16 + 64), each limb at the top of
    the range, just above 2^16, or anywhere"""
    return [rng.choice((R16_TIGHT, (1 << 16) + rng.randrange(64), rng.randrange(1 << 16), R16_TIGHT - rng.randrange(4)))
            for _ in range(16)]


def r16_at_bound(rng):
    """a tight limb vector that reaches the bound: lanes 0, 1 and 15 (the
    lanes whose carries differ: the 38 x wrap's target, its neighbour, and
    the top) exactly 2^16 + 63, the others tight at random -- or, one time in
    four, every lane at 2^16 + 63"""
    l = [R16_TIGHT] * 16 if rng.randrange(4) == 0 else r16_random_tight(rng)
    for c in (0, 1, 15):
        l[c] = R16_TIGHT
    assert r16_val(l) != 0
    return l


# ---- edwards25519, affine ------------------------------------------------------

def ed_add(a, b):
    (x1, y1), (x2, y2) = a, b
    t = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + x2 * y1) * pow(1 + t, P - 2, P) % P, (y1 * y2 + x1 * x2) * pow(1 - t, P - 2, P) % P)


def ed_dbl(a):
    """the doubling law on its own (2xy / (y^2 - x^2), (y^2 + x^2) / (2 - y^2 + x^2)), not ed_add(a, a)"""
    x, y = a
    xx, yy = x * x % P, y * y % P
    return (2 * x * y * pow(yy - xx, P - 2, P) % P, (yy + xx) * pow(2 - yy + xx, P - 2, P) % P)


def ed_neg(a):
    return ((-a[0]) % P, a[1])


def ed_mul(k, pt):
    r, q = (0, 1), pt
    while k:
        if k & 1:
            r = ed_add(r, q)
        q = ed_add(q, q)
        k >>= 1
    return r


def on_curve(a):
    x, y = a
    return (-x * x + y * y - 1 - D * x * x * y * y) % P == 0


def recover_x(y, sign=0):
    u, v = (y * y - 1) % P, (D * y * y + 1) % P
    x = u * pow(v, 3, P) * pow(u * pow(v, 7, P), (P - 5) // 8, P) % P
    if (v * x * x - u) % P:
        x = x * SQRTM1 % P
    assert (v * x * x - u) % P == 0
    return P - x if (x & 1) != sign else x


BY = 4 * pow(5, P - 2, P) % P
BASE = (recover_x(BY, 0), BY)
# the order-8 points' y (fd25519_dsm.h ge_decode, y0)
Y8 = from_words([0x8f95e826, 0xb027b2c2, 0x89f4c345, 0xf098eff2, 0x05acdfd5, 0x3933c6d3, 0x880238b1, 0x05fc536d])
IDENT = (0, 1)
ORDER2 = (0, P - 1)
ORDER4 = [(SQRTM1, 0), (P - SQRTM1, 0)]
ORDER8 = (recover_x(Y8, 0), Y8)
TORSION = [IDENT, ORDER2] + ORDER4 + [ORDER8]


def random_point(rng):
    return ed_mul(rng.randrange(1, L), BASE)


def point_pairs(rng, n_random=6):
    """operand pairs (P, Q) for an addition: random points, every torsion
    point, B; P with -P, P with P, P with P + torsion"""
    pts = [random_point(rng) for _ in range(n_random)]
    special = TORSION + [BASE]
    pairs = [(pts[i], pts[(i + 1) % n_random]) for i in range(n_random)]
    pairs += [(a, b) for a in special for b in special]
    pairs += [(pts[0], s) for s in special] + [(s, pts[1]) for s in special]
    for a in (pts[2], BASE, ORDER8):
        pairs += [(a, ed_neg(a)), (a, a)] + [(a, ed_add(a, t)) for t in TORSION[1:]]
    assert all(on_curve(a) and on_curve(b) for a, b in pairs)
    return pairs


# ---- scalars -------------------------------------------------------------------

def scalar_edges_512(rng, n_random=2000):
    """the inputs of sc_reduce512 / mod_l: below 2^512"""
    top = (2**512 - 1) // L
    xs = [0, 1, L - 1, L, L + 1, 2**252 - 1, 2**252, 2**253 - 1, 2**256 - 1, 2**483 - 1, 2**483 + 1, 2**511, 2**512 - 1]
    for m in (1, 2, 3, 7, 8, 2**32 - 1, 2**32, 2**33, 2**128, 2**200, 2**259, top):
        xs += [m * L - 1, m * L, m * L + 1]
    # residues in [2^252, L): digit 11 of the reduced value is exactly 2^21
    gap = L - 2**252
    for r in [2**252, 2**252 + 1, L - 1, L - 2, 2**252 + gap // 2] + [2**252 + rng.randrange(gap) for _ in range(40)]:
        xs += [r + m * L for m in (0, 1, 2, 2**31, 2**128 + 5, 2**200 - 1, top - 1)]
    # 21-bit digit patterns over all 24 digits
    def pat(d):
        return sum(d[i % len(d)] << (21 * i) for i in range(24)) & (2**512 - 1)
    ones = 2**21 - 1
    xs += [pat([ones]), pat([ones, 0]), pat([0, ones]), pat([2**20 - 1]), pat([2**20]), pat([2**20 + 1]),
           pat([2**20, 2**20 - 1]), pat([2**20 - 1, 2**20])]
    xs += [1 << b for b in range(512)] + [(2**512 - 1) ^ (1 << b) for b in range(512)]
    xs += [rng.getrandbits(512) for _ in range(n_random)] + [rng.getrandbits(406) for _ in range(n_random)]
    assert all(0 <= x < 2**512 for x in xs)
    return xs


def scalar_edges_lt_l(rng, n_random=300):
    """scalars below L for the recodings: the edge list restricted to < L,
    plus the nibble patterns that make every digit carry or sit at the edge"""
    xs = sorted({x for x in scalar_edges_512(rng, 0) if x < L})
    for nib in (0x8, 0x7, 0xf, 0x9, 0x80, 0x7f, 0x8000, 0x7fff):
        w = 4 if nib < 16 else 8 if nib < 256 else 16
        v = sum(nib << (w * i) for i in range(256 // w))
        xs += [v % (1 << b) for b in (252, 251, 248, 240)]
    xs += [rng.randrange(L) for _ in range(n_random)]
    assert all(0 <= x < L for x in xs)
    return xs
