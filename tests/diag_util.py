"""Loader for the test-only diagnostic library
(firedancer_amd/csrc/diag/fd_ed25519_diag.hip -> _lib/libfd_ed25519_diag.so)
and the exact references its tests compare with: integers mod p and mod L,
affine Edwards arithmetic, limb <-> value conversion for the one-lane
radix-2^25.5 form and the lane-split radix-2^16 form, and the operand
classes (limb vectors at the documented bounds, special values in several
representations, scalar edge lists); and for the hash family
(diag/fd_ed25519_diag_hash.hip) the byte-buffer layout, the case builders
and hashlib's digests in the word order the device returns; and the call
of the sign family (diag/fd_ed25519_diag_sign.hip), whose cases and model
are tests/sign_model.py's.  Test infrastructure, no product code.

Everything here is exact: Python integers, no tolerances."""
import ctypes
import hashlib
import os
import random

import numpy as np

import bounds_model as bm
import shred_model

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
# diag/fd_ed25519_diag_sign.hip: a family with one more argument, the signer's table (Diag.run_sign)
SIGN_OPS = ("base", "base_wide", "muladd", "encode")
SIGN_IN, SIGN_OUT = 32, 40
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
        self.lib.fd_ed25519_diag_hash.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_ulong, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_ulong]
        self.lib.fd_ed25519_diag_hash.restype = ctypes.c_int
        self.lib.fd_ed25519_diag_sign.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulong,
                                                  ctypes.c_void_p]
        self.lib.fd_ed25519_diag_sign.restype = ctypes.c_int

    def raw_sign(self, opnum, inp, out, n, btab):
        """fd_ed25519_diag_sign as it is: inp / out uint32 arrays, btab an int32 array or None; the HIP error code"""
        return self.lib.fd_ed25519_diag_sign(int(opnum), inp.ctypes.data, out.ctypes.data, int(n),
                                             None if btab is None else btab.ctypes.data)

    def run_sign(self, op, rows, btab=None):
        """run() for the sign family: btab is Engine.sign_table() (ops base and base_wide)"""
        n = len(rows)
        inp = np.zeros((max(n, 1), SIGN_IN), dtype=np.uint32)
        for i, r in enumerate(rows):
            assert len(r) <= SIGN_IN
            inp[i, :len(r)] = [int(v) & 0xffffffff for v in r]
        out = np.zeros((max(n, 1), SIGN_OUT), dtype=np.uint32)
        if btab is not None:
            btab = np.ascontiguousarray(btab, dtype=np.int32)
            assert btab.size == 129 * 36
        rc = self.raw_sign(SIGN_OPS.index(op), inp, out, n, btab)
        assert rc == 0, f"fd_ed25519_diag_sign({op}) returned HIP error {rc}"
        return out[:n].astype(np.int64)

    def raw_hash(self, opnum, buf, inp, out, n, buf_sz=None):
        """fd_ed25519_diag_hash as it is: buf a uint8 array, inp / out uint32 arrays; the HIP error code"""
        return self.lib.fd_ed25519_diag_hash(int(opnum), buf.ctypes.data, len(buf) if buf_sz is None else int(buf_sz),
                                             inp.ctypes.data, out.ctypes.data, int(n))

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


# ---- the hash family (diag/fd_ed25519_diag_hash.hip) ---------------------------

# the op numbers of fd_ed25519_diag_hash.hip's enum, in order
HASH_OPS = ("sha512_pre8", "sha512_ram", "sha512_ram_2w", "sha256_bytes", "sha256_leaf", "sha256_node",
            "sha256_node_pair")
HASH_IN, HASH_OUT = 24, 16
HASH_PAD = 16                      # filler bytes in front of and behind every message
HASH_MAX_N, HASH_MAX_BUF = 1 << 20, 1 << 28
HIP_ERROR_UNKNOWN = 999            # the entry point's "a lane past n stored"
LEAF_PREFIX, NODE_PREFIX = shred_model.LEAF, shred_model.NODE
SHA512_OPS = {"sha512_pre8": 32, "sha512_ram": 64, "sha512_ram_2w": 64}     # op -> prefix bytes
SHA512_SIZES = list(range(601)) + [1232, 1233, 65535, 65536, 65537]
LEAF_REAL_SIZES = [1115 - 20 * d + x for d in range(16) for x in (0x18, 0x19)]   # fd_shred_core.h: P


def hash_per_block(op):
    """cases a block serves: case i is lane i % per of block i // per"""
    return 32 if op == "sha512_ram_2w" else 64


def sha512_blocks(total):
    """FIPS 180-4 5.1.2: 0x80, zeros, 128-bit length"""
    return (total + 17 + 127) // 128


def sha256_blocks(total):
    """FIPS 180-4 5.1.1: 0x80, zeros, 64-bit length"""
    return (total + 9 + 63) // 64


def sha512_full_blocks(pre, sz):
    """blocks of prefix || message that are message bytes from end to end"""
    return sum(1 for b in range(sha512_blocks(pre + sz)) if 128 * b >= pre and 128 * b + 128 <= pre + sz)


class HashBuf:
    """The byte buffer of one launch: every message is placed at the next
    offset of the wanted byte shift (offset % 4; the device allocation is
    256-byte aligned) with at least `lead` bytes of filler in front of it and
    HASH_PAD behind, so the bytes next to a message are never another
    case's.  `spans` records (start, end) of every message."""

    def __init__(self):
        self.parts, self.end, self.spans = [], 0, []

    def place(self, data, shift, lead=HASH_PAD):
        off = self.end + lead
        off += (shift - off) % 4
        self.parts.append((off, bytes(data)))
        self.spans.append((off, off + len(data)))
        self.end = off + len(data)
        return off

    def size(self):
        return self.end + HASH_PAD

    def bytes(self, filler):
        buf = np.full(self.size(), filler, np.uint8)
        for off, data in self.parts:
            buf[off:off + len(data)] = np.frombuffer(data, np.uint8)
        return buf


def le_words(b):
    return [int(x) for x in np.frombuffer(b, "<u4")]


def be_words(b):
    return [int(x) for x in np.frombuffer(b, ">u4")]


def hash_case(op, off, sz, shift, want, opnd=(), flag=0, note=""):
    """want: the 16 (SHA-512, little-endian) or 8 (SHA-256, big-endian)
    words the device returns for the reference digest"""
    assert off % 4 == shift or op == "sha256_node_pair"
    return dict(op=op, off=off, sz=sz, shift=shift, flag=flag, opnd=list(opnd), want=want, note=note)


def hash_bounds_ok(c, buf_sz):
    """the entry point's own rule: the bytes a case reads lie inside [0, buf_sz)"""
    op, off, sz = c["op"], c["off"], c["sz"]
    if op in SHA512_OPS:
        return off + sz <= buf_sz
    if op == "sha256_bytes":
        return sz >= 1 and off + sz <= buf_sz
    if op == "sha256_leaf":
        return sz >= 38 and off + 64 + sz <= buf_sz
    if op == "sha256_node":
        return off + 20 <= buf_sz
    return op == "sha256_node_pair"


def _rand_bytes(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "little") if n else b""


def sha512_prefix(rng, kind, nbytes):
    """prefix rows: random, all-zero and all-ones words"""
    return {"zero": bytes(nbytes), "ones": b"\xff" * nbytes}.get(kind) or _rand_bytes(rng, nbytes)


def sha512_cases(op, sizes_shifts, rng, buf, kinds=None):
    """one case per (size, shift) in the order given; the prefix is operand
    words [0, prefix / 4)"""
    pre_sz = SHA512_OPS[op]
    cases = []
    for i, (sz, shift) in enumerate(sizes_shifts):
        kind = kinds[i] if kinds else rng.choice(("zero", "ones") + ("random",) * 6)
        pre, msg = sha512_prefix(rng, kind, pre_sz), _rand_bytes(rng, sz)
        off = buf.place(msg, shift)
        cases.append(hash_case(op, off, sz, shift, le_words(hashlib.sha512(pre + msg).digest()), le_words(pre),
                               note=kind))
    return cases


def sha512_sweep(op, seed=71):
    """every size of SHA512_SIZES at every byte shift, laid out in size order
    (buffer, cases sorted by size: near-uniform waves, as the length sort
    gives them)"""
    rng = random.Random(seed)
    buf = HashBuf()
    cases = sha512_cases(op, [(sz, sh) for sz in SHA512_SIZES for sh in range(4)], rng, buf)
    return buf, cases


def shuffled(cases, seed=72):
    """a seeded shuffle of the same cases: divergent waves"""
    out = list(cases)
    random.Random(seed).shuffle(out)
    return out


def sha512_wave_compositions(op, seed=77):
    """(buffer, cases, names): whole blocks of chosen sizes, one composition
    a block (64 cases in the one-wave form, 32 in the two-wave form), lane l
    at byte shift l % 4.  The all-empty block comes last: in the two-wave
    form every wave also runs to case n - 1's block count, which so adds
    nothing to any composition."""
    per = hash_per_block(op)
    lanes = (0, 15, 31) if per == 32 else (0, 31, 32, 63)
    comps = [(f"all lanes {sz} bytes", [sz] * per) for sz in (47, 48, 304)]
    comps.append(("ascending with the lane", [600 * l // (per - 1) for l in range(per)]))
    comps.append(("descending with the lane", [600 * (per - 1 - l) // (per - 1) for l in range(per)]))
    for at in lanes:
        comps.append((f"one 600-byte lane at {at} among empty messages", [600 if l == at else 0 for l in range(per)]))
        comps.append((f"one empty message at lane {at} among 600-byte ones", [0 if l == at else 600 for l in range(per)]))
    comps.append(("all lanes 0 bytes", [0] * per))
    rng = random.Random(seed)
    buf, cases = HashBuf(), []
    for name, sizes in comps:
        blk = sha512_cases(op, [(sz, l % 4) for l, sz in enumerate(sizes)], rng, buf)
        for c in blk:
            c["note"] = name
        cases += blk
    return buf, cases, [name for name, _ in comps]


def sha512_dead_lane_cases(n, last, seed=78):
    """n cases of the two-wave form whose last case (the one dead lanes
    repeat, and whose block count every wave runs to) is the longest or the
    shortest of its block"""
    rng = random.Random(seed + n)
    body = [0, 47, 48, 175, 176, 303, 304, 431, 432]
    sizes = [body[i % len(body)] + (64 if last == "shortest" else 0) for i in range(n - 1)]
    sizes.append(600 if last == "longest" else 0)
    buf = HashBuf()
    return buf, sha512_cases("sha512_ram_2w", [(sz, i % 4) for i, sz in enumerate(sizes)], rng, buf)


def sha256_bytes_sweep(seed=73):
    rng = random.Random(seed)
    buf, cases = HashBuf(), []
    for sz in range(1, 301):
        for shift in range(4):
            msg = _rand_bytes(rng, sz)
            cases.append(hash_case("sha256_bytes", buf.place(msg, shift), sz, shift,
                                   be_words(hashlib.sha256(msg).digest())))
    return buf, cases


def sha256_leaf_sweep(seed=74):
    """leaf_sz 38..300 and the real leaf sizes at every shift.  The case's
    offset is 64 bytes in front of the leaf data (a shred's start); the 26
    bytes in front of the data, which the function loads and replaces with
    the prefix, are filler: the data is placed with 64 + HASH_PAD bytes of
    filler in front."""
    rng = random.Random(seed)
    buf, cases = HashBuf(), []
    for sz in list(range(38, 301)) + LEAF_REAL_SIZES:
        for shift in range(4):
            data = _rand_bytes(rng, sz)
            at = buf.place(data, shift, lead=64 + HASH_PAD)
            cases.append(hash_case("sha256_leaf", at - 64, sz, shift,
                                   be_words(hashlib.sha256(LEAF_PREFIX + data).digest())))
    return buf, cases


CHILD_CLASSES = ("random", "zero", "ones", "top", "lo16", "hi16")


def child_words(rng, cls):
    """five big-endian words of a 20-byte Merkle node; lo16 / hi16 are for the
    16-bit funnel shifts and x[0] >> 16"""
    if cls == "random":
        return [rng.getrandbits(32) for _ in range(5)]
    return [{"zero": 0, "ones": 0xffffffff, "top": 0x80000000, "lo16": 0x0000ffff, "hi16": 0xffff0000}[cls]] * 5


def words_be_bytes(w):
    return b"".join(int(x).to_bytes(4, "big") for x in w)


def sha256_node_sweep(seed=75):
    """(buffer, node cases, pair cases): every class of running node x every
    class of sibling x sibling shift x right; pair case i has the same two
    children as node case i.  A node case's operand is the running node's
    five words; the test appends words 5..7."""
    rng = random.Random(seed)
    buf, nodes, pairs = HashBuf(), [], []
    for ca in CHILD_CLASSES:
        for cb in CHILD_CLASSES:
            for shift in range(4):
                for right in (0, 1):
                    h, s = child_words(rng, ca), child_words(rng, cb)
                    left, rgt = (s, h) if right else (h, s)
                    want = be_words(hashlib.sha256(NODE_PREFIX + words_be_bytes(left) + words_be_bytes(rgt)).digest())
                    off = buf.place(words_be_bytes(s), shift)
                    note = f"node {ca}, sibling {cb}"
                    nodes.append(hash_case("sha256_node", off, 20, shift, want, h, flag=right, note=note))
                    pairs.append(hash_case("sha256_node_pair", 0, 0, 0, want, left + rgt, flag=right, note=note))
    return buf, nodes, pairs


def hash_rows(cases):
    inp = np.zeros((max(len(cases), 1), HASH_IN), np.uint32)
    for i, c in enumerate(cases):
        inp[i, 0], inp[i, 1], inp[i, 2] = c["off"], c["sz"], c["flag"]
        inp[i, 4:4 + len(c["opnd"])] = c["opnd"]
    return inp


OUT_FILL = 0x5a5aa5a5


def run_hash(diag, op, buf, cases, extra_rows=0):
    """one launch: the (n + extra_rows, 16) out array, which went in filled
    with OUT_FILL (rows past n belong to the caller and must come back so)"""
    n = len(cases)
    assert all(c["op"] == op for c in cases)
    inp = hash_rows(cases)
    out = np.full((max(n, 1) + extra_rows, HASH_OUT), OUT_FILL, np.uint32)
    rc = diag.raw_hash(HASH_OPS.index(op), buf, inp, out, n)
    assert rc == 0, f"fd_ed25519_diag_hash({op}) returned HIP error {rc}"
    return out


def hash_describe(cases, i):
    """where case i ran: op, size, shift, lane, and its wave's composition"""
    c = cases[i]
    per = hash_per_block(c["op"])
    blk = cases[i - i % per:i - i % per + per]
    sizes = [x["sz"] for x in blk]
    comp = f"block {i // per} of {len(blk)} cases, sizes {min(sizes)}..{max(sizes)}"
    if len(set(sizes)) > 1:
        comp += f" (lanes {[s for s in sizes[:8]]}...)"
    if c["op"] == "sha512_ram_2w":
        comp += f", case n-1 of {len(cases)} has {cases[-1]['sz']} bytes"
    return (f"{c['op']}: sz {c['sz']}, shift {c['shift']}, case {i} = lane {i % per} of {comp}"
            + (f", right {c['flag']}" if c["op"] == "sha256_node" else "") + (f" [{c['note']}]" if c["note"] else ""))


def hash_mismatches(cases, out):
    """descriptions of the cases whose words differ from hashlib's"""
    bad = []
    for i, c in enumerate(cases):
        w = c["want"]
        if [int(x) for x in out[i, :len(w)]] != w:
            bad.append(hash_describe(cases, i))
    return bad
