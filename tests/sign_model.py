"""Plain-integer model of the device signer (fd_ed25519_sign_kernel,
firedancer_amd/csrc/fd_ed25519_gen.hip) and the case builders of
tests/test_gpu_sign_diag.py.  Test infrastructure, no product code.

  sign            RFC 8032 5.1.5-5.1.6 with hashlib, dsm_model.base_mul and
                  integers mod L; every intermediate is returned
  recode256       the radix-256 signed digits ge_scalarmult_base walks
  table           the signer's table as integers: entry e = (y+x, y-x, 2dxy)
                  of [e]B, e = 0..128
  base_points     [s]B for many s, affine, with one inversion for all
  *_cases         the operand classes; tests/test_sign_cases.py asserts on
                  the CPU what each promises

Everything is exact: Python integers, no tolerances."""
import hashlib
import random

import bounds_model as bm
import diag_util as du
import dsm_model as dm
from diag_util import BASE, D2, L, P

BTAB_ENTRIES, BTAB_STRIDE = 129, 36      # fd_ed25519_hip_internal.h FD_ED25519_BTAB_*
M256 = 2**256 - 1


# ---- the signer ----------------------------------------------------------------

def encode(pt):
    """RFC 8032 5.1.2: canonical y, the parity of canonical x in bit 255"""
    x, y = pt[0] % P, pt[1] % P
    return y | ((x & 1) << 255)


def batch_affine(xpts):
    """affine (x, y) of extended points, one inversion for all (Montgomery's trick)"""
    pre, acc = [], 1
    for p in xpts:
        pre.append(acc)
        acc = acc * p[2] % P
    inv = pow(acc, P - 2, P)
    assert acc * inv % P == 1        # no Z is 0
    out = [None] * len(xpts)
    for i in range(len(xpts) - 1, -1, -1):
        zi = inv * pre[i] % P
        inv = inv * xpts[i][2] % P
        out[i] = (xpts[i][0] * zi % P, xpts[i][1] * zi % P)
    return out


def base_points(scalars):
    """[s mod L]B for every s, affine"""
    return batch_affine([dm.base_mul(s % L) for s in scalars])


def clamp(h32):
    return (int.from_bytes(h32, "little") & ((1 << 255) - 8)) | (1 << 254)


def sign_many(privs, msgs):
    """RFC 8032 signatures of msgs[i] under the 32-byte private keys privs[i]:
    a list of dicts with a (clamped, not reduced), prefix, r, k (both mod L),
    R, A (affine), S, and the bytes sig (64) and pub (32)"""
    hs = [hashlib.sha512(p).digest() for p in privs]
    a = [clamp(h[:32]) for h in hs]
    A = base_points(a)
    pubs = [encode(pt).to_bytes(32, "little") for pt in A]
    r = [int.from_bytes(hashlib.sha512(h[32:] + m).digest(), "little") % L for h, m in zip(hs, msgs)]
    R = base_points(r)
    out = []
    for i, m in enumerate(msgs):
        rb = encode(R[i]).to_bytes(32, "little")
        k = int.from_bytes(hashlib.sha512(rb + pubs[i] + m).digest(), "little") % L
        S = (r[i] + k * a[i]) % L
        out.append(dict(a=a[i], prefix=hs[i][32:], r=r[i], k=k, R=R[i], A=A[i], S=S,
                        sig=rb + S.to_bytes(32, "little"), pub=pubs[i]))
    return out


def sign(priv, msg):
    return sign_many([priv], [msg])[0]


# ---- the scalar multiply's digits and table -----------------------------------

def recode256(s):
    """fd25519_dsm.h recode_radix256: 32 digits, sum f_j 256^j = s, f_j in
    [-128, 127] for j < 31 (a byte of 128 or more borrows from the next)"""
    assert 0 <= s < 2**256
    out, carry = [], 0
    for j in range(32):
        f = ((s >> (8 * j)) & 255) + carry
        carry = (f + 128) >> 8
        out.append(f - 256 * carry)
    assert carry == 0 or s >= 2**255
    return out


def leading_zero_digits(d):
    n = 0
    while n < 32 and d[31 - n] == 0:
        n += 1
    return n


_TABLE = None


def table():
    """entry e = (y + x, y - x, 2 d x y) mod p of [e]B, e = 0 .. 128, by repeated addition of B"""
    global _TABLE
    if _TABLE is None:
        pts, cur = [], dm.XIDENT
        for _ in range(BTAB_ENTRIES):
            pts.append(cur)
            cur = dm.xadd(cur, dm.xpt(BASE))
        _TABLE = [((y + x) % P, (y - x) % P, D2 * x * y % P) for x, y in batch_affine(pts)]
    return _TABLE


def entry_point(ent):
    """the affine point of a table entry (y+x, y-x, .)"""
    i2 = pow(2, P - 2, P)
    return ((ent[0] - ent[1]) * i2 % P, (ent[0] + ent[1]) * i2 % P)


# ---- op 0: scalars below L -----------------------------------------------------

BYTE_EDGES = (0x01, 0x7f, 0x80, 0x81, 0xff)
TOP_DIGITS = range(0, 17)
"""recode_radix256 documents f_31 in [0, 17], which holds for any scalar below
2^252 + 2^247.  Below L it is [0, 16]: L = 2^252 + 2^124.6.., so a scalar with
top byte 0x10 has bytes 16..30 zero and nothing carries into digit 31."""


def base_scalars(seed=61):
    """(scalars, classes): every scalar is below L; classes maps a class name to its index range"""
    xs, classes = [], {}

    def add(name, vals):
        vals = list(vals)
        assert all(0 <= v < L for v in vals), name
        classes[name] = (len(xs), len(xs) + len(vals))
        xs.extend(vals)

    add("edges", du.scalar_edges_lt_l(random.Random(seed)))
    # L - 0 is L itself: the table's ends from below are e and, for e >= 1, L - e
    add("small", [e for e in range(129)] + [L - e for e in range(1, 129)])
    alone, filled = [], []
    for pos in range(32):
        for b in BYTE_EDGES:
            alone.append(b << (8 * pos))
            filled.append((b << (8 * pos)) | ((1 << (8 * pos)) - 1))
    add("byte alone", [v for v in alone if v < L])
    add("byte over ones", [v for v in filled if v < L])
    add("repeated", [int.from_bytes(bytes([b]) * 32, "little") % L for b in (0x80, 0x7f)])
    add("powers", [v for k in range(253) for v in (2**k, 2**k - 1)])
    # what the lists above leave open: every digit value at every lower position (a byte b alone at
    # position j recodes to b, or to b - 256 with 1 carried up), and every top digit with and
    # without a carry into it
    add("every byte", [b << (8 * pos) for pos in range(31) for b in range(1, 256)])
    add("top", [t << 248 for t in range(17)] + [(t << 248) | (0x80 << 240) for t in range(16)])
    if len(xs) % 256 == 0:
        add("odd lane", [L - 129])
    return xs, classes


# ---- op 1: any 256-bit scalar --------------------------------------------------

def base_wide_scalars(seed=62):
    rng = random.Random(seed)
    xs = [2**254, 2**255 - 8, 2**254 + 8, 2**255 - 16, M256, 0, 1]
    m = 1
    while L * m - 1 <= M256:
        xs += [v for v in (L * m - 1, L * m, L * m + 1) if v <= M256]
        m += 1
    assert m == 16
    xs += [rng.getrandbits(256) for _ in range(300)]
    return xs


# ---- op 2: k a + r -------------------------------------------------------------

def muladd_triples(seed=63):
    """(k, a, r) triples, each operand below 2^256"""
    rng = random.Random(seed)
    ends = (0, 1, M256)
    ts = [(k, a, r) for k in ends for a in ends for r in ends]
    ts += [(k, a, r) for k in (L - 1, L, L + 1) for a in (2**254, 2**255 - 8) for r in (L - 1, M256)]
    for w in range(8):
        one = 0xffffffff << (32 * w)
        rnd = [rng.getrandbits(256) for _ in range(3)]
        for others in ((0, 0), (M256, M256), (rnd[0], rnd[1])):
            ts += [(one, others[0], others[1]), (others[0], one, others[1]), (others[0], others[1], one)]
        ts += [(one, 0xffffffff << (32 * v), rnd[2]) for v in range(8)]
    # (2^256 - 1)^2 = 2^512 - 2^257 + 1: the low half is 1, so r = 2^256 - 1 makes the sum's low half
    # exactly 2^256 -- every low word wraps to zero and the carry leaves word 7 for the upper half
    ts += [(M256, M256, M256), (M256, M256, M256 - 1), (M256, M256, 0)]
    for _ in range(40):              # multiples of L and one less
        k, a = rng.getrandbits(256), rng.getrandbits(256)
        r = -(k * a) % L
        ts += [(k, a, r), (k, a, (r - 1) % L), (L * rng.randrange(1, 16), a, 0), (k, L * rng.randrange(1, 16), L)]
    ts += [(rng.getrandbits(256), rng.getrandbits(256), rng.getrandbits(256)) for _ in range(2000)]
    assert all(0 <= v <= M256 for t in ts for v in t)
    return ts


# ---- op 3: points to encode ----------------------------------------------------

def encode_bound():
    """per-limb upper ends of what ge_p1p1_to_p2 leaves in the scalar multiply (about two units)"""
    Q, _, _ = bm.sign_base_loop()
    return {c: [hi for _, hi in Q[c]] for c in "XYZ"}, {c: [lo for lo, _ in Q[c]] for c in "XYZ"}


def encode_cases(seed=64):
    """(X limbs, Y limbs, Z limbs, affine point, note): torsion points, B and
    random points of either x parity, over Z = 1, a random Z in plain digits
    and Z in the unsigned form of ge_p1p1_to_p2's output (random limbs in its
    interval, and every limb at the interval's end), X and Y in each
    representation du.fe_reps finds within that bound"""
    rng = random.Random(seed)
    hi, lo = encode_bound()
    # unsigned products: nothing below zero but what the carry join can take from limbs 1 and 6
    assert all(-1024 < v <= 0 for c in "XYZ" for v in lo[c])
    pts = [("identity", du.IDENT), ("order 2", du.ORDER2), ("order 4", du.ORDER4[0]), ("order 4'", du.ORDER4[1]),
           ("order 8", du.ORDER8), ("order 8 negated", du.ed_neg(du.ORDER8)), ("B", BASE), ("-B", du.ed_neg(BASE))]
    rnd = base_points([rng.randrange(1, L) for _ in range(24)])
    even, odd = [p for p in rnd if p[0] % 2 == 0][:4], [p for p in rnd if p[0] % 2 == 1][:4]
    assert len(even) == 4 and len(odd) == 4
    pts += [("random, x even", p) for p in even] + [("random, x odd", p) for p in odd]
    cases = []
    for name, pt in pts:
        assert du.on_curve(pt)
        zs = [("Z = 1", [1] + [0] * 9), ("Z plain", du.fe_digits(rng.randrange(1, P))),
              ("Z unsigned", [rng.randint(l, h) for l, h in zip(lo["Z"], hi["Z"])]), ("Z at the bound", list(hi["Z"]))]
        for zname, zl in zs:
            z = du.fe_val(zl)
            assert z != 0 and du.within(zl, lo["Z"], hi["Z"])
            xr, yr = du.fe_reps(pt[0] * z % P, hi["X"]), du.fe_reps(pt[1] * z % P, hi["Y"])
            for i in range(max(len(xr), len(yr))):
                cases.append((xr[i % len(xr)], yr[i % len(yr)], zl, pt, f"{name}, {zname}, rep {i}"))
    return cases


# ---- the whole kernel: roots ---------------------------------------------------

ROOTS = 2048


def root_cases(seed=65, n=ROOTS):
    """(privs, msgs): n seeded private keys with one 32-byte message each, the seal's shape"""
    rng = random.Random(seed)
    privs = [rng.getrandbits(256).to_bytes(32, "little") for _ in range(n)]
    msgs = [rng.getrandbits(256).to_bytes(32, "little") for _ in range(n)]
    return privs, msgs


_ROOT_SIGS = {}


def root_signatures(seed=65, n=ROOTS):
    """sign_many of root_cases, computed once a process"""
    if (seed, n) not in _ROOT_SIGS:
        _ROOT_SIGS[(seed, n)] = sign_many(*root_cases(seed, n))
    return _ROOT_SIGS[(seed, n)]
