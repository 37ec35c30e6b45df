"""Plain-integer model of what each dsm loop must answer, and the packers
from (scalars, flags, points) into the work arrays each form reads
(Engine.diag_dsm, csrc/fd_ed25519_hip_internal.h).  Test infrastructure, no
product code.

The model evaluates the group sums on edwards25519 with Python integers
(extended coordinates, the complete a = -1 addition law; checked against
diag_util's affine ed_add / ed_mul in tests/test_dsm_model.py):

  half-size    [c](-A) + [|d|](-sign(d) R) + [s_lo]B + [s_hi][2^144]B == 0
  split        sum [c_i](-A_i) + sum [d_i](-+R_i) + sum [s'_q][2^(CB q)]B == 0
  full-length  [k](-A) + [S]B == R

and restates the reference's order of the checks before the equation.

The crafted cases of tests/test_gpu_dsm_diag.py are built from known
discrete logarithms -- A = [a]B + [ta]E8, R = [r]B + [tr]E8, E8 a generator
of the 8-torsion -- so their expected code also follows from two
congruences (mod L and mod 8); `case_expect` computes it that way and
tests/test_dsm_model.py holds it against the point evaluation."""
import ctypes
import hashlib
import random

import numpy as np

import diag_util as du
from diag_util import BASE, D2, L, ORDER8, P

SUCCESS, ERR_SIG, ERR_PUBKEY, ERR_MSG = 0, -1, -2, -3
PF_FAIL, PF_SMALL = 1, 2
HF_DNEG, HF_FULL = 1, 2
HALF_BITS, DBITS_MAX, BW_SHIFT = 131, 151, 144   # fd25519_half.h, FD_ED25519_BTABW_SHIFT
FORMS = {"wide": 0, "quad": 1, "oct": 2, "r16": 3, "split4": 4, "split8": 8}
# dsm16s<S>: parts per scalar, bits per part, words per part, bits per s' chunk
SPLIT = {4: dict(H=2, G=66, KW=3, CB=72), 8: dict(H=4, G=33, KW=2, CB=32)}

# ---- extended coordinates ------------------------------------------------------


def xpt(a):
    return (a[0], a[1], 1, a[0] * a[1] % P)


def xadd(p, q):
    X1, Y1, Z1, T1 = p
    X2, Y2, Z2, T2 = q
    A = (Y1 - X1) * (Y2 - X2) % P
    B = (Y1 + X1) * (Y2 + X2) % P
    C = T1 * D2 % P * T2 % P
    Dd = 2 * Z1 * Z2 % P
    E, F, G, H = B - A, Dd - C, Dd + C, B + A
    return (E * F % P, G * H % P, F * G % P, E * H % P)


def xdbl(p):
    X, Y, Z, _ = p
    A, B, C = X * X % P, Y * Y % P, 2 * Z * Z % P
    E = ((X + Y) * (X + Y) - A - B) % P
    G = B - A
    F, H = G - C, -A - B
    return (E * F % P, G * H % P, F * G % P, E * H % P)


def xneg(p):
    return ((-p[0]) % P, p[1], p[2], (-p[3]) % P)


XIDENT = (0, 1, 1, 0)


def xmul(k, p):
    r = XIDENT
    for b in bin(k)[2:] if k else "":
        r = xdbl(r)
        if b == "1":
            r = xadd(r, p)
    return r


def xmul2(k1, p1, k2, p2):
    """[k1]p1 + [k2]p2 with shared doublings"""
    both = xadd(p1, p2)
    r = XIDENT
    for i in range(max(k1.bit_length(), k2.bit_length()) - 1, -1, -1):
        r = xdbl(r)
        s = ((k1 >> i) & 1) | (((k2 >> i) & 1) << 1)
        if s:
            r = xadd(r, (p1, p2, both)[s - 1])
    return r


def x_is_ident(p):
    return p[0] % P == 0 and (p[1] - p[2]) % P == 0


def xaffine(p):
    zi = pow(p[2], P - 2, P)
    return (p[0] * zi % P, p[1] * zi % P)


_BTAB = None


def base_mul(s):
    """[s]B from [b 256^i]B, i < 32"""
    global _BTAB
    if _BTAB is None:
        _BTAB, q = [], xpt(BASE)
        for _ in range(32):
            row, cur = [XIDENT], XIDENT
            for _ in range(255):
                cur = xadd(cur, q)
                row.append(cur)
            _BTAB.append(row)
            q = xadd(cur, q)
    assert 0 <= s < 2**256
    r = XIDENT
    for i in range(32):
        b = (s >> (8 * i)) & 255
        if b:
            r = xadd(r, _BTAB[i][b])
    return r


# ---- what each loop must answer ---------------------------------------------


def half_is_identity(c, dm, dneg, s_lo, s_hi, A, R):
    """A, R affine; the half-size sum as the loops evaluate it"""
    na = xneg(xpt(A))
    rr = xpt(R) if dneg else xneg(xpt(R))
    s = xmul2(c, na, dm, rr)
    s = xadd(s, base_mul(s_lo))
    s = xadd(s, xmul(1 << BW_SHIFT, base_mul(s_hi)))
    return x_is_ident(s)


def split_is_identity(waves, parts, dneg, chunks, As, Rs):
    """parts: the 2H split scalars (c_0.., d_0..); chunks: the S chunks of
    s'; As, Rs: the H points of each side as the test supplied them
    (extended coordinates)"""
    k = SPLIT[waves]
    s = XIDENT
    for i in range(k["H"]):
        s = xadd(s, xmul(parts[i], xneg(As[i])))
        s = xadd(s, xmul(parts[k["H"] + i], Rs[i] if dneg else xneg(Rs[i])))
    for q in range(waves):
        s = xadd(s, base_mul(chunks[q] << (k["CB"] * q)))
    return x_is_ident(s)


def full_is_equal(kk, S, A, R):
    """[k](-A) + [S]B == R as affine points"""
    s = xadd(xmul(kk, xneg(xpt(A))), base_mul(S))
    return xaffine(s) == (R[0] % P, R[1] % P)


def precheck(sflag, af, rf, portable):
    """the reference's checks before the equation, in its order; None: pending"""
    if not sflag:
        return ERR_SIG
    if af & PF_FAIL:
        return ERR_PUBKEY if portable else ERR_SIG
    if rf & PF_FAIL:
        return ERR_SIG
    if af & PF_SMALL:
        return ERR_PUBKEY
    if rf & PF_SMALL:
        return ERR_SIG
    return None


def model_code(case, portable, A, R):
    """the code of one case from its flags, scalars and affine points"""
    pre = precheck(case["sflag"], case["af"], case["rf"], portable)
    if pre is not None:
        return pre
    if case["full"]:
        ok = full_is_equal(case["k"], case["S"], A, R)
    else:
        sp = case["sp"]
        ok = half_is_identity(case["c"], case["dm"], case["dneg"], sp % (1 << BW_SHIFT), sp >> BW_SHIFT, A, R)
    return SUCCESS if ok else ERR_MSG


# ---- points with known discrete logarithms ------------------------------------

_PT = {}


def dl_point(a, t):
    """[a]B + [t]E8, affine"""
    key = (a % L, t % 8)
    if key not in _PT:
        _PT[key] = xaffine(xadd(base_mul(key[0]), xmul(key[1], xpt(ORDER8))))
    return _PT[key]


def case_expect(case, portable=False):
    """the expected code from the discrete logarithms alone"""
    pre = precheck(case["sflag"], case["af"], case["rf"], portable)
    if pre is not None:
        return pre
    (a, ta), (r, tr) = case["A"], case["R"]
    if case["full"]:   # -k A + S B - R
        ok = (case["S"] - case["k"] * a - r) % L == 0 and (case["k"] * ta + tr) % 8 == 0
    else:              # -c A - sign(d) |d| R + s' B
        sd = -case["dm"] if case["dneg"] else case["dm"]
        ok = (case["sp"] - case["c"] * a - sd * r) % L == 0 and (case["c"] * ta + sd * tr) % 8 == 0
    return SUCCESS if ok else ERR_MSG


def half_case(c, d, sp, A, R, **kw):
    case = dict(c=c, dm=abs(d), dneg=int(d < 0), sp=sp, A=A, R=R, sflag=1, af=0, rf=0, full=False, k=0, S=0)
    case.update(kw)
    return case


def solve_sp(c, d, A, R):
    return (c * A[0] + d * R[0]) % L


def solve_r(c, d, sp, A):
    """r with s' == c a + d r (mod L); d != 0 mod L"""
    return (sp - c * A[0]) * pow(d % L, L - 2, L) % L


def solve_tr(c, d, ta, target=0):
    """tr with c ta + d tr == target (mod 8), or None"""
    for tr in range(8):
        if (c * ta + d * tr - target) % 8 == 0:
            return tr
    return None


# ---- packers -------------------------------------------------------------------


def limbs_x(v):
    """tight centered limbs (what fe_mul leaves, sign applied)"""
    return du.fe_centered(v % P, True)


def limbs_y(v):
    """fe_frombytes's unsigned limbs of the canonical value"""
    return du.fe_digits(v % P)


def words5(v, n=5):
    return du.words(v, n)


def pack_nonsplit(cases, pts=None):
    """cases -> dict of the arrays of forms 0..3, stride n; pts: per case the
    affine (A, R), default the cases' discrete-log points"""
    n = len(cases)
    a = dict(sflag=np.zeros(n, np.uint8), hflag=np.zeros(n, np.uint8), pflag=np.zeros((2, n), np.uint8),
             pts=np.zeros((40, n), np.int32), hs=np.zeros((19, n), np.uint32), k=np.zeros((8, n), np.uint32),
             S=np.zeros((n, 64), np.uint8))
    for j, cs in enumerate(cases):
        A, R = pts[j] if pts is not None else (dl_point(*cs["A"]), dl_point(*cs["R"]))
        a["sflag"][j] = cs["sflag"]
        a["hflag"][j] = (HF_DNEG if cs["dneg"] else 0) | (HF_FULL if cs["full"] else 0)
        a["pflag"][0, j], a["pflag"][1, j] = cs["af"], cs["rf"]
        a["pts"][:, j] = limbs_x(A[0]) + limbs_y(A[1]) + limbs_x(R[0]) + limbs_y(R[1])
        sp = cs["sp"]
        a["hs"][:, j] = words5(cs["c"]) + words5(cs["dm"]) + words5(sp % (1 << BW_SHIFT)) + words5(sp >> BW_SHIFT, 4)
        a["k"][:, j] = du.words(cs["k"], 8)
        a["S"][j, 32:] = np.frombuffer(int(cs["S"]).to_bytes(32, "little"), np.uint8)
    return a


def record(cs):
    """hsrec's 32-word record of a half-size case"""
    sp = cs["sp"]
    rec = du.words(cs["k"], 8) + words5(cs["c"]) + words5(cs["dm"]) + words5(sp % (1 << BW_SHIFT)) + \
        words5(sp >> BW_SHIFT, 4) + [cs["sflag"], cs["dneg"]] + [0] * 3
    return np.array(rec, np.uint32)


def split_rule(waves, c, dm, sp):
    """the split rule restated: (the 2H parts, the S chunks of s')"""
    k = SPLIT[waves]
    H, G, CB = k["H"], k["G"], k["CB"]
    parts = []
    for v in (c, dm):
        parts += [(v >> (G * i)) & ((1 << G) - 1) for i in range(H - 1)] + [v >> (G * (H - 1))]
    return parts, [(sp >> (CB * q)) & ((1 << CB) - 1) for q in range(waves)]


def split_rows(waves, c, dm, sp):
    """... as hssplit's 24 rows of words"""
    k = SPLIT[waves]
    parts, chunks = split_rule(waves, c, dm, sp)
    rows = []
    for v in parts:
        rows += du.words(v, k["KW"])
    for v in chunks:
        rows += du.words(v, (k["CB"] + 31) // 32)
    return rows + [0] * (24 - len(rows))


def hssplit(lib, rec, waves, cap=1, j=0):
    f = lib.fd_ed25519_hip_private_hssplit
    if f.argtypes is None:
        f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_ulong, ctypes.c_ulong]
        f.restype = None
    hq = np.zeros((24, cap), np.uint32)
    rec = np.ascontiguousarray(rec, np.uint32)
    f(rec.ctypes.data, waves, hq.ctypes.data, cap, j)
    return hq


_DBL = {}


def doubled(pt, waves, rng):
    """[2^(G i)]pt, i < H, in extended coordinates; i >= 1 scaled by a random Z != 1"""
    k = SPLIT[waves]
    if (pt, waves) not in _DBL:
        chain, cur = [], xpt(pt)
        for _ in range(1, k["H"]):
            for _ in range(k["G"]):
                cur = xdbl(cur)
            chain.append(cur)
        _DBL[(pt, waves)] = chain
    out = [xpt(pt)]
    for cur in _DBL[(pt, waves)]:
        z = rng.randrange(2, P)
        out.append(tuple(v * z % P for v in cur))
    return out


def pack_split(lib, waves, cases, rng, pts=None):
    """cases -> the split form's arrays (scalars through the product's own
    hssplit), and per case the points supplied (for the model)"""
    n = len(cases)
    a = dict(sflag=np.zeros(n, np.uint8), hflag=np.zeros(n, np.uint8), pflag=np.zeros((2, n), np.uint8),
             pts=np.zeros((waves * 40, n), np.int32), hs=np.zeros((24, n), np.uint32))
    supplied = []
    for j, cs in enumerate(cases):
        assert not cs["full"]
        A, R = pts[j] if pts is not None else (dl_point(*cs["A"]), dl_point(*cs["R"]))
        a["sflag"][j] = cs["sflag"]
        a["hflag"][j] = HF_DNEG if cs["dneg"] else 0
        a["pflag"][0, j], a["pflag"][1, j] = cs["af"], cs["rf"]
        a["hs"][:, j] = hssplit(lib, record(cs), waves)[:, 0]
        As, Rs = doubled(A, waves, rng), doubled(R, waves, rng)
        supplied.append((As, Rs))
        for side, (aff, ext) in enumerate(((A, As), (R, Rs))):
            a["pts"][side * 40:side * 40 + 20, j] = limbs_x(aff[0]) + limbs_y(aff[1])
            for i in range(1, SPLIT[waves]["H"]):
                row = (2 * i + side) * 40
                a["pts"][row:row + 40, j] = sum((limbs_x(v) for v in ext[i]), [])
    return a, supplied


def take(arrays, idx):
    """the arrays of the cases idx (columns; S by rows)"""
    return {k: (v[idx] if k in ("sflag", "hflag", "S") else v[:, idx]) for k, v in arrays.items()}


# ---- the fixtures' signatures as cases --------------------------------------

def fixture_cases(lib, d, avx, dbits=151):
    """per signature of a fixture: (case, A, R) -- the case from hsrec (or k
    and the full-length flag), the points and flags from hsdec_n"""
    from conftest import case
    lib.fd_ed25519_hip_private_hsrec.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_ulong,
                                                 ctypes.c_int, ctypes.c_void_p]
    lib.fd_ed25519_hip_private_hsdec_n.argtypes = [ctypes.c_void_p, ctypes.c_ulong, ctypes.c_int, ctypes.c_void_p,
                                                   ctypes.c_void_p]
    lib.fd_ed25519_hip_private_hsdec_n.restype = None
    n = len(d["msg_sz"])
    encs = []
    for i in range(n):
        _, s, p = case(d, i)
        encs += [p, s[:32]]
    bufs = [ctypes.create_string_buffer(e, 32) for e in encs]
    arr = (ctypes.c_void_p * len(bufs))(*[ctypes.addressof(b) for b in bufs])
    pt = np.zeros((2 * n, 20), np.int32)
    fl = np.zeros(2 * n, np.uint8)
    lib.fd_ed25519_hip_private_hsdec_n(ctypes.addressof(arr), 2 * n, 1 if avx else 0, pt.ctypes.data, fl.ctypes.data)
    out = []
    for i in range(n):
        m, s, p = case(d, i)
        rec = np.zeros(32, np.uint32)
        S = int.from_bytes(s[32:], "little")
        if lib.fd_ed25519_hip_private_hsrec(s, p, m, len(m), dbits, rec.ctypes.data):
            w = lambda a, k: du.from_words(rec[a:a + k])
            cs = half_case(w(8, 5), -w(13, 5) if rec[28] & 1 else w(13, 5), w(18, 5) + (w(23, 4) << 144), None, None,
                              sflag=int(rec[27]), dneg=int(rec[28] & 1))
            assert int(rec[27]) == int(S < L)
        else:
            k = int.from_bytes(hashlib.sha512(s[:32] + p + m).digest(), "little") % L
            cs = full_case(k, S, None, None)
            assert S < L   # hsrec: only a k without a pair, under S < L, has no record
        cs["af"], cs["rf"] = int(fl[2 * i]), int(fl[2 * i + 1])
        A = (du.fe_val(pt[2 * i][:10]), du.fe_val(pt[2 * i][10:]))
        R = (du.fe_val(pt[2 * i + 1][:10]), du.fe_val(pt[2 * i + 1][10:]))
        out.append((cs, A, R, pt[2 * i], pt[2 * i + 1]))
    return out


# ---- operand classes -----------------------------------------------------------


def pat(nib, bits):
    """the nibble (or byte) pattern repeated below 2^bits"""
    w = 4 if nib < 16 else 8
    return sum(nib << (w * i) for i in range(bits // w + 1)) & ((1 << bits) - 1)


def window_values(bits):
    """values below 2^bits for c (bits 131) and |d| (bits 151 or 131)"""
    nw = (bits + 3) // 4
    xs = [0, 1, 2**131 - 1]
    for i in range(nw):
        xs += [v << (4 * i) for v in (1, 7, 8, 9, 15)]
        xs += [1 << (4 * i + 3), (1 << (4 * i + 3)) - 1]
    xs += [pat(0x8, bits), pat(0x7, bits), pat(0xf0, bits), pat(0x0f, bits), pat(0x8, bits - 1), pat(0x8, bits - 2)]
    top = 4 * (nw - 1)
    xs += [(t << top) | pat(0x8, top) for t in range(8)] + [(t << top) | pat(0x7, top) for t in range(8)]  # top digit recodes to t+1, t
    xs += [v for v in (1, 7, 8, 9, 15)] + [(v << 120) for v in (1, 8, 15)]   # a low digit under thirty zero windows, and above them
    return sorted({x for x in xs if x < 2**bits})


def d_lengths(lo=128, hi=151):
    """|d| = 2^(b-1) and 2^b - 1: both sides of every window step"""
    return [v for b in range(lo, hi + 1) for v in (1 << (b - 1), (1 << b) - 1)]


def sp_values():
    xs = [0, 1, L - 1, L, 2**144 - 1, 2**144, 2**253 - 1]
    for bw in (24, 16):
        for base, top in ((0, 144), (144, 253)):
            for m in range((top - base + bw - 1) // bw):
                lo = base + bw * m
                xs += [1 << lo, (((1 << bw) - 1) << lo) & ((1 << top) - 1)]
    for cb in (72, 32):
        for q in range(256 // cb + 1):
            if cb * q < 253:
                xs.append((((1 << cb) - 1) << (cb * q)) & (2**253 - 1))                    # a chunk alone at its maximum
                xs.append((2**253 - 1) & ~(((1 << cb) - 1) << (cb * q)))                  # ... alone at 0
    return sorted({x for x in xs if x < 2**253})


def split_scalar_values(bits):
    xs = []
    for G, H in ((66, 2), (33, 4)):
        for i in range(H):
            for v in (1, (1 << G) - 1, pat(0x8, G), pat(0x8, G - 1)):
                xs.append(v << (G * i))                               # the chunk alone
                xs.append(((1 << bits) - 1) & ~(((1 << G) - 1) << (G * i)))   # the chunk alone at 0
    return sorted({x for x in xs if x < 2**bits})


def crafted_half_cases(seed=7, dbits=DBITS_MAX):
    """the valid cases with their near misses: (cases, kinds)"""
    rng = random.Random(seed)
    pool = [(rng.randrange(1, L), t) for t in (0, 0, 0, 1, 2, 3, 4, 5, 6, 7)] + [(m, 0) for m in (1, 2, 3, 8)]
    out, kinds = [], []

    def rnd_c():
        return rng.getrandbits(HALF_BITS)

    def rnd_d():
        return (rng.getrandbits(rng.choice((HALF_BITS, HALF_BITS, dbits))) | 1) * rng.choice((1, -1))

    def emit(cs, kind):
        out.append(cs)
        kinds.append(kind)

    def family(c, d, sp=None, A=None, R=None, misses=("sp", "win", "sign")):
        """one valid case and near misses of it.  With sp given r is solved
        (d != 0), else s' is solved from the points."""
        A = A or rng.choice(pool)
        if R is None:
            if sp is None:
                sp = rng.randrange(L)
            if d % L:
                tr = solve_tr(c, d, A[1])
                if tr is None:
                    A, tr = (A[0], 0), 0
                R = (solve_r(c, d, sp, A), tr)
            else:   # no R term: a is solved instead (c != 0), or s' itself
                R = rng.choice(pool)
                if c % L:
                    A = ((sp * pow(c, L - 2, L)) % L, 0)
                else:
                    sp = sp if sp % L == 0 else 0
        else:
            sp = solve_sp(c, d, A, R)
        v = half_case(c, d, sp, A, R)
        emit(v, "valid" if case_expect(v) == SUCCESS else "invalid")
        m = list(misses)
        if "sp" in m:
            for e in (1, -1):
                if 0 <= sp + e < 2**253:
                    emit(half_case(c, d, sp + e, A, R), "sp")
        if "win" in m:
            i = rng.randrange(33)
            for cc, dd in ((c + (1 << (4 * i)), d), (c - (1 << (4 * i)), d),
                           (c, (abs(d) + (1 << (4 * i))) * (1 if d >= 0 else -1))):
                if 0 <= cc < 2**HALF_BITS and abs(dd) < 2**dbits:
                    emit(half_case(cc, dd, sp, A, R), "win")
        if "sign" in m:
            emit(half_case(c, -d, sp, A, R, dneg=int(d >= 0)), "sign")
            emit(half_case(c, d, sp, A, (-R[0] % L, -R[1] % 8)), "rneg")
        if "tors" in m and d % 2:
            for t in range(1, 8):
                emit(half_case(c, d, sp, A, (R[0], solve_tr(c, d, A[1], t))), "tors")

    cv, dv = window_values(HALF_BITS), window_values(dbits)
    for i, c in enumerate(cv):
        family(c, rnd_d(), misses=("sp", "win") if i % 4 else ("sp", "win", "sign", "tors"))
    for i, dm in enumerate(dv):
        family(rnd_c(), dm * (1 if i % 2 else -1), misses=("sp", "sign") if i % 4 else ("sp", "win", "sign", "tors"))
    for dm in d_lengths(128, dbits):
        for s in (1, -1):
            family(rnd_c(), s * dm, misses=("sp", "sign"))
    for i, sp in enumerate(sp_values()):
        family(rnd_c(), rnd_d(), sp=sp, misses=("sp",) if i % 4 else ("sp", "win", "sign", "tors"))
    for v in split_scalar_values(HALF_BITS):
        family(v, rnd_d(), misses=("sp", "win"))
    for v in split_scalar_values(dbits):
        family(rnd_c(), v * rng.choice((1, -1)), misses=("sp", "sign"))
    family(0, 0, sp=0, misses=("sp",))
    family(0, 0, sp=L, misses=("sp",))
    family(0, rnd_d(), misses=("sp", "sign"))
    family(rnd_c(), 0, misses=("sp", "win"))
    # points: every torsion component on A and on R, A = R, A = -R, small multiples of B
    a0 = rng.randrange(1, L)
    for ta in range(8):
        for tr in range(8):
            family(rnd_c(), rnd_d(), A=(a0, ta), R=(rng.randrange(1, L), tr), misses=("sp",))
    for A, R in (((a0, 0), (a0, 0)), ((a0, 0), (-a0 % L, 0)), ((a0, 3), (a0, 3)), ((a0, 3), (-a0 % L, 5)),
                 ((0, 0), (a0, 0)), ((a0, 0), (0, 0)), ((0, 4), (0, 1))):
        family(rnd_c(), rnd_d(), A=A, R=R, misses=("sp", "sign"))
    for ma in (1, 2, 3, 4, 7, 8, 9, 16, 2**16, 2**24 - 1, 2**144):
        for mr in (1, 2, 8, 2**144 % L):
            family(rnd_c(), rnd_d(), A=(ma, 0), R=(mr, 0), misses=("sp",))
            family(rng.randrange(1, 9), rng.choice((1, 3, -5, 7)), A=(ma, 0), R=(mr, 0), misses=("sp",))
    for _ in range(40):
        family(rnd_c(), rnd_d(), misses=("sp", "win", "sign", "tors"))
    return out, kinds


def full_case(k, S, A, R, **kw):
    cs = dict(c=0, dm=1, dneg=0, sp=0, A=A, R=R, sflag=int(S < L), af=0, rf=0, full=True, k=k, S=S)
    cs.update(kw)
    return cs


def crafted_full_cases(seed=11):
    """the full-length form: k [k](-A) + [S]B == R' with R' = R, -R, R + torsion"""
    rng = random.Random(seed)
    ks = [0, 1, L - 1, pat(0x8, 252), pat(0x7, 252), pat(0x8, 251)] + [v << (4 * i) for i in range(63) for v in (1, 8, 15)
                                                                    if (v << (4 * i)) < 2**253]
    Ss = [0, 1, L - 1] + [v << (16 * i) for i in range(16) for v in (0x7fff, 0x8000, 0xffff)]
    out = []

    def family(k, S, full=True):
        A = (rng.randrange(1, L), rng.randrange(8))
        R = ((S - k * A[0]) % L, (-k * A[1]) % 8)
        out.append(full_case(k, S, A, R))
        if full:
            out.append(full_case(k, S, A, (-R[0] % L, -R[1] % 8)))
            out.append(full_case(k, S, A, (R[0], (R[1] + rng.randrange(1, 8)) % 8)))
            out.append(full_case(k, S, A, ((R[0] + 1) % L, R[1])))

    for i, k in enumerate(ks):
        family(k, rng.randrange(L), full=i % 8 == 0 or i < 6)
    for i, S in enumerate(Ss):
        family(rng.randrange(L), S, full=i % 8 == 0 or i < 3)
    return out
