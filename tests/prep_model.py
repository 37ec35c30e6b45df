"""Plain-integer model of the work arrays the hash, scalar and decode phases
hand to dsm (csrc/fd_ed25519_hip_internal.h: k, sflag, hs, hflag, pts,
pflag), and the inputs those phases are checked on (Engine.diag_prep,
tests/test_gpu_prep_diag.py; tests/test_prep_model.py pins the model and the
inputs on the CPU first).  Test infrastructure: hashlib, Python integers and
the Euclid of tests/half_euclid_model.py, no import of the code under test.

  k      = SHA-512(R || A || M) mod L, or the caller's digest mod L
  sflag  = S < L
  c, d   : half_euclid_model.pair_cd(k), found within dbits or not
  s'     = d S mod L for the signed d, stored as s' mod 2^144 (rows 10..14,
           row 14 below 2^16) and s' >> 144 (rows 15..18)
  points : the reference's decompression rules (fd_ed25519_point_frombytes,
           fd_ed25519_affine_is_small_order), `expected` below

The inputs: every signature draws R, A, S and its message (or digest) on its
own from pools of edge values, so that the classes a whole verify cannot
observe -- non-canonical y, S = 0 under d < 0, k without a pair beside S >= L
-- all occur, in every position of a wave."""
import functools
import hashlib
import random

import numpy as np

import half_euclid_model as hm
from conftest import load_golden

P = 2**255 - 19
L = hm.L
D = (-121665 * pow(121666, P - 2, P)) % P
SQRTM1 = pow(2, (P - 1) // 4, P)
OFF = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
# the order-8 points' y (fd25519_dsm.h ge_decode)
Y0 = int.from_bytes(bytes.fromhex("26e8958fc2b227b045c3f489f2ef98f0d5dfac05d3c63339b13802886d53fc05"), "little")
Y1 = int.from_bytes(bytes.fromhex("c7176a703d4dd84fba3c0b760d10670f2a2053fa2c39ccc64ec7fd7792ac037a"), "little")
BW_SHIFT = 144   # FD_ED25519_BTABW_SHIFT
PF_FAIL, PF_SMALL = 1, 2
HF_DNEG, HF_FULL = 1, 2
UNWRITTEN = 0x55   # FD_ED25519_DIAG_DSM_UNWRITTEN
FORMS = {"wide": 0, "fused1": 1, "fused2": 2, "r16": 3, "r16_decode": 4, "r16_full": 5}
DSM_FORM = {"wide": (0,), "fused1": (1,), "fused2": (2,), "r16": (3,)}   # the dsm form(s) that consume a prep form's arrays


def expected(enc, avx):
    """(flags, sign-adjusted x, y as encoded) of a 32-byte point encoding"""
    raw = int.from_bytes(enc, "little")
    sign = raw >> 255
    yr = raw & (2**255 - 1)
    y = yr % P
    u, v = (y * y - 1) % P, (D * y * y + 1) % P
    x = u * pow(v, 3, P) * pow(u * pow(v, 7, P), (P - 5) // 8, P) % P
    vxx = v * x * x % P
    root, iroot = vxx == u, vxx == (-u) % P
    if not root:
        x = x * SQRTM1 % P
    x0 = x == 0
    fail = not (root or iroot) or (avx and x0 and sign == 1)
    if (x & 1) != sign:
        x = (P - x) % P
    small = x0 or y == 0 or y == Y0 or y == Y1
    return (1 if fail else 0) | (2 if small else 0), x, yr


expected_kept = functools.lru_cache(maxsize=None)(expected)   # the pools repeat their encodings


def y_limbs(yr):
    """fe_frombytes's split of the encoding's low 255 bits"""
    return [(yr >> o) & ((1 << (26 if i % 2 == 0 else 25)) - 1) for i, o in enumerate(OFF)]


def limbs_value(cols):
    """the values mod p of ten rows of limbs [10][n], as Python integers"""
    acc = np.zeros(cols.shape[1], dtype=object)
    for i in range(10):
        acc = acc + (cols[i].astype(object) << OFF[i])
    return acc % P


def words(v, n):
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def scalar_rows(k, S, dbits):
    """(found, d < 0, the 19 rows of hs) for one signature; the rows mean
    something only where found"""
    c, d = hm.pair_cd(k)
    if not hm.found(c, d, dbits):
        return 0, 0, [0] * 19
    sp = d * S % L
    lo, hi = sp % (1 << BW_SHIFT), sp >> BW_SHIFT
    assert lo >> 128 < 2**16 and hi < 2**109
    return 1, int(d < 0), words(c, 5) + words(abs(d), 5) + words(lo, 5) + words(hi, 4)


# ---- inputs --------------------------------------------------------------------

S_EDGES = [0, 1, L - 1, L, L + 1, 2**252, 2**253 - 1, 2**256 - 1]
MSG_EDGES = [0, 47, 48, 111, 112, 175, 176]      # SHA-512 padding edges of R || A || M
MSG_BUCKET_EDGES = [7855, 7856]                  # (msg_sz + 208) >> 7 == 62 | 63: the sort's last bucket
MSG_LONG = 20000                                 # beyond the clamp


def sort_bucket(msg_sz):
    """the hash order's key: SHA-512 blocks of R || A || M, clamped to the last bucket"""
    return min((msg_sz + 208) >> 7, 63)


@functools.lru_cache(maxsize=None)
def point_pool():
    """encodings for R and A: test_hsdec's edge encodings, the fixtures'
    points, and y with x = 0 under the sign bit (1, p - 1, and the
    non-canonical p + 1)"""
    from test_hsdec import edge_encodings
    out = list(edge_encodings())
    for name in ("adversarial", "mixed_order", "vectors"):
        d = load_golden(name)
        for i in range(min(48, len(d["msg_sz"]))):
            out += [d["pubs"][i].tobytes(), d["sigs"][i][:32].tobytes()]
    for yv in (1, P - 1, P + 1):
        out += [(yv | (1 << 255)).to_bytes(32, "little")] * 4
    return tuple(out)


@functools.lru_cache(maxsize=None)
def digest_ks():
    """(the k the search's tests chose for their quotients -- reduced mod L,
    as a digest's is --, the fixtures' k without a 131-bit pair and random k)"""
    edge = hm.quotient_edge_ks() + hm.golden_ratio_ks() + [k for k, _, _ in hm.big_quotient_ks()]
    rest = hm.fixture_ks(("halfsize", "longd")) + hm.random_ks(100, seed=41)
    return tuple(k % L for k in edge), tuple(rest)


def _draw_s(rng):
    return rng.choice(S_EDGES) if rng.random() < 0.4 else rng.randrange(L)


def _draw_points(rng, n, sigs, pubs):
    pool = point_pool()
    for i in range(n):
        sigs[i, :32] = np.frombuffer(rng.choice(pool), np.uint8)
        pubs[i] = np.frombuffer(rng.choice(pool), np.uint8)
        sigs[i, 32:] = np.frombuffer(_draw_s(rng).to_bytes(32, "little"), np.uint8)


def build_hashed(n, seed, big_at=(2, 30, 31)):
    """n signatures with messages: all but a few under 64 bytes, one in eight
    at a padding edge, the bucket edges and the long one at big_at (and a few
    more further on), every message at its own byte alignment"""
    rng = random.Random(seed)
    sigs, pubs = np.zeros((n, 64), np.uint8), np.zeros((n, 32), np.uint8)
    _draw_points(rng, n, sigs, pubs)
    big = dict(zip(big_at, (MSG_LONG, *MSG_BUCKET_EDGES)))
    for j, sz in enumerate((MSG_LONG, *MSG_BUCKET_EDGES, *MSG_BUCKET_EDGES)):
        big[300 + 777 * j] = sz
    msg_sz = np.array([big.get(i, rng.choice(MSG_EDGES) if rng.randrange(8) == 0 else rng.randrange(64))
                       for i in range(n)], np.uint32)
    msg_off, pos = np.zeros(n, np.uint64), 0
    for i in range(n):
        pos += (i - pos) % 4 if i < 64 else (rng.randrange(4) - pos) % 4   # the first 64: alignment i % 4
        msg_off[i] = pos
        pos += int(msg_sz[i]) + rng.randrange(3)
    msgs = np.frombuffer(rng.getrandbits(8 * (pos + 1)).to_bytes(pos + 1, "little"), np.uint8)
    return dict(n=n, sigs=sigs, pubs=pubs, msgs=msgs, msg_off=msg_off, msg_sz=msg_sz, digests=None)


def build_digests(n, seed):
    """n signatures with digests k + t L, t = 0, 1 and the largest below
    2^512: every third k from the search's edge list, the others from the
    fixtures and random draws, each list walked in a shuffled order so that
    all of it is reached"""
    rng = random.Random(seed)
    sigs, pubs = np.zeros((n, 64), np.uint8), np.zeros((n, 32), np.uint8)
    _draw_points(rng, n, sigs, pubs)
    lists = []
    for ks in digest_ks():
        ent = [k + t * L for k in ks for t in (0, 1, (2**512 - 1 - k) // L)]
        rng.shuffle(ent)
        lists.append(ent)
    digests = np.zeros((n, 64), np.uint8)
    for i in range(n):
        ent = lists[0] if i % 3 == 0 else lists[1]
        v = ent[(i // 3 if i % 3 == 0 else i - i // 3 - 1) % len(ent)]
        assert v < 2**512
        digests[i] = np.frombuffer(v.to_bytes(64, "little"), np.uint8)
    return dict(n=n, sigs=sigs, pubs=pubs, msgs=None, msg_off=None, msg_sz=None, digests=digests)


def from_fixture(d, count=None):
    """a golden fixture's signatures as inputs (its own messages)"""
    n = len(d["msg_sz"]) if count is None else count
    return dict(n=n, sigs=np.ascontiguousarray(d["sigs"][:n]), pubs=np.ascontiguousarray(d["pubs"][:n]),
                msgs=np.ascontiguousarray(d["msgs"]), msg_off=np.ascontiguousarray(d["msg_off"][:n], np.uint64),
                msg_sz=np.ascontiguousarray(d["msg_sz"][:n], np.uint32), digests=None)


def window(inp, start, n):
    """signatures start .. start + n (wrapping) of a set of inputs; the message bytes stay whole"""
    idx = np.arange(start, start + n) % inp["n"]
    out = dict(inp, n=n, sigs=np.ascontiguousarray(inp["sigs"][idx]), pubs=np.ascontiguousarray(inp["pubs"][idx]))
    for f in ("msg_off", "msg_sz", "digests"):
        if inp[f] is not None:
            out[f] = np.ascontiguousarray(inp[f][idx])
    return out, idx


def k_of(inp, i):
    if inp["digests"] is not None:
        return int.from_bytes(inp["digests"][i].tobytes(), "little") % L
    off, sz = int(inp["msg_off"][i]), int(inp["msg_sz"][i])
    h = hashlib.sha512(inp["sigs"][i, :32].tobytes() + inp["pubs"][i].tobytes() + inp["msgs"][off:off + sz].tobytes())
    return int.from_bytes(h.digest(), "little") % L


def s_of(inp, i):
    return int.from_bytes(inp["sigs"][i, 32:].tobytes(), "little")


class Model:
    """the expected arrays of a set of inputs, stride n; the parts that do
    not depend on the engine are computed once, scalars(dbits) and
    points(avx) on demand and kept"""

    def __init__(self, inp):
        n = self.n = inp["n"]
        self.ks = [k_of(inp, i) for i in range(n)]
        self.Ss = [s_of(inp, i) for i in range(n)]
        self.k = np.array([words(k, 8) for k in self.ks], np.uint32).T.reshape(8, n)
        self.sflag = np.array([int(S < L) for S in self.Ss], np.uint8)
        self.enc = [(inp["pubs"][i].tobytes(), inp["sigs"][i, :32].tobytes()) for i in range(n)]   # A, R
        self._sc, self._pt = {}, {}

    def scalars(self, dbits):
        """found [n], dneg [n], hs [19][n]"""
        if dbits not in self._sc:
            rows = [scalar_rows(k, S, dbits) for k, S in zip(self.ks, self.Ss)]
            self._sc[dbits] = (np.array([r[0] for r in rows], bool), np.array([r[1] for r in rows], np.uint8),
                               np.array([r[2] for r in rows], np.uint32).T.reshape(19, self.n))
        return self._sc[dbits]

    def points(self, avx):
        """pflag [2][n], y limbs [2][10][n], x values [2][n] (Python integers)"""
        if avx not in self._pt:
            pf, y, x = np.zeros((2, self.n), np.uint8), np.zeros((2, 10, self.n), np.int32), np.zeros((2, self.n), object)
            for i, pair in enumerate(self.enc):
                for which, enc in enumerate(pair):
                    pf[which, i], x[which, i], yr = expected_kept(enc, bool(avx))
                    y[which, :, i] = y_limbs(yr)
            self._pt[avx] = (pf, y, x)
        return self._pt[avx]

    def take(self, idx):
        """the model of window(inp, ...)'s signatures"""
        m = Model.__new__(Model)
        m.n, m.ks, m.Ss, m.enc = len(idx), [self.ks[i] for i in idx], [self.Ss[i] for i in idx], [self.enc[i] for i in idx]
        m.k, m.sflag = self.k[:, idx], self.sflag[idx]
        m._sc = {b: (f[idx], g[idx], h[:, idx]) for b, (f, g, h) in self._sc.items()}
        m._pt = {a: (pf[:, idx], y[:, :, idx], x[:, idx]) for a, (pf, y, x) in self._pt.items()}
        return m


def classes(model, dbits, avx):
    """how often each class the builder claims occurs, from the model alone"""
    found, dneg, _ = model.scalars(dbits)
    pf, _, _ = model.points(avx)
    S = model.Ss
    out = {}
    for which, side in enumerate("AR"):
        out[side + " accepted"] = int((pf[which] == 0).sum())
        out[side + " no root"] = int(((pf[which] & PF_FAIL) != 0).sum())
        out[side + " small order"] = int(((pf[which] & PF_SMALL) != 0).sum())
    out["d < 0 with S = 0"] = sum(1 for i in range(model.n) if found[i] and dneg[i] and S[i] == 0)
    nopair = [i for i in range(model.n) if not found[i]]
    out["no pair"] = len(nopair)
    out["no pair, distinct k"] = len({model.ks[i] for i in nopair})
    out["no pair with S >= L"] = sum(1 for i in nopair if S[i] >= L)
    out["no pair with S < L"] = sum(1 for i in nopair if S[i] < L)
    return out


# ---- the sets the tests share ----------------------------------------------------

POOL_N = 4200
SIZES = {"wide": (1, 255, 256, 257, 4095, 4096, 4097),   # the decode grid's A / R boundary inside a wave, one sort block +- 1
         "fused": (1, 63, 64, 65, 129),
         "r16": (1, 2, 3, 4, 5, 31, 32, 33, 64, 65)}     # prep16: four points a decode wave, 32 signatures a hash block


@functools.lru_cache(maxsize=None)
def pool(mode):
    """(inputs, model) of POOL_N signatures, mode "hashed" or "digests"; every launch of the tests is a window of one"""
    inp = build_hashed(POOL_N, 11) if mode == "hashed" else build_digests(POOL_N, 12)
    return inp, Model(inp)


def windows(kind, nmax=None):
    """(n, cap, start) of every launch of a form: each size with cap = n from
    the pool's start (the long messages) and with cap = n + 3 from elsewhere"""
    out = []
    for i, n in enumerate(SIZES[kind]):
        n = n if nmax is None else min(n, nmax)
        out += [(n, n, 0), (n, n + 3, 64 + 97 * i)]
    return out


def union_model(mode, kind):
    """the model of every signature some launch of the form sees"""
    inp, model = pool(mode)
    seen = sorted({int(j) for n, _, start in windows(kind) for j in np.arange(start, start + n) % inp["n"]})
    return model.take(np.array(seen))
