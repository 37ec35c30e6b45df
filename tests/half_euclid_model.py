"""The half-size pair of fd25519_half.h restated on Python integers, and the
inputs the search is checked on (tests/test_half_euclid.py on the host build,
tests/test_gpu_half_euclid.py on the device).

The pair: Euclid on (8L, k) to the first remainder r_i below 2^131;
(r_i, t_i) if t_i is odd, else (r_{i-1} - m r_i, t_{i-1} - m t_i) with the
least m that brings the first coordinate below 2^131; found iff d is odd,
0 <= c < 2^131 and |d| < 2^dbits."""
import functools
import hashlib
import math
import random

import numpy as np

from conftest import load_golden

L = 2**252 + 27742317777372353535851937790883648493
N8L = 8 * L
BITS = 131
DBITS = (131, 151)


def pair(k):
    """(c, d, quotients) of the rule above"""
    c, d, qs = _pair(k, [])
    return c, d, qs


@functools.lru_cache(maxsize=None)
def pair_cd(k):
    """(c, d) alone, kept: the tests share one reference"""
    return _pair(k, None)[:2]


def _pair(k, qs):
    r0, t0, r1, t1 = N8L, 0, k, 1
    lim = 1 << BITS
    while r1 >= lim:
        q, r = divmod(r0, r1)
        if qs is not None:
            qs.append(q)
        r0, t0, r1, t1 = r1, t1, r, t0 - q * t1
    if t1 & 1:
        return r1, t1, qs
    if r1 == 0:
        return 0, 0, qs   # d even: never found
    m = (r0 - lim) // r1 + 1 if r0 >= lim else 0
    return r0 - m * r1, t0 - m * t1, qs


def takes_fixup(k):
    """the cofactor of the first remainder below 2^131 is even: the pair
    comes from the (r_{i-1} - m r_i, ...) family"""
    t0, t1 = 0, 1
    r0, r1 = N8L, k
    while r1 >= 1 << BITS:
        q, r = divmod(r0, r1)
        r0, t0, r1, t1 = r1, t1, r, t0 - q * t1
    return t1 % 2 == 0


def found(c, d, dbits):
    return int(d % 2 != 0 and 0 <= c < 2**BITS and abs(d) < 2**dbits)


def words(k):
    return [(k >> (32 * i)) & 0xffffffff for i in range(8)]


def unpack(o):
    """(found, c, d) of the 12 words the harness and the device diagnostic write"""
    c = sum(int(o[2 + w]) << (32 * w) for w in range(5))
    d = sum(int(o[7 + w]) << (32 * w) for w in range(5))
    return int(o[0]), c, (-d if o[1] else d)


def fixture_ks(names=("halfsize", "longd", "adversarial", "mixed_order")):
    ks = []
    for nm in names:
        d = load_golden(nm)
        for i in range(len(d["msg_sz"])):
            off, sz = int(d["msg_off"][i]), int(d["msg_sz"][i])
            h = hashlib.sha512(d["sigs"][i][:32].tobytes() + d["pubs"][i].tobytes() + bytes(d["msgs"][off:off + sz]))
            ks.append(int.from_bytes(h.digest(), "little") % L)
    return ks


QUOTS = (2, 3, 2**20 - 1, 2**20, 2**20 + 1, 2**26, 2**40, 2**63)


def quotient_edge_ks():
    """floor(8L / q) and its neighbours: a first quotient at and beyond every
    estimate's bound (below 8L; those of q = 2, 3 are above L, which the
    search takes all the same: it only needs k < 8L)"""
    return [N8L // q + e for q in QUOTS for e in (-1, 0, 1)]


def golden_ratio_ks():
    """k nearest 8L / phi (every quotient 1 down to 2^131), and the nearest
    below L with the same tail (k / 8 phi: a first quotient of 12)"""
    s5 = math.isqrt(5 << 1200)                       # sqrt(5) 2^600
    inv_phi = (s5 - (1 << 600), 1 << 601)            # (sqrt(5) - 1) / 2
    k = (N8L * inv_phi[0] + inv_phi[1] // 2) // inv_phi[1]
    return [k - 1, k, k + 1, k // 13, (N8L * inv_phi[0]) // (inv_phi[1] * 8)]


def from_quotients(qs):
    """k = round(8L / [q1; q2, ...]): Euclid on (8L, k) starts with the
    quotients qs as long as the convergents' denominators stay far below
    sqrt(8L)"""
    h0, h1, k0, k1 = 1, qs[0], 0, 1
    for q in qs[1:]:
        h0, h1, k0, k1 = h1, q * h1 + h0, k1, q * k1 + k0
    return (N8L * k1 + h1 // 2) // h1


BIG_QUOTS = (2**20, 2**25 + 12345, 2**30 - 1, 2**30)


def big_quotient_ks(seed=7, positions=70):
    """One partial quotient of 2^20..2^30 at each position of the expansion
    that the search walks through (it takes ~60-75 steps of small quotients
    to come down from 2^255 to 2^131, 12-13 to a round): wherever a round
    begins, some k here has the big quotient first, second, ... in it.
    Returns (k, position, quotient) with the position counted from 0; the
    first quotient is at least 8 for k < L."""
    rng = random.Random(seed)
    out = []
    for pos in range(positions):
        big = BIG_QUOTS[pos % len(BIG_QUOTS)]
        qs = [rng.choice((1, 1, 1, 2, 2, 3, 4, 7)) for _ in range(pos)] + [big] + [1, 2, 1, 3]
        qs[0] = max(qs[0], 8) if pos else big
        out.append((from_quotients(qs), pos, big))
    return out


def random_ks(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(L) for _ in range(n)]


def k_array(ks):
    return np.array([words(k) for k in ks], dtype=np.uint32)
