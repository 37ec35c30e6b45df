"""Device scalar arithmetic on chosen inputs (libfd_ed25519_diag.so):
sc_reduce512, sc_is_canonical and the signed-window recodings of
fd25519_sc.h / fd25519_dsm.h, and the digit prologue of dsm_half_one,
against Python integers.

A verify only ever feeds these a hash output or a product of one, so
multiples of L +- 1, residues in [2^252, L) (where digit 11 of the reduced
value is exactly 2^21), digit patterns at the centered carries' rounding
boundary, a carry that ripples through every window, a top digit of
exactly 8 and |d| of exactly dbits bits are never reached that way.  All
comparisons are exact and every case is checked."""
import random

import pytest

from diag_util import HIP_ERROR_INVALID_VALUE, L, Diag, from_words, s32, scalar_edges_512, scalar_edges_lt_l, words

pytestmark = pytest.mark.gpu

DBITS_MAX = 151                    # fd25519_half.h FD_HALF_DBITS_MAX
WMAX = (DBITS_MAX + 4) // 4        # 38 windows


@pytest.fixture(scope="module")
def diag():
    return Diag()


def test_sc_reduce512(diag):
    xs = scalar_edges_512(random.Random(51))
    out = diag.run("sc", "reduce512", [words(x, 16) for x in xs])
    for x, o in zip(xs, out):
        got = from_words(o[:8])
        assert got < L, hex(x)
        assert got == x % L, (hex(x), hex(got))
    print(f"sc_reduce512: {len(xs)} cases")


def test_sc_is_canonical(diag):
    xs = [0, 1, 2**256 - 1, 2**252, 2**252 - 1, 2**253]
    xs += [L + d for d in (-2, -1, 0, 1, 2)]
    for w in range(8):
        for d in (-1, 1):
            wl = words(L, 8)
            wl[w] = (wl[w] + d) & 0xffffffff
            xs.append(from_words(wl))
    out = diag.run("sc", "is_canonical", [words(x, 8) for x in xs])
    for x, o in zip(xs, out):
        assert int(o[0]) == (1 if x < L else 0), hex(x)
    print(f"sc_is_canonical: {len(xs)} cases")


# radix bits -> (digits, (lo, hi) of a digit, (lo, hi) of the top digit), as
# the comments above recode_radix16 / 256 / 65536 state them (fd25519_dsm.h)
RECODE = {4: ("recode16", 64, (-8, 7), (0, 2)),
          8: ("recode256", 32, (-128, 127), (0, 17)),
          16: ("recode65536", 16, (-2**15, 2**15), (0, 2**13 + 1))}


@pytest.mark.parametrize("bits", [4, 8, 16])
def test_recode_radix(diag, bits):
    op, nd, (lo, hi), (tlo, thi) = RECODE[bits]
    xs = scalar_edges_lt_l(random.Random(52))
    out = diag.run("sc", op, [words(x, 8) for x in xs])
    for x, o in zip(xs, out):
        d = [s32(v) for v in o[:nd]]
        assert all(lo <= v <= hi for v in d[:-1]), (hex(x), d)
        assert tlo <= d[-1] <= thi, (hex(x), d)
        assert sum(v << (bits * i) for i, v in enumerate(d)) == x, (hex(x), d)
    print(f"recode_radix{1 << bits}: {len(xs)} cases")


def digits160_cases():
    rng = random.Random(53)
    pat8 = sum(8 << (4 * i) for i in range(40))
    pat7 = sum(7 << (4 * i) for i in range(40))
    cs = [0, 1, 2**131 - 1, 2**130, pat8 % 2**131, pat7 % 2**131, pat8 % 2**130, 2**131 - 8, 2**131 - 9]
    cs += [rng.randrange(2**131) for _ in range(40)]
    ds = list(cs)
    for dbits in (131, 151):        # exactly dbits bits, odd
        ds += [2**(dbits - 1) + 1, 2**dbits - 1, (pat8 % 2**(dbits - 1)) | 2**(dbits - 1) | 1,
               (pat7 % 2**(dbits - 1)) | 2**(dbits - 1) | 1]
        ds += [rng.getrandbits(dbits - 1) | 2**(dbits - 1) | 1 for _ in range(20)]
    for b in range(131, 152):       # every top-window position
        ds += [2**b - 1, 2**(b - 1), pat8 % 2**b]
    cases = []
    for W in range(33, WMAX + 1):
        # a lane's windows: |d| < 2^(4W-1) (fd_ed25519_kernels.hip, dsm_half_one)
        fit = [d for d in ds if d < 2**(4 * W - 1)]
        for i, d in enumerate(fit):
            cases.append((cs[i % len(cs)], d, W))
        for c in cs:
            cases.append((c, fit[-1], W))
    return cases


def test_digits160(diag):
    cases = digits160_cases()
    assert {W for _, _, W in cases} == set(range(33, WMAX + 1))
    out = diag.run("digits160", "digits", [words(c, 5) + words(d, 5) + [W] for c, d, W in cases])
    top8 = 0
    for (c, d, W), o in zip(cases, out):
        for v, dig in ((c, o[:40]), (d, o[40:80])):
            e = [s32(x) for x in dig]
            assert not any(e[W:]), (hex(v), W, e)
            assert all(-8 <= x <= 7 for x in e[:W - 1]), (hex(v), W, e)
            assert 0 <= e[W - 1] <= 8, (hex(v), W, e)
            assert sum(x << (4 * i) for i, x in enumerate(e[:W])) == v, (hex(v), W, e)
            top8 += e[W - 1] == 8
    assert top8 > 0     # the top digit of exactly 8, read unsigned, is among the cases
    print(f"digits160: {len(cases)} cases, {top8} top digits of 8")


def test_entry_points_reject_bad_arguments(diag):
    import numpy as np
    inp, out = np.zeros((4, 128), np.uint32), np.zeros((4, 128), np.uint32)
    for fam in ("fe", "r16", "sc", "ge", "ge4", "ge16", "digits160"):
        assert diag.raw(fam, -1, inp, out, 1) == HIP_ERROR_INVALID_VALUE
        assert diag.raw(fam, 99, inp, out, 1) == HIP_ERROR_INVALID_VALUE
        assert diag.raw(fam, 0, inp, out, (1 << 20) + 1) == HIP_ERROR_INVALID_VALUE
    assert diag.raw("digits160", 0, inp, out, 1) == HIP_ERROR_INVALID_VALUE     # W = 0
    assert diag.raw("sc", 0, inp, out, 0) == 0                                   # nothing to do
