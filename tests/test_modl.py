"""The host's x mod L (host/fd_ed25519_hip_hsrec.cc mod_l, through
fd_ed25519_hip_private_mod_l) against Python's % L, on inputs that take
its "add L back" branch.

mod_l goes word by word from the top: t = r 2^32 + w, q = t >> 252 is
floor(t / L) or one more, and a borrow out of t - q L adds L back.  For a
hash the estimate is one too many with probability about 2^-94 per step,
so hash-derived inputs miss that branch (the fixtures of
tests/test_hsrec.py reach it only through some of their d S products,
not by design).  It is
taken exactly when t mod L >= L - q (L - 2^252): inputs built as
((m L - j) << 32 s) | low have a prefix just below a multiple of L and
take it when the prefix's last word comes in.  The test restates the
estimate in Python and asserts that the branch is in fact reached, at the
last step and at earlier ones, so the edge cannot drop out of the input set
unnoticed.  CPU only."""
import ctypes
import random

import numpy as np
import pytest

from diag_util import L, from_words, scalar_edges_512, words


@pytest.fixture(scope="module")
def mod_l():
    from firedancer_amd import ed25519
    f = ed25519.library().fd_ed25519_hip_private_mod_l
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    f.restype = None

    def run(x, n):
        inp = np.array(words(x, n), dtype=np.uint32)
        out = np.zeros(8, dtype=np.uint32)
        f(out.ctypes.data, inp.ctypes.data, n)
        return from_words(out)
    return run


def addback_steps(x, n):
    """the steps (word index, from the top) at which the loop's estimate
    t >> 252 exceeds t // L"""
    r, hit = 0, []
    for i in range(n - 1, -1, -1):
        t = (r << 32) | ((x >> (32 * i)) & 0xffffffff)
        q = t >> 252
        assert q - t // L in (0, 1)
        if q != t // L:
            hit.append(i)
        r = t % L
    return hit


def nwords(x):
    return max(1, (x.bit_length() + 31) // 32)


def built_inputs():
    rng = random.Random(44)
    out = []
    for s in range(9):
        for m in (1, 2, 5, 2**31, 2**32 - 1):
            for j in (1, 2, 1000):
                for low in (0, (1 << (32 * s)) - 1, rng.getrandbits(32 * s) if s else 0):
                    out.append((((m * L - j) << (32 * s)) | low))
    # m L has up to 285 bits: every s fits the 16 words but s = 8 with the two largest m
    return [x for x in out if nwords(x) <= 16]


def test_mod_l_matches_python_and_takes_the_add_back_branch(mod_l):
    rng = random.Random(43)
    cases = []
    for x in scalar_edges_512(rng, 500):
        cases.append((x, nwords(x)))
        cases.append((x, 16))
    for x in built_inputs():
        cases.append((x, nwords(x)))
        cases.append((x, min(16, nwords(x) + 1)))      # a zero top word
    for n in range(1, 17):
        cases += [(rng.getrandbits(32 * n), n) for _ in range(20)]
        cases += [((1 << (32 * n)) - 1, n), (0, n), (L % (1 << (32 * n)), n)]
    assert {n for _, n in cases} == set(range(1, 17))
    hit_any = hit_early = 0
    for x, n in cases:
        assert 0 <= x < 1 << (32 * n)
        got = mod_l(x, n)
        assert got == x % L, (hex(x), n, hex(got))
        steps = addback_steps(x, n)
        hit_any += bool(steps)
        hit_early += any(i > 0 for i in steps)
    print(f"mod_l: {len(cases)} inputs, {hit_any} take the add-back branch, {hit_early} before the last step")
    assert hit_any >= 100
    assert hit_early >= 1


def test_every_built_input_takes_the_branch():
    for x in built_inputs():
        assert addback_steps(x, nwords(x)), hex(x)
