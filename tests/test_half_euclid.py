"""The half-size scalar search (csrc/fd25519_half.h) on the host against an
independent big-integer Euclid (tests/half_euclid_model.py): the same found,
c, |d| and sign, at dbits 131 and 151, for the fixtures' k, the edges of
[0, L), first quotients at and beyond the bound of every quotient estimate
(2^20 single precision, 2^30 the fused 32-bit update, 2^52 the leading
bits), the golden-ratio k, one large quotient at every position of the
expansion and 200,000 random k.  The same comparison then runs once as a
stand-alone program built with the address and undefined-behaviour
sanitizers.  CPU only."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import half_euclid_model as hm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "half_euclid_harness.cpp")
INC = os.path.join(REPO, "firedancer_amd", "csrc")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("half_euclid") / "half_euclid.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-I", INC, SRC, "-o", out])
    so = ctypes.CDLL(out)
    so.half_scalars_batch.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]
    so.half_scalars_batch.restype = None
    so.half_hook_counts.argtypes = [ctypes.c_void_p] * 2
    so.half_hook_counts.restype = None
    return so


def hook_counts(so):
    """(steps accepted from leading bits, those that were not true Euclidean
    steps of the whole integers) so far, as the harness redid them"""
    steps, bad = ctypes.c_uint64(), ctypes.c_uint64()
    so.half_hook_counts(ctypes.addressof(steps), ctypes.addressof(bad))
    return steps.value, bad.value


def batch(so, ks, dbits):
    kw = hm.k_array(ks)
    out = np.zeros((len(ks), 12), dtype=np.uint32)
    so.half_scalars_batch(kw.ctypes.data, len(ks), dbits, out.ctypes.data)
    return out


def compare(so, ks):
    """every k at both bounds; returns how many were found at each.  Every
    step the one-quotient inner loop accepted on the way must be a true
    Euclidean step (the harness redoes each on the whole integers)."""
    want = [hm.pair_cd(k) for k in ks]
    n_found = []
    for dbits in hm.DBITS:
        out = batch(so, ks, dbits)
        cnt = 0
        for k, (c, d), o in zip(ks, want, out):
            f = hm.found(c, d, dbits)
            got_f, got_c, got_d = hm.unpack(o)
            assert got_f == f, (hex(k), dbits, got_f, f)
            if f:
                cnt += 1
                assert (got_c, got_d) == (c, d), (hex(k), dbits)
        n_found.append(cnt)
    steps, bad = hook_counts(so)
    assert bad == 0, bad
    return n_found


def test_fixture_k(lib):
    ks = hm.fixture_ks()
    strict, ext = compare(lib, ks)
    assert strict < ext <= len(ks)   # halfsize.npz and longd.npz are the k without a strict pair


def test_edges_of_the_range(lib):
    compare(lib, [0, 1, 2, hm.L - 1])


def test_first_quotient_at_every_estimate_bound(lib):
    ks = hm.quotient_edge_ks()
    for k in ks:
        assert 0 < k < hm.N8L
    compare(lib, ks)


def test_golden_ratio_k(lib):
    ks = hm.golden_ratio_ks()
    assert set(hm.pair(ks[1])[2]) == {1}   # every quotient down to 2^131 is 1
    compare(lib, ks)


def test_big_quotient_at_every_position(lib):
    cases = hm.big_quotient_ks()
    seen = set()
    for k, pos, big in cases:
        qs = hm.pair(k)[2]
        if pos < len(qs):
            assert qs[pos] in (big, big - 1, big + 1), (pos, qs[pos], big)   # the rounding of k may move it by one
            seen.add(pos)
    # the walk from 2^255 to 2^131 passes at least 40 quotients even with a 2^30 among them
    assert set(range(40)) <= seen
    compare(lib, [k for k, _, _ in cases])


@pytest.mark.parametrize("part", range(4))
def test_random_k(lib, part):
    ks = hm.random_ks(50000, seed=100 + part)
    strict, ext = compare(lib, ks)
    assert 0 < len(ks) - strict < 0.004 * len(ks)   # ~0.16% need |d| >= 2^131
    assert ext >= len(ks) - 2                        # ~1e-6 beyond 151 bits


def test_accepted_steps_are_most_of_the_walk(lib):
    """the hook is live: of the ~72 steps from 2^255 to 2^131 the rounds take
    nearly all from leading bits"""
    ks = hm.random_ks(2000, seed=9)
    s0 = hook_counts(lib)[0]
    batch(lib, ks, 151)
    steps, bad = hook_counts(lib)
    total = sum(len(hm.pair(k)[2]) for k in ks)
    assert bad == 0 and 0.97 * total <= steps - s0 <= total, (steps - s0, total)


def test_sanitized_program(tmp_path):
    """the same header and harness as a program of its own under ASan and
    UBSan, on the same k, at both bounds"""
    exe = str(tmp_path / "half_euclid_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-DHALF_EUCLID_MAIN",
                           "-I", INC, SRC, "-o", exe])
    ks = ([0, 1, 2, hm.L - 1] + hm.fixture_ks() + hm.quotient_edge_ks() + hm.golden_ratio_ks() +
          [k for k, _, _ in hm.big_quotient_ks()] + [k for part in range(4) for k in hm.random_ks(50000, seed=100 + part)])
    want = [hm.pair_cd(k) for k in ks]
    for dbits in hm.DBITS:
        path = str(tmp_path / ("cases%d.bin" % dbits))
        with open(path, "wb") as f:
            f.write(struct.pack("<Qii", len(ks), dbits, 0))
            for k, (c, d) in zip(ks, want):
                fnd = hm.found(c, d, dbits)
                rec = hm.words(k) + [fnd, int(d < 0)] + hm.words(c)[:5] + hm.words(abs(d) % 2**160)[:5]
                f.write(struct.pack("<20I", *rec))
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
        assert "%d records, 0 differ," % len(ks) in r.stdout and ", 0 not Euclidean" in r.stdout, r.stdout
