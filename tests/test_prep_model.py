"""The model and the inputs of tests/test_gpu_prep_diag.py, pinned without a
GPU: fd_ed25519_hip_private_diag_prep_check's refusals one by one; the
classes the input builder claims, counted with the model alone; and the
model's records and points against the host's own (hsrec, hsdec), which the
device's are documented to equal.  CPU only."""
import ctypes

import numpy as np
import pytest

import half_euclid_model as hm
import prep_model as pm
from prep_model import L
from test_half_euclid import lib as half_lib   # noqa: F401  (the CPU harness of fd25519_half.h, a fixture)

INVAL = -22   # FD_ED25519_HIP_ERR_INVAL (include/fd_ed25519_hip.h)


@pytest.fixture(scope="module")
def lib():
    from firedancer_amd import ed25519
    return ed25519.library()


def check(lib, form=0, n=4, n_max=8, cap=4, sigs=True, pubs=True, msgs=True, msg_off=True, msg_sz=True, digests=None,
          shift=(0, 0, 0), sizes=None):
    """the check function on real arrays; a False argument passes NULL, shift moves sigs / pubs / digests off their alignment"""
    keep = [np.zeros(64 * 16 + 16, np.uint8), np.zeros(32 * 16 + 16, np.uint8), np.zeros(64, np.uint8),
            np.zeros(16, np.uint64), np.array(sizes if sizes is not None else [3] * 16, np.uint32),
            np.zeros(64 * 16 + 16, np.uint8)]

    def ptr(a, on, sh=0):
        assert a.ctypes.data % 16 == 0
        return ctypes.c_void_p(a.ctypes.data + sh) if on else None
    return lib.fd_ed25519_hip_private_diag_prep_check(form, n, n_max, cap, ptr(keep[0], sigs, shift[0]),
                                                      ptr(keep[1], pubs, shift[1]), ptr(keep[2], msgs),
                                                      ptr(keep[3], msg_off), ptr(keep[4], msg_sz),
                                                      ptr(keep[5], digests, shift[2]))


def test_check_accepts_what_it_should(lib):
    for form in range(6):
        assert check(lib, form=form) == 0
        assert check(lib, form=form, digests=True, msgs=False, msg_off=False, msg_sz=False) == 0
    assert check(lib, n=8, cap=8) == 0 and check(lib, n=1, cap=1) == 0 and check(lib, cap=7) == 0
    assert check(lib, msgs=False, sizes=[0] * 16) == 0            # no bytes to read
    assert check(lib, sizes=[0x7fffffff] * 16) == 0               # FD_ED25519_HIP_MSG_SZ_MAX itself


@pytest.mark.parametrize("what,kw", [
    ("form below", dict(form=-1)), ("form above", dict(form=6)),
    ("n == 0", dict(n=0)), ("n above n_max", dict(n=9, cap=9)), ("the form unavailable", dict(n_max=0)),
    ("cap < n", dict(cap=3)),
    ("sigs NULL", dict(sigs=False)), ("pubs NULL", dict(pubs=False)),
    ("sigs misaligned", dict(shift=(8, 0, 0))), ("pubs misaligned", dict(shift=(0, 4, 0))),
    ("digests misaligned", dict(digests=True, shift=(0, 0, 1))),
    ("no digests, no msg_off", dict(msg_off=False)), ("no digests, no msg_sz", dict(msg_sz=False)),
    ("no msgs but bytes to read", dict(msgs=False)),
    ("msg_sz above the device hash's", dict(sizes=[3, 3, 3, 0x80000000] + [3] * 12)),
])
def test_check_refuses(lib, what, kw):
    assert check(lib, **kw) == INVAL, what


def test_check_reads_only_n_sizes(lib):
    assert check(lib, n=3, cap=3, sizes=[3, 3, 3, 0x80000000] + [3] * 12) == 0


def harness_cd(so, ks, dbits):
    kw = hm.k_array(ks)
    out = np.zeros((len(ks), 12), dtype=np.uint32)
    so.half_scalars_batch(kw.ctypes.data, len(ks), dbits, out.ctypes.data)
    return [hm.unpack(o) for o in out]


@pytest.mark.parametrize("kind", ["wide", "fused", "r16"])
@pytest.mark.parametrize("mode", ["hashed", "digests"])
def test_every_decode_test_meets_every_point_class(kind, mode):
    m = pm.union_model(mode, kind)
    for avx in (True, False):
        got = pm.classes(m, 151, avx)
        for side in "AR":
            for cls in ("accepted", "no root", "small order"):
                assert got[f"{side} {cls}"] >= 8, (kind, mode, avx, got)
    # the encodings no valid signature can carry: y >= p on either side
    noncanon = [sum(1 for pair in m.enc if int.from_bytes(pair[w], "little") & (2**255 - 1) >= pm.P) for w in (0, 1)]
    assert min(noncanon) >= 8, noncanon


def test_digest_pool_classes_at_151_bits(half_lib):   # noqa: F811
    inp, m = pm.pool("digests")
    got = pm.classes(m, 151, True)
    assert got["d < 0 with S = 0"] >= 1
    assert got["no pair, distinct k"] >= 10 and got["no pair with S >= L"] >= 5 and got["no pair with S < L"] >= 5
    found = m.scalars(151)[0]
    nopair = sorted({m.ks[i] for i in range(m.n) if not found[i]})
    left = harness_cd(half_lib, nopair, 151)
    assert not any(f for f, _, _ in left)
    long_c = sum(1 for _, c, _ in left if c.bit_length() > 131)
    long_d = sum(1 for _, _, d in left if abs(d).bit_length() > 151)
    print(f"151 bits: {len(nopair)} k without a pair, {long_c} leave c above 131 bits, {long_d} |d| above 151")
    assert long_c >= 5
    # The search's edge lists hold 33 such k as they stand (16 with a long
    # c), seven of them above L; a digest is reduced first, which turns those
    # seven into other k: 34 and 19 of what the device can see.
    raw = hm.quotient_edge_ks() + [k for k, _, _ in hm.big_quotient_ks()]
    raw_nopair = [k for k in raw if not hm.found(*hm.pair_cd(k), 151)]
    assert len(raw_nopair) == 33 and sum(1 for _, c, _ in harness_cd(half_lib, raw_nopair, 151) if c.bit_length() > 131) == 16
    assert (len(nopair), long_c) == (34, 19)


def test_digest_pool_classes_at_131_bits():
    inp, m = pm.pool("digests")
    got = pm.classes(m, 131, True)
    assert got["d < 0 with S = 0"] >= 1
    assert got["no pair, distinct k"] >= 100   # halfsize.npz's, all without a strict pair
    assert got["no pair with S >= L"] >= 5 and got["no pair with S < L"] >= 5


@pytest.mark.parametrize("kind", ["fused", "r16"])
def test_small_launches_meet_the_scalar_classes_too(kind):
    m = pm.union_model("digests", kind)
    for dbits in (151, 131):
        got = pm.classes(m, dbits, True)
        assert got["no pair with S >= L"] >= 2 and got["no pair with S < L"] >= 2, (kind, dbits, got)


def test_digest_multiples_of_l():
    inp, m = pm.pool("digests")
    vals = [int.from_bytes(inp["digests"][i].tobytes(), "little") for i in range(m.n)]
    ts = {(v - k) // L for v, k in zip(vals, m.ks)}
    assert {0, 1} <= ts and max(vals) + L >= 2**512 and all((v - k) % L == 0 for v, k in zip(vals, m.ks))


def test_hashed_pool_messages():
    inp, _ = pm.pool("hashed")
    sz, off = inp["msg_sz"], inp["msg_off"]
    assert set(pm.MSG_EDGES + pm.MSG_BUCKET_EDGES + [pm.MSG_LONG]) <= set(sz.tolist())
    assert (sz >= 64).sum() < len(sz) // 6
    for s in set(pm.MSG_EDGES):   # every edge size at every alignment
        assert {int(o) % 4 for o, z in zip(off, sz) if z == s} == {0, 1, 2, 3}, s
    assert {pm.sort_bucket(int(s)) for s in sz} >= {1, 2, 3, 62, 63}
    ends = sorted((int(o), int(o) + int(z)) for o, z in zip(off, sz))
    assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:])) and ends[-1][1] <= len(inp["msgs"])


def test_s_pool_reached():
    for mode in ("hashed", "digests"):
        _, m = pm.pool(mode)
        assert set(pm.S_EDGES) <= set(m.Ss) and sum(1 for S in m.Ss if S not in pm.S_EDGES) > m.n // 2


@pytest.mark.parametrize("dbits", [151, 131])
def test_model_records_equal_the_hosts(lib, halfsize, dbits):
    """hsrec on the hashed pool and on halfsize.npz: the same k, sflag, pair, sign and split s'"""
    f = lib.fd_ed25519_hip_private_hsrec
    f.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_ulong, ctypes.c_int, ctypes.c_void_p]
    f.restype = ctypes.c_int
    seen = {"record": 0, "declined": 0, "S >= L without a pair": 0}
    for inp, m in (pm.pool("hashed"), (lambda i: (i, pm.Model(i)))(pm.from_fixture(halfsize))):
        found, dneg, hs = m.scalars(dbits)
        for i in range(m.n):
            off, sz = int(inp["msg_off"][i]), int(inp["msg_sz"][i])
            rec = np.zeros(32, np.uint32)
            ok = f(inp["sigs"][i].tobytes(), inp["pubs"][i].tobytes(), inp["msgs"][off:off + sz].tobytes(), sz, dbits,
                   rec.ctypes.data)
            assert ok == int(found[i] or not m.sflag[i]), i
            if not ok:
                seen["declined"] += 1
                continue
            assert rec[:8].tolist() == m.k[:, i].tolist() and rec[27] == m.sflag[i]
            if found[i]:
                seen["record"] += 1
                assert rec[8:27].tolist() == hs[:, i].tolist() and rec[28] == dneg[i], i
            else:   # the host never stores an unverified pair: c = 0, d = 1, s' = S mod L
                seen["S >= L without a pair"] += 1
                sp = m.Ss[i] % L
                assert rec[8:27].tolist() == pm.words(0, 5) + pm.words(1, 5) + pm.words(sp % 2**144, 5) + \
                    pm.words(sp >> 144, 4) and rec[28] == 0
    assert seen["record"] > 1000 and (dbits == 151 or (seen["declined"] > 50 and seen["S >= L without a pair"] > 5)), seen


@pytest.mark.parametrize("avx", [True, False])
def test_model_points_equal_the_hosts(lib, avx):
    """hsdec_n on both pools' encodings: flags, y limbs, x mod p where the decode did not fail"""
    f = lib.fd_ed25519_hip_private_hsdec_n
    f.argtypes = [ctypes.c_void_p, ctypes.c_ulong, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    f.restype = None
    for mode in ("hashed", "digests"):
        _, m = pm.pool(mode)
        pf, y, x = m.points(avx)
        encs = [e for pair in m.enc for e in pair]
        bufs = [ctypes.create_string_buffer(e, 32) for e in encs]
        arr = (ctypes.c_void_p * len(bufs))(*[ctypes.addressof(b) for b in bufs])
        pt, fl = np.zeros((len(encs), 20), np.int32), np.zeros(len(encs), np.uint8)
        f(ctypes.addressof(arr), len(encs), 1 if avx else 0, pt.ctypes.data, fl.ctypes.data)
        assert fl.reshape(-1, 2).T.tolist() == pf.tolist()
        assert pt[:, 10:].reshape(-1, 2, 10).transpose(1, 2, 0).tolist() == y.tolist()
        got = pm.limbs_value(pt[:, :10].T).reshape(-1, 2).T
        ok = (pf & pm.PF_FAIL) == 0
        assert ok.sum() > m.n and (got[ok] == x[ok]).all()
