"""The device signer's arithmetic on chosen operands (libfd_ed25519_diag.so,
firedancer_amd/csrc/diag/fd_ed25519_diag_sign.hip): ge_scalarmult_base,
ge_encode and mul256_add -- which fd_ed25519_sign_kernel alone calls -- and
the [0..128]B table that kernel alone reads, against Python integers
(tests/sign_model.py).

A signature only ever multiplies B by a SHA-512 output and only ever encodes
the result: digit -128 (table entry 128, negated), a zero digit after a
non-zero one, runs of leading zero digits, the top digit's whole range, a
product k a + r at the ends of its range or a multiple of L, a point with
x = 0 or y = p - 1 in an uncommon limb form are never reached that way.
tests/test_sign_cases.py asserts on the CPU what the case lists cover.  All
comparisons are exact and every case is checked."""
import ctypes
import random

import numpy as np
import pytest

import bounds_model as bm
import diag_util as du
import sign_model as sm
from diag_util import HIP_ERROR_INVALID_VALUE, L, P, from_words, s32, words

pytestmark = pytest.mark.gpu

ERR_INVAL = -22     # include/fd_ed25519_hip.h FD_ED25519_HIP_ERR_INVAL


@pytest.fixture(scope="module")
def diag():
    return du.Diag()


@pytest.fixture(scope="module")
def fd():
    from firedancer_amd import ed25519
    return ed25519


@pytest.fixture(scope="module")
def eng(fd):
    e = fd.Engine(0, max_chunk=512, compact=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def btab(eng):
    """the engine's own table: what sign_dev and gen_dev multiply with"""
    t = eng.sign_table()
    assert t.shape == (sm.BTAB_ENTRIES, sm.BTAB_STRIDE) and t.dtype == np.int32
    return t


@pytest.fixture(scope="module")
def q_intervals():
    """the limb intervals of the ge_p2 ge_scalarmult_base returns (bounds_model's chain)"""
    Q, iters, _ = bm.sign_base_loop()
    assert iters < 6
    return Q


@pytest.fixture(scope="module")
def base_cases():
    """(scalars, their affine [s]B): computed once for both orders"""
    xs, _ = sm.base_scalars()
    return xs, sm.base_points(xs)


def test_sign_table(btab):
    model = sm.table()
    tight = du.TIGHT
    for e in range(sm.BTAB_ENTRIES):
        row = [int(v) for v in btab[e]]
        got = tuple(du.fe_val(row[10 * f:10 * f + 10]) for f in range(3))
        assert got == model[e], e
        assert not any(row[30:36]), e
        # ge_madd takes the entry's y+x and y-x as 19-sides and adds its 2dxy product to a doubled
        # tight Z; bounds_model.sign_entry takes all three tight, as gen_btab leaves them
        for f in range(3):
            assert du.within(row[10 * f:10 * f + 10], [-x for x in tight], tight), (e, f)
    assert tuple(du.fe_val([int(v) for v in btab[0][10 * f:10 * f + 10]]) for f in range(3)) == (1, 1, 0)
    b = sm.entry_point(model[1])
    for e in range(sm.BTAB_ENTRIES - 1):      # entry e + 1 = entry e + entry 1, on the device's values
        cur = tuple(du.fe_val([int(v) for v in btab[e][10 * f:10 * f + 10]]) for f in range(2))
        nxt = tuple(du.fe_val([int(v) for v in btab[e + 1][10 * f:10 * f + 10]]) for f in range(2))
        assert du.ed_add(sm.entry_point(cur), b) == sm.entry_point(nxt), e


def check_base(out, xs, pts, q_iv, what):
    def where(i):
        return (f"{what}: s = {hex(xs[i])}, case {i} = lane {i % 256} of block {i // 256}, "
                f"digits {sm.recode256(xs[i] % L)}")

    for i, pt in enumerate(pts):
        o = [int(v) for v in out[i]]
        assert from_words(o[:8]) == sm.encode(pt), where(i)
        X, Y, Z = ([s32(v) for v in o[8 + 10 * c:18 + 10 * c]] for c in range(3))
        z = du.fe_val(Z)
        assert z != 0 and du.fe_val(X) == pt[0] * z % P and du.fe_val(Y) == pt[1] * z % P, where(i)
        for c, limbs in zip("XYZ", (X, Y, Z)):
            assert du.inside(limbs, q_iv[c]), (where(i), c, limbs)


@pytest.mark.parametrize("order", ["listed", "shuffled"])
def test_scalarmult_base(diag, btab, base_cases, q_intervals, order):
    xs, pts = base_cases
    idx = list(range(len(xs)))
    if order == "shuffled":
        random.Random(66).shuffle(idx)
    assert len(idx) % 256 != 0
    out = diag.run_sign("base", [words(xs[i], 8) for i in idx], btab)
    check_base(out, [xs[i] for i in idx], [pts[i] for i in idx], q_intervals, order)
    print(f"ge_scalarmult_base: {len(xs)} cases, {order}")


def test_scalarmult_base_wide(diag, btab, q_intervals):
    xs = sm.base_wide_scalars()
    out = diag.run_sign("base_wide", [words(x, 8) for x in xs], btab)
    check_base(out, xs, sm.base_points(xs), q_intervals, "wide")
    print(f"public-key path: {len(xs)} cases")


def test_muladd(diag):
    ts = sm.muladd_triples()
    out = diag.run_sign("muladd", [words(k, 8) + words(a, 8) + words(r, 8) for k, a, r in ts])
    for (k, a, r), o in zip(ts, out):
        want = k * a + r
        assert from_words(o[:16]) == want, (hex(k), hex(a), hex(r), hex(from_words(o[:16])))
        S = from_words(o[16:24])
        assert S < L and S == want % L, (hex(k), hex(a), hex(r), hex(S))
    print(f"mul256_add: {len(ts)} cases")


def test_encode(diag):
    cases = sm.encode_cases()
    out = diag.run_sign("encode", [list(X) + list(Y) + list(Z) for X, Y, Z, _, _ in cases])
    for (X, Y, Z, pt, note), o in zip(cases, out):
        assert from_words(o[:8]) == sm.encode(pt), (note, X, Y, Z)
        assert not any(o[8:]), note
    print(f"ge_encode: {len(cases)} cases")


def _sign_dev_inputs(eng, privs, msgs):
    n = len(privs)
    buf = b"".join(msgs)
    off = np.arange(n, dtype=np.uint64) * 32
    sz = np.full(n, 32, np.uint32)
    assert all(len(m) == 32 for m in msgs)
    d_m = eng.alloc(len(buf) + 16).upload(np.frombuffer(buf, np.uint8))
    d_off, d_sz = eng.alloc(8 * n).upload(off), eng.alloc(4 * n).upload(sz)
    d_pr = eng.alloc(32 * n).upload(np.frombuffer(b"".join(privs), np.uint8))
    return d_m, d_off, d_sz, d_pr


def test_sign_dev_on_roots(fd, eng, oracle):
    """the whole kernel in the seal's shape: 2048 keys, a 32-byte 4-aligned
    message each, one launch; signature and public key equal the oracle's and
    the Python signer's byte for byte"""
    privs, msgs = sm.root_cases()
    n = len(privs)
    d_m, d_off, d_sz, d_pr = _sign_dev_inputs(eng, privs, msgs)
    assert d_m.ptr % 4 == 0
    d_sig, d_pub = eng.alloc(64 * n), eng.alloc(32 * n)
    eng.sign_dev(n, d_m.ptr, d_off.ptr, d_sz.ptr, d_pr.ptr, d_sig.ptr, d_pub.ptr)
    eng.sync()
    sigs = d_sig.download(np.uint8, 64 * n).reshape(n, 64)
    pubs = d_pub.download(np.uint8, 32 * n).reshape(n, 32)
    model = sm.root_signatures()
    for i in range(n):
        where = f"case {i} = lane {i % 256} of block {i // 256}"
        pub, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
        oracle.oracle_ed25519_public_from_private(pub, privs[i])
        oracle.oracle_ed25519_sign(sig, msgs[i], 32, pub.raw, privs[i])
        assert pub.raw == model[i]["pub"] and sig.raw == model[i]["sig"], where    # the two references agree
        assert pubs[i].tobytes() == pub.raw, where
        assert sigs[i].tobytes() == sig.raw, where

    # argument checks: a pointer off the 16-byte grid is refused before anything is launched
    call = fd.library().fd_ed25519_hip_sign_dev
    fill = np.full(64 * 4 + 16, 0xA5, np.uint8)
    d_s2, d_p2, d_pr2 = eng.alloc(len(fill)).upload(fill), eng.alloc(len(fill)).upload(fill), eng.alloc(32 * 4 + 16)
    d_pr2.upload(np.frombuffer(b"".join(privs[:4]) + bytes(16), np.uint8))
    for dp, ds, dq in ((4, 0, 0), (0, 4, 0), (0, 0, 4), (8, 8, 8), (0, 1, 0)):
        rc = call(eng._h, 4, d_m.ptr, d_off.ptr, d_sz.ptr, d_pr2.ptr + dp, d_s2.ptr + ds, d_p2.ptr + dq, None)
        assert rc == ERR_INVAL, (dp, ds, dq)
    eng.sync()
    assert (d_s2.download(np.uint8, len(fill)) == 0xA5).all() and (d_p2.download(np.uint8, len(fill)) == 0xA5).all()
    assert call(eng._h, 0, d_m.ptr, d_off.ptr, d_sz.ptr, d_pr2.ptr, d_s2.ptr, d_p2.ptr, None) == 0      # n = 0
    assert call(eng._h, 0, None, None, None, None, None, None, None) == 0
    eng.sync()
    assert (d_s2.download(np.uint8, len(fill)) == 0xA5).all() and (d_p2.download(np.uint8, len(fill)) == 0xA5).all()
    print(f"sign_dev: {n} root signatures")


def test_entry_point_rejects_bad_arguments(diag, btab):
    inp, out = np.zeros((4, du.SIGN_IN), np.uint32), np.zeros((4, du.SIGN_OUT), np.uint32)
    tab = np.ascontiguousarray(btab, np.int32)
    for op in (-1, len(du.SIGN_OPS), 99):
        assert diag.raw_sign(op, inp, out, 1, tab) == HIP_ERROR_INVALID_VALUE
    for op in range(len(du.SIGN_OPS)):
        assert diag.raw_sign(op, inp, out, (1 << 20) + 1, tab) == HIP_ERROR_INVALID_VALUE
        assert diag.raw_sign(op, inp, out, 0, tab) == 0                 # nothing to do
    for op in (0, 1):                                                   # the table is required
        assert diag.raw_sign(op, inp, out, 1, None) == HIP_ERROR_INVALID_VALUE
    call = diag.lib.fd_ed25519_diag_sign
    assert call(2, None, out.ctypes.data, 1, None) == HIP_ERROR_INVALID_VALUE
    assert call(2, inp.ctypes.data, None, 1, None) == HIP_ERROR_INVALID_VALUE
    assert not out.any()
    assert diag.raw_sign(2, inp, out, 1, None) == 0 and not out.any()   # 0 * 0 + 0, no table needed
    assert diag.raw_sign(3, inp, out, 4, None) == 0                     # nor for an encoding
