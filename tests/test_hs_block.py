"""The host-scalar launch's host side (host/fd_ed25519_hip_hs.c): the block
the calling thread fills and dsm16 / dsm16s read in place, and the host's
batch_single_msg combine rule.  CPU only: the fill steps run on a plain
numpy buffer through fd_ed25519_hip_private_hs_init.

The layout, restated from fd_ed25519_hip_internal.h (every array
[row][stride], signature j at column j, each array starting 16-byte
aligned):
    sflag [stride] u8 | hflag [stride] u8 | hs [24][stride] u32 |
    pts [8][40][stride] i32 | pflag [2][stride] u8 | go, 16 bytes
dsm16 reads hs rows 0..18 (the record's words 8..26) and pts rows of 20
limbs (A, R); dsm16s reads 24 rows (hssplit's) and pts rows of 40 limbs (A,
R, A_1, R_1, ..).  pts, pflag and go exist only in a host-decoded block
(stride FD_ED25519_HS_STRIDE = 8)."""
import ctypes

import numpy as np
import pytest

HS_STRIDE = 8
MARK = 0xA5


def a16(x):
    return (x + 15) & ~15


def layout(stride):
    o = {"sflag": 0, "hflag": a16(stride), "hs": 2 * a16(stride)}
    o["pts"] = o["hs"] + 24 * 4 * stride
    o["pflag"] = o["pts"] + 8 * 40 * 4 * stride
    o["go"] = a16(o["pflag"] + 2 * stride)
    return o


@pytest.fixture(scope="module")
def lib():
    from firedancer_amd import ed25519
    L = ed25519.library()
    vp, ul, ci, cp = ctypes.c_void_p, ctypes.c_ulong, ctypes.c_int, ctypes.c_char_p
    L.fd_ed25519_hip_private_hs_bytes.argtypes = [ul, ci]
    L.fd_ed25519_hip_private_hs_bytes.restype = ul
    L.fd_ed25519_hip_private_hs_init.argtypes = [vp, vp, ul, ci, ul, ci, ci]
    L.fd_ed25519_hip_private_hs_init.restype = None
    L.fd_ed25519_hip_private_hs_scalars.argtypes = [vp, ul, cp, cp, cp, ul, ci]
    L.fd_ed25519_hip_private_hs_points.argtypes = [vp, vp]
    L.fd_ed25519_hip_private_hs_points.restype = None
    L.fd_ed25519_hip_private_hs_combine.argtypes = [vp, ul, ul]
    L.fd_ed25519_hip_private_hsrec.argtypes = [cp, cp, cp, ul, ci, vp]
    L.fd_ed25519_hip_private_hssplit.argtypes = [vp, ci, vp, ul, ul]
    L.fd_ed25519_hip_private_hssplit.restype = None
    L.fd_ed25519_hip_private_hsdec3_n.argtypes = [vp, ul, ci, vp, vp, ci, ci, vp]
    L.fd_ed25519_hip_private_hsdec3_n.restype = None
    return L


def test_block_sizes(lib):
    """A host-decoded block ends after its go word; one whose points the
    device decodes after dsm16's 19 rows of hs (no pts at that stride)."""
    for stride in (1, 7, 8, 16, 255, 256, 1 << 16):
        o = layout(stride)
        assert lib.fd_ed25519_hip_private_hs_bytes(stride, 1) == o["go"] + 16
        assert lib.fd_ed25519_hip_private_hs_bytes(stride, 0) == o["hs"] + 19 * 4 * stride
        assert all(v % 16 == 0 for v in o.values())


def _expect(lib, sigs, stride, decode, split, avx):
    """what the block's documented positions hold, from hsrec / hssplit /
    hsdec3_n on their own: {byte offset: (bytes)}"""
    o, want = layout(stride), {}
    hq = np.zeros((24, stride), np.uint32)
    for j, (m, s, p) in enumerate(sigs):
        rec = np.zeros(32, np.uint32)
        assert lib.fd_ed25519_hip_private_hsrec(s, p, m, len(m), 151, rec.ctypes.data) == 1
        if split:
            lib.fd_ed25519_hip_private_hssplit(rec.ctypes.data, split, hq.ctypes.data, stride, j)
        else:
            hq[:19, j] = rec[8:27]
        want[o["sflag"] + j] = bytes([int(rec[27]) & 255])
        want[o["hflag"] + j] = bytes([int(rec[28]) & 255])
    for j in range(len(sigs)):
        for w in range(24 if split else 19):
            want[o["hs"] + 4 * (w * stride + j)] = hq[w, j].tobytes()
    if decode:
        nx, step = (split // 2 - 1, 66 if split == 4 else 33) if split else (0, 33)
        rs = 40 if split else 20
        for j, (_, s, p) in enumerate(sigs):   # this signature's A and R alone
            bufs = [ctypes.create_string_buffer(e, 32) for e in (p, s[:32])]
            arr = (ctypes.c_void_p * 2)(*[ctypes.addressof(b) for b in bufs])
            pt = np.zeros((2, 20), np.int32)
            px = np.zeros((2, max(nx, 1), 40), np.int32)
            fl = np.zeros(2, np.uint8)
            lib.fd_ed25519_hip_private_hsdec3_n(ctypes.addressof(arr), 2, avx, pt.ctypes.data,
                                                px.ctypes.data if split else None, nx, step, fl.ctypes.data)
            for side in range(2):
                for l in range(20):
                    want[o["pts"] + 4 * ((side * rs + l) * stride + j)] = pt[side, l].tobytes()
                for m in range(1, nx + 1):
                    for l in range(40):
                        want[o["pts"] + 4 * (((2 * m + side) * 40 + l) * stride + j)] = px[side, m - 1, l].tobytes()
                want[o["pflag"] + side * stride + j] = bytes([int(fl[side])])
    return want


def _fill(lib, sigs, stride, decode, split, avx, dbits=151):
    size = lib.fd_ed25519_hip_private_hs_bytes(stride, decode)
    raw = np.full(size + 64 + 16, MARK, np.uint8)   # 16-byte aligned block, marker bytes after it too
    base = (-raw.ctypes.data) % 16
    desc = np.zeros(128 // 8, np.uint64)            # FD_ED25519_HS_DESC_MAX bytes
    lib.fd_ed25519_hip_private_hs_init(desc.ctypes.data, raw.ctypes.data + base, stride, decode, len(sigs), split, avx)
    ok = [lib.fd_ed25519_hip_private_hs_scalars(desc.ctypes.data, j, s, p, m, len(m), dbits)
          for j, (m, s, p) in enumerate(sigs)]
    if decode and all(ok):
        bufs = [ctypes.create_string_buffer(e, 32) for _, s, p in sigs for e in (p, s[:32])]
        arr = (ctypes.c_void_p * len(bufs))(*[ctypes.addressof(b) for b in bufs])
        lib.fd_ed25519_hip_private_hs_points(desc.ctypes.data, ctypes.addressof(arr))
    return ok, raw[base:]


@pytest.mark.parametrize("stride,decode,split", [(HS_STRIDE, 1, 0), (HS_STRIDE, 1, 4), (HS_STRIDE, 1, 8), (256, 0, 0)])
@pytest.mark.parametrize("n", [1, 2, 4])
@pytest.mark.parametrize("fixture", ["adversarial", "longd"])
def test_block_fill(lib, request, fixture, n, stride, decode, split):
    """Every element at its documented position equals hsrec's, hssplit's
    and hsdec3_n's own output for that signature; every other byte of the
    block (and after it) is untouched."""
    from conftest import case
    d = request.getfixturevalue(fixture)
    total = len(d["msg_sz"])
    for g in range(0, min(total, 40) - n + 1, n):
        sigs = [case(d, g + i) for i in range(n)]
        for avx in (1, 0):
            ok, blk = _fill(lib, sigs, stride, decode, split, avx)
            assert ok == [1] * n
            want = _expect(lib, sigs, stride, decode, split, avx)
            expect = np.full(len(blk), MARK, np.uint8)
            for off, b in want.items():
                expect[off:off + len(b)] = np.frombuffer(b, np.uint8)
            bad = np.nonzero(blk != expect)[0]
            assert len(bad) == 0, (fixture, g, avx, bad[:8])


def test_no_half_size_pair_returns_zero(lib, halfsize):
    """A k without a pair at 131 bits: the scalars step returns 0 and
    writes nothing (the launch then ends with GO_CANCEL, or without dsm16)."""
    from conftest import case
    seen = 0
    for i in range(len(halfsize["msg_sz"])):
        m, s, p = case(halfsize, i)
        rec = np.zeros(32, np.uint32)
        if lib.fd_ed25519_hip_private_hsrec(s, p, m, len(m), 131, rec.ctypes.data):
            continue
        seen += 1
        for stride, decode, split in ((HS_STRIDE, 1, 4), (256, 0, 0)):
            ok, blk = _fill(lib, [(m, s, p)], stride, decode, split, 1, dbits=131)
            assert ok == [0]
            assert (blk == MARK).all()
    assert seen


def test_combine_matches_batch_single_msg(lib, oracle, batch):
    """Every transaction of batch.npz (0 and 17 signatures included): the
    oracle's per-signature codes through the host combine give the code
    recorded from the reference's fd_ed25519_verify_batch_single_msg."""
    nsig = len(batch["sigs"])
    codes = np.zeros(nsig + 32, np.int8)
    done = np.zeros(nsig + 32, bool)
    tags = set()
    for t in range(len(batch["txn_cnt"])):
        off, sz = int(batch["txn_msg_off"][t]), int(batch["txn_msg_sz"][t])
        f, c = int(batch["txn_first"][t]), int(batch["txn_cnt"][t])
        m = bytes(batch["msgs"][off:off + sz])
        for i in range(f, min(f + c, nsig)):
            if not done[i]:
                codes[i] = oracle.oracle_ed25519_verify(m, len(m), batch["sigs"][i].tobytes(), batch["pubs"][i].tobytes(), 0)
                done[i] = True
        got = lib.fd_ed25519_hip_private_hs_combine(codes.ctypes.data, f, c)
        assert got == int(batch["codes_avx512"][t]), (t, str(batch["tags"][t]), got)
        tags.add(c)
    assert 0 in tags and 17 in tags
