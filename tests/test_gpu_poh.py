"""A block's proof-of-history hash chain on the GPU (include/fd_ed25519_hip.h
Part 2i): the four device hashes on chosen operands, byte shifts and lanes
(libfd_ed25519_diag.so, fd_ed25519_diag_poh_hash), and fd_ed25519_hip_poh_dev,
_host and _blocks_host against the test-side model (poh_model: hashlib) and
the reference's own output (tests/golden/poh.npz, the captured batch).

No test passes a hash_cnt above 4,096: were the bound not held, a run would
merely be longer and a code wrong."""
import ctypes
import random
import struct

import numpy as np
import pytest

import diag_util as du
import poh_model as model
import poh_util as util

pytestmark = pytest.mark.gpu

OPS = ("sha256_leaf65", "sha256_node65", "sha256_chain32", "sha256_mix64")
FILL = 0x55


@pytest.fixture(scope="module")
def ed():
    from firedancer_amd import ed25519
    return ed25519


@pytest.fixture(scope="module")
def eng(ed):
    e = ed.Engine(0, max_chunk=512, compact=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def diag():
    d = du.Diag()
    d.lib.fd_ed25519_diag_poh_hash.argtypes = d.lib.fd_ed25519_diag_hash.argtypes
    d.lib.fd_ed25519_diag_poh_hash.restype = ctypes.c_int
    return d


# ---- the four hashes ---------------------------------------------------------

def run_op(diag, op, buf, rows, extra_rows=64):
    """rows: (off, sz, 16 operand words, the 8 words wanted); one launch,
    every row, every word and every row past n checked"""
    n = len(rows)
    inp = np.zeros((n, du.HASH_IN), np.uint32)
    for i, (off, sz, opnd, _) in enumerate(rows):
        inp[i, 0], inp[i, 1] = off, sz
        inp[i, 4:4 + len(opnd)] = opnd
    out = np.full((n + extra_rows, du.HASH_OUT), du.OUT_FILL, np.uint32)
    rc = diag.lib.fd_ed25519_diag_poh_hash(OPS.index(op), buf.ctypes.data, len(buf), inp.ctypes.data, out.ctypes.data, n)
    assert rc == 0, f"fd_ed25519_diag_poh_hash({op}) returned HIP error {rc}"
    bad = [(i, i % 64, rows[i][0] % 16, rows[i][1]) for i in range(n) if out[i, :8].tolist() != rows[i][3]]
    assert not bad, f"{op}: (case, lane, shift, sz) {bad[:10]} of {n} differ from hashlib"
    assert (out[:n, 8:] == du.OUT_FILL).all() and (out[n:] == du.OUT_FILL).all(), f"{op}: a store outside a case's 8 words"


@pytest.mark.parametrize("filler", [0x00, 0xff])
@pytest.mark.parametrize("n", [1, 32, 64, 101])
def test_leaf65_at_every_byte_shift_and_lane(diag, n, filler):
    """case i sits at byte shift (i + lane group) % 16 of a 16-byte grid:
    lanes 0, 31 and 63 and the partial wave see every shift 0..15 over the
    16 rounds"""
    rng = random.Random(293 + n)
    for rnd in range(16):
        buf, rows = bytearray(), []
        for i in range(n):
            buf += bytes([filler]) * (16 + (i + rnd - len(buf)) % 16)
            sig = bytes(rng.getrandbits(8) for _ in range(64))
            assert len(buf) % 16 == (i + rnd) % 16
            rows.append((len(buf), 64, [], du.be_words(model.sha(b"\x00" + sig))))
            buf += sig
        buf += bytes([filler]) * 16
        run_op(diag, "sha256_leaf65", np.frombuffer(bytes(buf), np.uint8), rows)


def test_leaf65_rejects_a_signature_past_the_buffer(diag):
    buf, inp, out = np.zeros(100, np.uint8), np.zeros((1, du.HASH_IN), np.uint32), np.zeros((1, du.HASH_OUT), np.uint32)
    inp[0, 0] = 37
    assert diag.lib.fd_ed25519_diag_poh_hash(0, buf.ctypes.data, 100, inp.ctypes.data, out.ctypes.data, 1) == 1
    inp[0, 0], inp[0, 1] = 0, 4097
    assert diag.lib.fd_ed25519_diag_poh_hash(2, buf.ctypes.data, 100, inp.ctypes.data, out.ctypes.data, 1) == 1
    assert diag.lib.fd_ed25519_diag_poh_hash(4, buf.ctypes.data, 100, inp.ctypes.data, out.ctypes.data, 1) == 1


def operand(rng, cls):
    return {"zero": [0] * 8, "ones": [0xffffffff] * 8, "top": [0x80000000] * 8, "low": [1] * 8}.get(cls) or \
        [rng.getrandbits(32) for _ in range(8)]


def be_bytes(w):
    return b"".join(struct.pack(">I", x) for x in w)


@pytest.mark.parametrize("op", ["sha256_node65", "sha256_mix64"])
@pytest.mark.parametrize("n", [1, 64, 101])
def test_node65_and_mix64(diag, op, n):
    rng = random.Random(307 + n)
    classes = ("random", "zero", "ones", "top", "low")
    rows = []
    for i in range(n):
        a, b = operand(rng, classes[i % 5]), operand(rng, classes[(i // 5) % 5])
        msg = (b"\x01" if op == "sha256_node65" else b"") + be_bytes(a) + be_bytes(b)
        rows.append((0, 0, a + b, du.be_words(model.sha(msg))))
    run_op(diag, op, np.zeros(16, np.uint8), rows)


@pytest.mark.parametrize("n", [1, 64, 70])
def test_chain32_every_fixture_k_mixed_in_a_wave(diag, n):
    """lane i runs KS[i % 9] compressions: lanes 0, 31 and 63 and the partial
    wave, and every wave holds every k"""
    g = util.golden()
    rng = random.Random(311)
    rows = [(0, int(k), du.be_words(g["append_in"].tobytes()), du.be_words(out.tobytes()))
            for k, out in zip(g["append_k"], g["append_out"])]
    while len(rows) < n:
        state, k = operand(rng, ("random", "zero", "ones")[len(rows) % 3]), util.KS[(len(rows) * 7) % 9]
        rows.append((0, k, state, du.be_words(model.append(be_bytes(state), k))))
    rows = rows[-n:] if n < 9 else rows
    run_op(diag, "sha256_chain32", np.zeros(16, np.uint8), rows)


# ---- poh_dev -------------------------------------------------------------------

def run_dev(eng, ed, d, bound=model.CEIL, shift=0, with_hash=True):
    """fd_ed25519_hip_poh_dev with buf at byte `shift` of its allocation ->
    (codes, states or None, the workspace after the call).  The outputs carry
    8 slots more and the workspace 64 bytes more than the call is told of:
    they must come back as they went in."""
    n, n_sig = d.n, len(d.sig_off)
    size = len(d.buf)
    host = np.full(shift + size + 16, FILL, np.uint8)
    host[shift:shift + size] = np.frombuffer(d.buf, np.uint8)
    d_buf = eng.alloc(len(host)).upload(host)
    d_hdr = eng.alloc(8 * n + 8).upload(np.append(d.hdr_off, np.uint64(0)))
    d_in = eng.alloc(8 * n + 8).upload(np.append(d.in_off, np.uint64(0)))
    d_first = eng.alloc(4 * n + 4).upload(d.sig_first)
    d_sig = eng.alloc(8 * n_sig + 8).upload(np.append(d.sig_off, np.uint64(0)))
    d_out = eng.alloc(n + 8).upload(np.full(n + 8, FILL, np.int8))
    d_hash = eng.alloc(32 * n + 256).upload(np.full(32 * n + 256, FILL, np.uint8))
    work_bytes = ed.poh_work_bytes(n, n_sig)
    d_work = eng.alloc(work_bytes + 64).upload(np.full(work_bytes + 64, FILL, np.uint8))
    eng.poh_dev(n, d_buf.ptr + shift, size, d_hdr.ptr, d_in.ptr, d_first.ptr, n_sig, d_sig.ptr, bound, d_out.ptr,
                d_hash.ptr if with_hash else None, d_work.ptr)
    eng.sync()
    out = d_out.download(np.int8, n + 8)
    states = d_hash.download(np.uint8, 32 * n + 256)
    work = d_work.download(np.uint8, work_bytes + 64)
    assert (out[n:] == FILL).all() and (states[32 * n:] == FILL).all() and (work[33 * n + 32 * n_sig:] == FILL).all()
    assert (d_buf.download(np.uint8, len(host)) == host).all()
    if not with_hash:
        assert (states == FILL).all()
    for b in (d_buf, d_hdr, d_in, d_first, d_sig, d_out, d_hash, d_work):
        b.free()
    return out[:n], (states[:32 * n].reshape(-1, 32) if with_hash else None), work


def check_dev(eng, ed, d, bound=model.CEIL, shift=0, want=None):
    want = d.want(bound) if want is None else want
    codes, states, work = run_dev(eng, ed, d, bound, shift)
    bad = np.nonzero(codes != want[0])[0]
    assert not len(bad), (bad[:8].tolist(), codes[bad[:8]].tolist(), want[0][bad[:8]].tolist())
    assert np.array_equal(states, want[1])
    return codes, states, work


@pytest.mark.parametrize("shift", range(16))
def test_dev_with_buf_at_every_byte_of_16(eng, ed, shift):
    d, verdicts, states, _ = util.fixture_microblocks()
    check_dev(eng, ed, d, shift=shift, want=(verdicts, states))


def test_dev_on_the_captured_batch(eng, ed):
    g = util.golden()
    codes, states, _ = check_dev(eng, ed, util.captured(), want=(g["cap_verdict"], g["cap_state"]))
    assert not codes.any()
    codes, states, _ = run_dev(eng, ed, util.captured(), with_hash=False)
    assert not codes.any()


def test_dev_on_every_signature_count_and_k(eng, ed):
    """1 .. 300 signatures (the LDS tree, the in-place layers above 128, the
    odd layers) and one wave holding k = 0, 1, 2, 3, 63, 64, 65, 1000 and 4096
    together"""
    d = util.shapes()
    assert d.n <= 64 and {1, 128, 129, 300} <= set(np.diff(d.sig_first).tolist())
    codes, _, _ = check_dev(eng, ed, d, shift=5)
    assert not codes.any()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_dev_on_n_microblocks(eng, ed, n):
    base = util.captured()
    want = base.want()
    pick = [i % 64 for i in range(n)]
    codes, _, _ = check_dev(eng, ed, util.cycle(base, n), want=(want[0][pick], want[1][pick]))
    assert not codes.any()


def test_divergent_wave(eng, ed):
    """ticks of k = 0, 1, 64 and 1000 interleaved in one wave, chained"""
    rng = random.Random(313)
    in_state = bytes(rng.getrandbits(8) for _ in range(32))
    blk = util.make_block(rng, in_state, [[((0, 1, 64, 1000)[i % 4], 0) for i in range(64)]])
    codes, _, _ = check_dev(eng, ed, util.describe(blk, in_state))
    assert not codes.any()


def test_rejected_unsupported_and_mismatching_among_good_ones(eng, ed):
    base = util.shapes(kmax=1000)
    d, touched = util.broken(base, over=1500)
    want = d.want(1200)
    codes, states, work = check_dev(eng, ed, d, bound=1200, want=want)
    assert {model.ERR_PARSE, model.UNSUPPORTED, model.ERR_HASH} == set(codes[touched].tolist())
    rest = [i for i in range(d.n) if i not in touched]
    assert not codes[rest].any()
    good = base.want()
    assert np.array_equal(states[rest], good[1][rest])
    # the workspace: roots behind the leaves, then the flags.  A microblock without signatures, and one whose
    # signature leaves the buffer, has no root written
    n_sig = len(d.sig_off)
    roots = work[32 * n_sig:32 * n_sig + 32 * d.n].reshape(-1, 32)
    for i in range(d.n):
        cnt = int(d.sig_first[i + 1]) - int(d.sig_first[i])
        sig_outside = any(int(o) + 64 > len(d.buf) for o in d.sig_off[d.sig_first[i]:d.sig_first[i + 1]])
        assert (roots[i] == FILL).all() == (cnt == 0 or sig_outside), i
    # the bound at k - 1, k and k + 1
    for bound, code in ((999, model.UNSUPPORTED), (1000, 0), (1001, 0)):
        codes, _, _ = run_dev(eng, ed, base, bound)
        ks = [model.steps(*struct.unpack_from("<Q32xQ", base.buf, int(h)))[0] for h in base.hdr_off]
        assert codes.tolist() == [code if k == 1000 else 0 for k in ks] and 1000 in ks


def test_dev_argument_checks(eng, ed):
    d = util.captured()
    with pytest.raises(ed.HipError):
        run_dev(eng, ed, d, bound=(1 << 17) + 1)
    eng.poh_dev(0, None, 0, None, None, None, 0, None, 16, None, None, None)     # n == 0: a no-op


# ---- poh_host and poh_blocks_host ----------------------------------------------

def test_host_on_fixture_shapes_and_broken(eng):
    d, verdicts, states, _ = util.fixture_microblocks()
    codes, got = eng.poh_host(*d.args())
    assert np.array_equal(codes, verdicts) and np.array_equal(got, states)
    base = util.shapes(kmax=1000)
    b, _ = util.broken(base, over=1500)
    want = b.want(1200)
    codes, got = eng.poh_host(*b.args(), hash_cnt_max=1200)
    assert np.array_equal(codes, want[0]) and np.array_equal(got, want[1])
    assert {0, model.ERR_PARSE, model.UNSUPPORTED, model.ERR_HASH} == set(codes.tolist())


def test_host_in_several_passes(eng):
    """more microblocks than a pass takes, and more signatures: the captured
    batch over and over, in the caller's order after the ordering by k"""
    base = util.captured()
    want = base.want()
    n = 16384 + 70
    d = util.cycle(base, n)
    pick = [i % 64 for i in range(n)]
    codes, states = eng.poh_host(*d.args())
    assert np.array_equal(codes, want[0][pick]) and np.array_equal(states, want[1][pick])


def test_blocks_host(eng, ed):
    rng = random.Random(317)
    cap = util.captured_block()
    in_state = bytes(rng.getrandbits(8) for _ in range(32))
    two = util.make_block(rng, in_state, [[(3, 2), (0, 0), (5, 0)], [(1, 1), (7, 130)]])
    slow = util.make_block(rng, in_state, [[(2, 1), (3000, 0), (4, 2)]])
    hdr = model.walk(two)[1]
    flipped = bytearray(two)
    flipped[hdr[3] + 8] ^= 1                       # the fourth microblock's hash: it and its successor mismatch
    blocks = [cap, cap, two, bytes(flipped), two[:-1], b"", slow, struct.pack("<Q", 0), cap[:model.walk(cap)[1][1]]]
    ins = [bytes(32), b"\x01" + bytes(31), in_state, in_state, in_state, in_state, in_state, in_state, bytes(32)]
    codes, first_bad, last = eng.poh_blocks_host(blocks, ins, hash_cnt_max=2000)
    want_codes, want_bad, want_last = [], [], []
    for blk, st in zip(blocks, ins):
        if model.walk(blk)[0] or not model.walk(blk)[1]:
            want_codes.append(model.ERR_PARSE); want_bad.append(0xFFFFFFFF); want_last.append(bytes(32))
            continue
        d = util.describe(blk, st)
        code, bad = model.reduce_block(d.want(2000)[0].tolist())
        want_codes.append(code); want_bad.append(bad)
        want_last.append(d.buf[int(d.hdr_off[-1]) + 8:int(d.hdr_off[-1]) + 40])
    assert codes.tolist() == want_codes == [0, -25, 0, -25, -16, -16, -18, -16, -16]
    assert first_bad.tolist() == want_bad and want_bad[1] == 0 and want_bad[3] == 3 and want_bad[6] == 1
    assert [x.tobytes() for x in last] == want_last
    with pytest.raises(ed.HipError):
        eng.poh_blocks_host([cap], [bytes(32)], hash_cnt_max=(1 << 17) + 1)


def test_blocks_host_in_several_passes(eng):
    """poh_blocks_host over more microblocks than a pass takes: 257 copies of
    the captured block (64 microblocks and 1,280 signatures each), every third
    one from another in state -- each block's first microblock reads its
    state from in_hash, in either pass, after the ordering by k.  Every block
    comes back as the same block and state submitted alone"""
    cap = util.captured_block()
    states = [bytes(32), b"\x01" + bytes(31)]
    alone = [eng.poh_blocks_host([cap], [st]) for st in states]
    assert [int(a[0][0]) for a in alone] == [0, model.ERR_HASH] and [int(a[1][0]) for a in alone] == [0xFFFFFFFF, 0]
    pick = [int(b % 3 == 1) for b in range(257)]
    assert 257 * 64 > 16384 and 257 * 1280 > 1 << 18 and len(set(pick[200:210])) == 2
    codes, first_bad, last = eng.poh_blocks_host([cap] * 257, [states[p] for p in pick])
    assert codes.tolist() == [int(alone[p][0][0]) for p in pick]
    assert first_bad.tolist() == [int(alone[p][1][0]) for p in pick]
    assert [x.tobytes() for x in last] == [alone[p][2][0].tobytes() for p in pick]
