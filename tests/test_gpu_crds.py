"""GPU: the CRDS values of gossip pull responses and push messages
(fd_ed25519_hip_crds_host / _dev, include/fd_ed25519_hip.h Part 2e) against
the test-side model of fd_gossip_recv_crds_value's rules (crds_model.judge: a
bincode walk, the reference's compiled verify, hashlib) and the reference
decoders' verdicts of the fixture.  A small engine: compact tables,
512-signature chunks."""
import hashlib
import struct

import numpy as np
import pytest

import crds_model as model
from crds_util import PULL_RESP, PUSH, Peer, fixture, mutated, packet, rule_cases, u32, valid_packets

pytestmark = pytest.mark.gpu

MAX_CHUNK = 512
PKT_CODES = {model.OK, model.ERR_PARSE, model.UNSUPPORTED}
VAL_CODES = {model.OK, model.UNSUPPORTED, model.ERR_SIGNATURE, model.OWN}


@pytest.fixture(scope="module")
def ed():
    from firedancer_amd import ed25519
    return ed25519


def flavour():
    """the code flavour of crds_model.verifier: the portable backend's where
    the reference is built (its library is the portable build), else the CPU
    oracle's AVX-512 codes; sig_out is compared code for code, so the engine
    is made with the same"""
    from txn_util import ref_lib
    return "portable" if ref_lib() is not None else "avx512"


@pytest.fixture(scope="module")
def eng(ed):
    e = ed.Engine(0, max_chunk=MAX_CHUNK, compact=True, codes=flavour())
    yield e
    e.close()


class Pool:
    """packets under one identity with the model's verdicts -- the packet's
    code and per value the code, verify's own code and the hash --, computed
    once"""

    def __init__(self, oracle):
        verify = model.verifier(oracle)
        self.self_key, fx = fixture()
        self.pkts, self.names = [], []
        for i, f in enumerate(fx):
            self.add(f"fixture:{i}", f["pkt"])
        self.decodes = [f["decodes"] for f in fx]
        for name, p in valid_packets(oracle, 263, None):
            self.add("valid:" + name, bytes(p))
        for name, p, _, _, _ in rule_cases(oracle):   # here under this identity, not the cases' own
            self.add("case:" + name, p)
        self.judged = [model.judge(verify, p, self.self_key) for p in self.pkts]
        self.codes = np.array([c for c, _ in self.judged], np.int8)

    def add(self, name, p):
        self.names.append(name)
        self.pkts.append(p)

    def of(self, kind):
        return [i for i, n in enumerate(self.names) if n.startswith(kind + ":")]

    def want(self, pick, reserve=None):
        """(packet codes, val_first, value codes, verify codes, hashes) of the
        packets pick, reserve[j] slots for the j-th in place of its count"""
        pkt, first, val, sig, hashes = [], [0], [], [], []
        for j, i in enumerate(pick):
            code, vals = self.judged[i]
            r = len(vals) if reserve is None or reserve[j] is None else reserve[j]
            if r != len(vals):
                code = model.BAD_RESERVATION if code == model.OK else code
                vals = [(code, 0, bytes(32))] * r
            pkt.append(code)
            first.append(first[-1] + r)
            val += [v[0] for v in vals]
            sig += [v[1] for v in vals]
            hashes += [v[2] for v in vals]
        return (np.array(pkt, np.int8), np.array(first, np.uint32), np.array(val, np.int8), np.array(sig, np.int8),
                np.frombuffer(b"".join(hashes), np.uint8).reshape(-1, 32))


@pytest.fixture(scope="module")
def pool(oracle):
    return Pool(oracle)


def check_host(eng, pool, pick, hashes=True):
    got = eng.crds_host([pool.pkts[i] for i in pick], pool.self_key, want_hashes=hashes)
    want = pool.want(pick)
    bad = np.nonzero(got[0] != want[0])[0]
    assert len(bad) == 0, [(pool.names[pick[i]], int(got[0][i]), int(want[0][i])) for i in bad[:10]]
    assert (got[1] == want[1]).all() and (got[2] == want[2]).all()
    if hashes:
        assert (got[3] == want[4]).all()


def run_dev(eng, ed, pkts, self_key, first, sig_out=True, hash_out=True, spread=None, pkt_bytes=None):
    """fd_ed25519_hip_crds_dev on device-resident inputs -> (pkt_out, val_out,
    sig_out, hash_out); spread: packet i starts at byte (i + spread) mod 16 of
    a 16-byte line.  Every output and the workspace have a guard behind them."""
    n, n_val, buf, off = len(pkts), int(first[-1]), bytearray(), []
    for i, s in enumerate(pkts):
        if spread is not None:
            buf += b"\xEE" * ((i + spread - len(buf)) % 16)
        off.append(len(buf))
        buf += s
    pkt_bytes = len(buf) if pkt_bytes is None else pkt_bytes
    d_buf = eng.alloc(len(buf) + 16).upload(np.frombuffer(bytes(buf) + bytes(16), np.uint8))   # readable 16 bytes past
    d_off = eng.alloc(8 * n).upload(np.array(off, np.uint64))
    d_sz = eng.alloc(4 * n).upload(np.array([len(s) for s in pkts], np.uint32))
    d_first = eng.alloc(4 * n + 4).upload(np.array(first, np.uint32))
    work = ed.crds_work_bytes(n, n_val)
    d_work = eng.alloc(work + 256).upload(np.full(work + 256, 0x55, np.uint8))
    d_pkt = eng.alloc(n + 8).upload(np.full(n + 8, 0x55, np.int8))
    d_val = eng.alloc(n_val + 8).upload(np.full(n_val + 8, 0x55, np.int8))
    d_sig = eng.alloc(n_val + 8).upload(np.full(n_val + 8, 0x55, np.int8))
    d_hash = eng.alloc(32 * n_val + 32).upload(np.full(32 * n_val + 32, 0x55, np.uint8))
    assert d_work.ptr % 16 == 0 and d_buf.ptr % 4 == 0
    eng.crds_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, pkt_bytes, self_key, d_first.ptr, n_val, d_work.ptr, d_pkt.ptr, d_val.ptr,
                 d_sig.ptr if sig_out else None, d_hash.ptr if hash_out else None)
    eng.sync()
    got = (d_pkt.download(np.int8, n + 8), d_val.download(np.int8, n_val + 8), d_sig.download(np.int8, n_val + 8),
           d_hash.download(np.uint8, 32 * n_val + 32), d_work.download(np.uint8, work + 256))
    for b in (d_buf, d_off, d_sz, d_first, d_work, d_pkt, d_val, d_sig, d_hash):
        b.free()
    # nothing written past the results, into an output that was not given, or past the workspace
    assert (got[0][n:] == 0x55).all() and (got[1][n_val:] == 0x55).all()
    assert (got[2][n_val if sig_out else 0:] == 0x55).all() and (got[3][32 * n_val if hash_out else 0:] == 0x55).all()
    assert (got[4][work:] == 0x55).all()
    return got[0][:n], got[1][:n_val], got[2][:n_val], got[3][:32 * n_val].reshape(-1, 32)


def check_dev(eng, ed, pool, pick, reserve=None, **kw):
    want = pool.want(pick, reserve)
    got = run_dev(eng, ed, [pool.pkts[i] for i in pick], pool.self_key, want[1], **kw)
    bad = np.nonzero(got[0] != want[0])[0]
    assert len(bad) == 0, [(pool.names[pick[i]], int(got[0][i]), int(want[0][i])) for i in bad[:10]]
    assert (got[1] == want[2]).all()
    if kw.get("sig_out", True):
        assert (got[2] == want[3]).all()
    if kw.get("hash_out", True):
        assert (got[3] == want[4]).all()
    return got


def test_fixture_packets(eng, ed, pool):
    """every packet the reference's decoders judged, through crds_host and
    crds_dev: ERR_PARSE exactly where they fail (message discriminants 0, 3,
    4, 5 aside: UNSUPPORTED unread), and the model's codes, code for code"""
    pick = pool.of("fixture")
    want = pool.want(pick)
    assert len(pick) >= 1500 and want[1][-1] > 2 * MAX_CHUNK
    assert set(want[0].tolist()) == PKT_CODES and set(want[2].tolist()) == VAL_CODES
    check_host(eng, pool, pick)
    got = check_dev(eng, ed, pool, pick)
    for i, c in zip(pick, got[0]):
        p = pool.pkts[i]
        if len(p) >= 4 and struct.unpack_from("<I", p)[0] in (0, 3, 4, 5):
            assert c == model.UNSUPPORTED
        else:
            assert (c == model.ERR_PARSE) == (not pool.decodes[i]), pool.names[i]


def test_rule_edges(eng, oracle):
    """every rule edge under its own identity, one call per identity"""
    verify = model.verifier(oracle)
    groups = {}
    for name, p, key, want_pkt, want_vals in rule_cases(oracle):
        groups.setdefault(key, []).append((name, p, want_pkt, want_vals))
    assert len(groups) == 3
    for key, cases in groups.items():
        pkt, first, vals = eng.crds_host([p for _, p, _, _ in cases], key)
        for j, (name, p, want_pkt, want_vals) in enumerate(cases):
            got = (int(pkt[j]), tuple(vals[first[j]:first[j + 1]].tolist()))
            judged = model.judge(verify, p, key)
            assert got == (want_pkt, want_vals) == (judged[0], tuple(v[0] for v in judged[1])), (name, got)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(eng, ed, pool, n):
    """around the stage kernel's 64-lane blocks and the finish kernel's 256"""
    src = pool.of("case") + pool.of("valid") + pool.of("fixture")[:150]
    pick = [src[(7 * i + 3 * n) % len(src)] for i in range(n)]
    check_host(eng, pool, pick)
    check_dev(eng, ed, pool, pick)


def test_a_packets_values_split_across_two_chunks(eng, ed, oracle):
    """52 packets of VAL_MAX values on an engine of 512-signature chunks: the
    values 510..519 of one packet lie on both sides of the chunk boundary;
    every fourth value has a signature of another peer"""
    pr, ot = Peer(oracle, 269), Peer(oracle, 271)
    pkts, want = [], []
    for i in range(52):
        signers = [ot if (10 * i + k) % 4 == 3 else pr for k in range(model.VAL_MAX)]
        pkts.append(bytes(packet(pr, [pr.version(6) for _ in range(model.VAL_MAX)], signers=signers)))
        want += [model.ERR_SIGNATURE if s is ot else 0 for s in signers]
    first = np.arange(53, dtype=np.uint32) * model.VAL_MAX
    assert any(f < MAX_CHUNK < f + model.VAL_MAX for f in first[:-1])
    pkt, val, sig, _ = run_dev(eng, ed, pkts, ot.pub[::-1], first)
    assert not pkt.any() and val.tolist() == want and ((sig != 0) == (val != 0)).all()
    got = eng.crds_host(pkts, ot.pub[::-1])
    assert not got[0].any() and (got[1] == first).all() and got[2].tolist() == want


def test_every_byte_offset(eng, ed, pool):
    """every variant starting at each of the bytes 0..15 of a 16-byte line
    (so at each of 0..3 of a dword), rule edges and fixture packets among them"""
    pick = pool.of("valid") + pool.of("case")[::5] + pool.of("fixture")[:60]
    seen = {d for i in pick for d, *_ in model.signed(pool.pkts[i], pool.self_key)[1]}
    assert seen == set(range(12))
    for spread in range(16):
        check_dev(eng, ed, pool, pick, spread=spread)


def test_val_max_own_rejected_and_unsupported_batches(eng, ed, pool, oracle):
    pr = Peer(oracle, 277)
    full = bytes(packet(pr, [pr.version(6) for _ in range(model.VAL_MAX)]))
    # a packet of VAL_MAX values, alone and under its own identity: only OWN values, nothing to verify
    for key, code in ((bytes(32), model.OK), (pr.pub, model.OWN)):
        pkt, val, sig, hashes = run_dev(eng, ed, [full], key, [0, model.VAL_MAX])
        assert pkt.tolist() == [0] and val.tolist() == [code] * model.VAL_MAX and not sig.any()
        assert [h.tobytes() for h in hashes] == [hashlib.sha256(full[44 + 115 * k:159 + 115 * k]).digest()
                                                 for k in range(model.VAL_MAX)]
        got = eng.crds_host([full] * 3, key, want_hashes=True)
        assert got[1].tolist() == [0, 10, 20, 30] and got[2].tolist() == [code] * 30
    # only rejected packets, only unsupported ones: no value slot at all
    for want in (model.ERR_PARSE, model.UNSUPPORTED):
        pick = [i for i in range(len(pool.codes)) if pool.codes[i] == want][:200]
        assert len(pick) >= 100
        check_host(eng, pool, pick)
        got = check_dev(eng, ed, pool, pick)
        assert len(got[1]) == 0


def test_reservations_one_too_few_and_one_too_many(eng, ed, pool):
    """BAD_RESERVATION for a decoded packet, its own code for one that does not
    decode; the slots of either get that code; every neighbour as before"""
    pick = (pool.of("valid") + pool.of("case"))[:120]
    counts = [len(pool.judged[i][1]) for i in pick]
    for delta in (-1, 1):
        reserve = [max(0, c + delta) if j % 3 == 1 else None for j, c in enumerate(counts)]
        want = pool.want(pick, reserve)
        assert (want[0] == model.BAD_RESERVATION).sum() >= 20 and (want[0] == model.ERR_PARSE).sum() >= 5
        got = check_dev(eng, ed, pool, pick, reserve=reserve)
        assert (got[0] == model.BAD_RESERVATION).sum() == (want[0] == model.BAD_RESERVATION).sum()
    assert any(r is not None and r > model.VAL_MAX for r in reserve)   # more slots than any packet decodes to
    # a val_first that is no prefix sum: a range that leaves n_val and one that runs backwards fill no slot, and the
    # slot nobody fills (out of a workspace of 0x55 bytes) gets BAD_RESERVATION too
    i = pool.names.index("valid:push_3_version_v1")
    pkt, val, sig, hashes = run_dev(eng, ed, [pool.pkts[i]] * 2, pool.self_key, [0, 3, 1])
    assert pkt.tolist() == [model.BAD_RESERVATION] * 2 and val.tolist() == [model.BAD_RESERVATION]
    assert not sig.any() and not hashes.any()


def test_neighbours_of_a_packet_without_verdicts(eng, ed, pool, oracle):
    """a rejected packet, an unsupported one and a bad reservation between
    judged packets change none of their results"""
    a, b = pool.names.index("valid:three_votes"), pool.names.index("valid:two_peers")
    alone = check_dev(eng, ed, pool, [a, b])
    for mid, reserve in ((pool.names.index("case:vote_short"), None), (pool.names.index("case:gossip_disc_4"), None),
                         (pool.names.index("valid:push_2_version_v1"), 3)):
        got = check_dev(eng, ed, pool, [a, mid, b], reserve=[None, reserve, None])
        assert got[0][1] != 0 and (got[0][[0, 2]] == alone[0]).all()
        k = 3 if reserve is None else 3 + reserve
        for x, y in zip(got[1:], alone[1:]):
            assert (x[:3] == y[:3]).all() and (x[k:] == y[3:]).all()


def test_a_packet_that_leaves_the_buffer(eng, ed, oracle):
    """pkt_off + pkt_sz > pkt_bytes: ERR_PARSE, unread; its neighbours judged"""
    pr = Peer(oracle, 281)
    pkts = [bytes(packet(pr, [pr.node_instance()])), bytes(packet(pr, [pr.lowest_slot(1)])), bytes(packet(pr, [pr.version(7)]))]
    total = sum(len(p) for p in pkts)
    pkt, val, _, hashes = run_dev(eng, ed, pkts, bytes(32), [0, 1, 2, 3], pkt_bytes=total - 1)
    assert pkt.tolist() == [0, 0, model.ERR_PARSE] and val.tolist() == [0, 0, model.ERR_PARSE] and not hashes[2].any()
    pkt, val, _, _ = run_dev(eng, ed, pkts, bytes(32), [0, 1, 2, 3], pkt_bytes=len(pkts[0]))
    assert pkt.tolist() == [0, model.ERR_PARSE, model.ERR_PARSE] and val.tolist() == pkt.tolist()
    pkt, val, _, _ = run_dev(eng, ed, pkts, bytes(32), [0, 1, 2, 3], pkt_bytes=total)
    assert not pkt.any() and not val.any()


def test_verify_level_rejects(eng, ed, oracle, adversarial):
    """S >= L, a small-order key, an undecodable R as a value's signature and
    key: ERR_SIGNATURE each, sig_out the reference's own code (none of these
    depends on the message)"""
    d, pr, verify = adversarial, Peer(oracle, 283), model.verifier(oracle)
    vals, want_sig = [], []
    for tag in ("S_plus_L", "A_small_order", "R_undecodable"):
        rows = [i for i in np.nonzero(d["tags"] == tag)[0] if d["codes_avx512"][i] not in (0, -3)][:3]
        assert len(rows) == 3, tag
        for k, i in enumerate(rows):
            sig, pub = d["sigs"][i].tobytes(), d["pubs"][i].tobytes()
            data = (pr.node_instance(key=pub), pr.lowest_slot(2, key=pub), pr.duplicate_shred(9, key=pub))[k]
            ref = verify(bytes(data), sig, pub)
            assert ref == d["codes_" + flavour()][i]
            vals.append(sig + bytes(data))
            want_sig.append(ref)
    good = pr.value(pr.version(6))
    pkts = [u32(PUSH) + pr.pub + struct.pack("<Q", 4) + b"".join(vals[:3] + [good]),
            u32(PULL_RESP) + pr.pub + struct.pack("<Q", 6) + b"".join(vals[3:])]
    assert [model.walk(p)[0] for p in pkts] == [0, 0]
    pkt, val, sig, _ = run_dev(eng, ed, pkts, bytes(32), [0, 4, 10])
    assert not pkt.any() and val.tolist() == [model.ERR_SIGNATURE] * 3 + [0] + [model.ERR_SIGNATURE] * 6
    assert sig.tolist() == want_sig[:3] + [0] + want_sig[3:]


def test_hash_out_alone_and_with_the_other_outputs(eng, ed, pool, oracle):
    """against hashlib.sha256 over signature through end of data, with and
    without sig_out; and values whose hashed bytes end at each edge of the
    padding: 55, 56, 63, 64 and 65 bytes into the last block"""
    pick = pool.of("valid") + pool.of("case")[::3]
    want = pool.want(pick)
    assert any(h.any() for h in want[4]) and any(not h.any() for h in want[4])
    for sig_out in (True, False):
        check_dev(eng, ed, pool, pick, sig_out=sig_out)
    got = check_dev(eng, ed, pool, pick, hash_out=False)
    assert (got[3] == 0x55).all()
    check_host(eng, pool, pick, hashes=False)
    pr = Peer(oracle, 317)
    pkts = [bytes(packet(pr, [pr.duplicate_shred(n), pr.node_instance()])) for n in (50, 51, 58, 59, 60)]
    assert [(len(p) - 44 - 124) % 64 for p in pkts] == [55, 56, 63, 0, 1]
    for spread in (0, 1, 2, 3):
        _, val, _, hashes = run_dev(eng, ed, pkts, bytes(32), [0, 2, 4, 6, 8, 10], sig_out=False, spread=spread)
        assert not val.any()
        assert [h.tobytes() for h in hashes] == [hashlib.sha256(v).digest() for p in pkts for v in (p[44:-124], p[-124:])]


def test_an_empty_batch_and_bad_arguments(eng, ed, pool):
    got = eng.crds_host([], pool.self_key, want_hashes=True)
    assert len(got[0]) == 0 and got[1].tolist() == [0] and len(got[2]) == 0 and len(got[3]) == 0
    eng.crds_dev(0, None, None, None, 0, pool.self_key, None, 0, None, None, None)
    from firedancer_amd.ed25519 import _lib
    out = np.zeros(8, np.int8)
    first = np.zeros(2, np.uint32)
    assert _lib.fd_ed25519_hip_crds_host(eng._h, 1, None, None, None, pool.self_key, first.ctypes.data, out.ctypes.data,
                                         out.ctypes.data, None) == -22
    assert _lib.fd_ed25519_hip_crds_host(eng._h, 0, None, None, None, None, None, None, None, None) == -22
    assert _lib.fd_ed25519_hip_crds_dev(eng._h, 0, None, None, None, 0, None, None, 0, None, None, None, None, None, None) == -22


def test_crds_host_in_two_passes(eng, oracle):
    """more packets than one pass of crds_host stages (16,384): packets with
    values on both sides of the seam among pings of 4 bytes, the value index
    running on across it"""
    pr, ot = Peer(oracle, 293), Peer(oracle, 307)
    ping = u32(4)
    seam = [bytes(packet(pr, [pr.version(6), pr.node_instance()])), bytes(packet(pr, [pr.vote()], signers=[ot])),
            bytes(packet(pr, [pr.lowest_slot(1), pr.version(7), pr.contact_info_v2()])), bytes(packet(pr, [pr.version(6)]))[:-1]]
    pkts = [ping] * 16382 + seam + [ping] * 50 + [bytes(packet(ot, [ot.duplicate_shred(2)]))]
    assert len(pkts) == 16437
    pkt, first, val, hashes = eng.crds_host(pkts, ot.pub, want_hashes=True)
    assert pkt.tolist() == [model.UNSUPPORTED] * 16382 + [0, 0, 0, model.ERR_PARSE] + [model.UNSUPPORTED] * 50 + [0]
    assert first.tolist() == [0] * 16383 + [2, 3] + [6] * 52 + [7]
    assert val.tolist() == [0, 0, model.ERR_SIGNATURE, 0, 0, model.UNSUPPORTED, model.OWN]
    assert hashes[6].tobytes() == hashlib.sha256(pkts[-1][44:]).digest() and not hashes[5].any()
    assert hashes[0].tobytes() == hashlib.sha256(seam[0][44:44 + 115]).digest()


def test_mutations_in_one_batch(eng, oracle):
    """600 seeded mutations under another identity"""
    verify = model.verifier(oracle)
    me = Peer(oracle, 311)
    pkts = [p for _, p in mutated(oracle, 600, 313, me)]
    judged = [model.judge(verify, p, me.pub) for p in pkts]
    pkt, first, val = eng.crds_host(pkts, me.pub)
    assert pkt.tolist() == [c for c, _ in judged]
    assert val.tolist() == [v[0] for _, vals in judged for v in vals]
    assert first.tolist() == np.cumsum([0] + [len(vals) for _, vals in judged]).tolist()
