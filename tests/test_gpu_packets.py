"""GPU: signed gossip and repair control packets (fd_ed25519_hip_packets_host /
_dev, include/fd_ed25519_hip.h Part 2d) against the test-side model of the
handlers' rules (packet_model.judge: a bincode walk and the reference's
compiled verify) and the reference decoders' verdicts of the fixture.  A
small engine: compact tables, 512-signature chunks."""
import struct

import numpy as np
import pytest

import packet_model as model
from packet_util import GOSSIP, REPAIR, Node, fixture, mutated, rule_cases, valid_packets

pytestmark = pytest.mark.gpu

MAX_CHUNK = 512
CODES = {model.OK, model.ERR_PARSE, model.UNSUPPORTED, model.ERR_SIGNATURE, model.NOT_FOR_SELF}


@pytest.fixture(scope="module")
def ed():
    from firedancer_amd import ed25519
    return ed25519


@pytest.fixture(scope="module")
def eng(ed):
    e = ed.Engine(0, max_chunk=MAX_CHUNK, compact=True)
    yield e
    e.close()


class Pool:
    """packets of both protocols under one identity with the model's verdicts
    (the code, and verify's own code), computed once"""

    def __init__(self, oracle):
        verify = model.verifier(oracle)
        self.self_key, fx = fixture()
        self.pkts, self.proto, self.names = [], [], []
        for i, f in enumerate(fx):
            self.add(f"fixture:{i}", f["proto"], f["pkt"])
        self.decodes = [f["decodes"] for f in fx]
        for name, proto, p in valid_packets(oracle, 103, self.self_key):
            self.add("valid:" + name, proto, p)
        for name, proto, p, _, _ in rule_cases(oracle):   # here under this identity, not the cases' own
            self.add("case:" + name, proto, p)
        for name, proto, p in mutated(oracle, 300, 157, self.self_key):
            self.add("mutation:" + name, proto, p)
        judged = [model.judge(verify, pr, p, self.self_key) for pr, p in zip(self.proto, self.pkts)]
        self.codes = np.array([c for c, _ in judged], np.int8)
        self.sig = np.array([v for _, v in judged], np.int8)
        self.proto = np.array(self.proto)

    def add(self, name, proto, p):
        self.names.append(name)
        self.proto.append(proto)
        self.pkts.append(p)

    def of(self, kind, proto=None):
        return [i for i, n in enumerate(self.names) if n.startswith(kind + ":") and proto in (None, self.proto[i])]


@pytest.fixture(scope="module")
def pool(oracle):
    return Pool(oracle)


def check_host(eng, pool, proto, pick):
    assert all(pool.proto[i] == proto for i in pick)
    codes = eng.packets_host(proto, [pool.pkts[i] for i in pick], pool.self_key)
    bad = np.nonzero(codes != pool.codes[pick])[0]
    assert len(bad) == 0, [(pool.names[pick[i]], int(codes[i]), int(pool.codes[pick[i]])) for i in bad[:10]]


@pytest.mark.parametrize("proto", [GOSSIP, REPAIR])
def test_fixture_packets(eng, pool, proto):
    """every packet the reference's decoders judged: ERR_PARSE exactly where
    they fail (gossip discriminants 0..2 aside: UNSUPPORTED unread), and the
    model's code"""
    pick = pool.of("fixture", proto)
    assert len(pick) >= 800 and set(pool.codes[pick].tolist()) == CODES
    codes = eng.packets_host(proto, [pool.pkts[i] for i in pick], pool.self_key)
    assert (codes == pool.codes[pick]).all()
    for i, c in zip(pick, codes):
        p = pool.pkts[i]
        if proto == GOSSIP and len(p) >= 4 and struct.unpack_from("<I", p)[0] <= 2:
            assert c == model.UNSUPPORTED
        else:
            assert (c == model.ERR_PARSE) == (not pool.decodes[i]), pool.names[i]


def test_rule_edges(eng, oracle):
    """every rule edge under its own identity, one call per protocol and identity"""
    verify = model.verifier(oracle)
    groups = {}
    for name, proto, p, key, want in rule_cases(oracle):
        groups.setdefault((proto, key), []).append((name, p, want))
    assert len(groups) == 6
    for (proto, key), cases in groups.items():
        codes = eng.packets_host(proto, [p for _, p, _ in cases], key)
        for (name, p, want), c in zip(cases, codes):
            assert c == want == model.judge(verify, proto, p, key)[0], (name, int(c), want)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_batch_sizes(eng, pool, n):
    """around the stage kernel's 64-lane blocks and the finish kernel's 256"""
    for proto in (GOSSIP, REPAIR):
        src = pool.of("case", proto) + pool.of("valid", proto) + pool.of("fixture", proto)[:150]
        check_host(eng, pool, proto, [src[(7 * i + 3 * n) % len(src)] for i in range(n)])


@pytest.mark.parametrize("proto", [GOSSIP, REPAIR])
def test_mixed_batch_spans_three_chunks(eng, pool, proto):
    pick = (pool.of("valid", proto) + pool.of("case", proto) + pool.of("mutation", proto) + pool.of("fixture", proto))[:1100]
    rng = np.random.default_rng(107)
    pick = [pick[i] for i in rng.permutation(len(pick))]
    assert len(pick) == 1100 > 2 * MAX_CHUNK and set(pool.codes[pick].tolist()) == CODES
    check_host(eng, pool, proto, pick)


@pytest.mark.parametrize("proto", [GOSSIP, REPAIR])
def test_only_rejected_and_only_unsupported_packets(eng, pool, proto):
    for want in ((model.ERR_PARSE, model.NOT_FOR_SELF), (model.UNSUPPORTED,)):
        pick = [i for i in range(len(pool.codes)) if pool.codes[i] in want and pool.proto[i] == proto][:200]
        assert len(pick) >= 20
        check_host(eng, pool, proto, pick)


def test_every_prune_size(eng, pool):
    pick = [i for i in pool.of("valid", GOSSIP) if "prune" in pool.names[i]]
    assert sorted((len(pool.pkts[i]) - 180) // 32 for i in pick) == list(range(33)) and not pool.codes[pick].any()
    check_host(eng, pool, GOSSIP, pick)


def run_dev(eng, ed, proto, pkts, self_key, sig_out=True, spread=None, pkt_bytes=None):
    """fd_ed25519_hip_packets_dev on device-resident inputs -> (out, sig_out);
    spread: packet i starts at byte (i + spread) mod 16 of a 16-byte line.
    The workspace has a guard behind the size the macro gives."""
    n, buf, off = len(pkts), bytearray(), []
    for i, s in enumerate(pkts):
        if spread is not None:
            buf += b"\xEE" * ((i + spread - len(buf)) % 16)
        off.append(len(buf))
        buf += s
    pkt_bytes = len(buf) if pkt_bytes is None else pkt_bytes
    d_buf = eng.alloc(len(buf) + 16).upload(np.frombuffer(bytes(buf) + bytes(16), np.uint8))   # readable 16 bytes past
    d_off = eng.alloc(8 * n).upload(np.array(off, np.uint64))
    d_sz = eng.alloc(4 * n).upload(np.array([len(s) for s in pkts], np.uint32))
    work = ed.packet_work_bytes(n, pkt_bytes)
    d_work = eng.alloc(work + 256).upload(np.full(work + 256, 0x55, np.uint8))
    d_out = eng.alloc(n + 8).upload(np.full(n + 8, 0x55, np.int8))
    d_sig = eng.alloc(n + 8).upload(np.full(n + 8, 0x55, np.int8))
    assert d_work.ptr % 16 == 0 and d_buf.ptr % 16 == 0
    eng.packets_dev(proto, n, d_buf.ptr, d_off.ptr, d_sz.ptr, pkt_bytes, self_key, d_work.ptr, d_out.ptr,
                    d_sig.ptr if sig_out else None)
    eng.sync()
    got = d_out.download(np.int8, n + 8), d_sig.download(np.int8, n + 8), d_work.download(np.uint8, work + 256)
    for b in (d_buf, d_off, d_sz, d_work, d_out, d_sig):
        b.free()
    # nothing written past the n results, into an output that was not given, or past the workspace
    assert (got[0][n:] == 0x55).all() and (got[1][n if sig_out else 0:] == 0x55).all()
    assert (got[2][work:] == 0x55).all()
    return got[0][:n], got[1][:n]


@pytest.mark.parametrize("proto", [GOSSIP, REPAIR])
def test_every_byte_offset(eng, ed, pool, proto):
    """every kind and every prune size starting at each of the bytes 0..15 of
    a 16-byte line, rule edges and fixture packets among them"""
    pick = pool.of("valid", proto) + pool.of("case", proto) + pool.of("fixture", proto)[:60]
    for spread in range(16):
        out, sig = run_dev(eng, ed, proto, [pool.pkts[i] for i in pick], pool.self_key, spread=spread)
        assert (out == pool.codes[pick]).all() and (sig == pool.sig[pick]).all(), spread


@pytest.mark.parametrize("proto", [GOSSIP, REPAIR])
def test_packets_dev_without_sig_out(eng, ed, pool, proto):
    pick = pool.of("valid", proto) + pool.of("case", proto)
    pkts = [pool.pkts[i] for i in pick]
    out, _ = run_dev(eng, ed, proto, pkts, pool.self_key, sig_out=False)
    assert (out == pool.codes[pick]).all()
    out, sig = run_dev(eng, ed, proto, pkts, pool.self_key)
    assert (out == pool.codes[pick]).all() and (sig == pool.sig[pick]).all()
    assert (sig[pool.codes[pick] != model.ERR_SIGNATURE] == 0).all()


def test_verify_level_rejects(eng, ed, oracle, adversarial):
    """S >= L, a small-order key, an undecodable R as a packet's signature and
    key: ERR_SIGNATURE each, sig_out the reference's own code (none of these
    depends on the message)"""
    d, me, nd = adversarial, Node(oracle, 109), Node(oracle, 113)
    for proto in (GOSSIP, REPAIR):
        pkts, want_sig = [], []
        for tag in ("S_plus_L", "A_small_order", "R_undecodable"):
            rows = [i for i in np.nonzero(d["tags"] == tag)[0] if d["codes_avx512"][i] not in (0, -3)][:3]
            assert len(rows) == 3, tag
            for k, i in enumerate(rows):
                sig, pub = d["sigs"][i].tobytes(), d["pubs"][i].tobytes()
                if proto == REPAIR:
                    p = bytearray(nd.request(8 + k, me.pub))
                    p[4:68], p[68:100] = sig, pub
                elif k == 2:
                    p = bytearray(nd.ping(4))
                    p[68:132], p[4:36] = sig, pub
                else:
                    p = bytearray(nd.prune(k + 1, me.pub))
                    p[-104:-40], p[36:68] = sig, pub
                code, s = model.signed(proto, bytes(p), me.pub)
                assert code == 0 and s[0] == pub and s[1] == sig
                ref = oracle.oracle_ed25519_verify(s[2], len(s[2]), sig, pub, 0)
                assert ref == d["codes_avx512"][i]
                pkts.append(bytes(p))
                want_sig.append(ref)
        pkts.append(nd.ping(5) if proto == GOSSIP else nd.request(10, me.pub))
        want_sig.append(0)
        out, sig = run_dev(eng, ed, proto, pkts, me.pub)
        assert out.tolist() == [model.ERR_SIGNATURE] * 9 + [0] and sig.tolist() == want_sig


def test_wrong_self_key_and_wrong_signer(eng, oracle):
    me, nd, ot = Node(oracle, 127), Node(oracle, 131), Node(oracle, 137)
    gossip = [nd.prune(3, me.pub), nd.prune(3, ot.pub), nd.prune(3, me.pub, outer=ot.pub),
              nd.prune(3, me.pub, outer=ot.pub, signer=ot), nd.ping(4)]
    assert eng.packets_host(GOSSIP, gossip, me.pub).tolist() == [0, model.NOT_FOR_SELF, 0, model.ERR_SIGNATURE, 0]
    assert eng.packets_host(GOSSIP, gossip, ot.pub).tolist() == [model.NOT_FOR_SELF, 0, model.NOT_FOR_SELF,
                                                                 model.NOT_FOR_SELF, 0]
    repair = [nd.request(8, me.pub), nd.request(9, ot.pub), nd.request(10, me.pub, signer=me), nd.request(9, me.pub)]
    assert eng.packets_host(REPAIR, repair, me.pub).tolist() == [0, model.NOT_FOR_SELF, model.ERR_SIGNATURE, 0]
    assert eng.packets_host(REPAIR, repair, ot.pub).tolist() == [model.NOT_FOR_SELF, 0, model.NOT_FOR_SELF,
                                                                 model.NOT_FOR_SELF]


def test_a_packet_that_leaves_the_buffer(eng, ed, oracle):
    """pkt_off + pkt_sz > pkt_bytes: ERR_PARSE, unread; its neighbours judged"""
    me, nd = Node(oracle, 139), Node(oracle, 149)
    pkts = [nd.request(8, me.pub), nd.request(9, me.pub), nd.request(10, me.pub)]
    total = sum(len(p) for p in pkts)
    out, _ = run_dev(eng, ed, REPAIR, pkts, me.pub, pkt_bytes=total - 1)
    assert out.tolist() == [0, 0, model.ERR_PARSE]
    out, _ = run_dev(eng, ed, REPAIR, pkts, me.pub, pkt_bytes=len(pkts[0]))
    assert out.tolist() == [0, model.ERR_PARSE, model.ERR_PARSE]
    pkts = [nd.ping(4), nd.prune(32, me.pub)]
    out, _ = run_dev(eng, ed, GOSSIP, pkts, me.pub, pkt_bytes=132 + 1203)
    assert out.tolist() == [0, model.ERR_PARSE]
    out, _ = run_dev(eng, ed, GOSSIP, pkts, me.pub, pkt_bytes=132 + 1204)
    assert out.tolist() == [0, 0]


def test_an_empty_batch_and_bad_arguments(eng, ed, pool):
    assert len(eng.packets_host(GOSSIP, [], pool.self_key)) == 0
    eng.packets_dev(REPAIR, 0, None, None, None, 0, pool.self_key, None, None)
    with pytest.raises(ed.HipError):
        eng.packets_host(2, [pool.pkts[0]], pool.self_key)
    with pytest.raises(ed.HipError):
        eng.packets_dev(7, 0, None, None, None, 0, pool.self_key, None, None)
    from firedancer_amd.ed25519 import _lib
    out = np.zeros(1, np.int8)
    assert _lib.fd_ed25519_hip_packets_host(eng._h, GOSSIP, 1, None, None, None, None, out.ctypes.data) == -22
    assert _lib.fd_ed25519_hip_packets_dev(eng._h, GOSSIP, 0, None, None, None, 0, None, None, None, None, None) == -22


def test_packets_host_in_two_passes(eng, oracle):
    """more packets than one pass of packets_host stages (16,384): judged
    packets on both sides of the seam among legacy requests of 4 bytes"""
    me, nd, ot = Node(oracle, 163), Node(oracle, 167), Node(oracle, 173)
    legacy = struct.pack("<I", 2)
    pkts = [legacy] * 16382 + [nd.request(8, me.pub), nd.request(10, ot.pub), nd.request(9, me.pub), nd.request(10, me.pub)[:-1]] + \
        [legacy] * 50 + [nd.request(10, me.pub, signer=ot)]
    want = [model.UNSUPPORTED] * 16382 + [0, model.NOT_FOR_SELF, 0, model.ERR_PARSE] + [model.UNSUPPORTED] * 50 + \
        [model.ERR_SIGNATURE]
    assert len(pkts) == 16437
    assert eng.packets_host(REPAIR, pkts, me.pub).tolist() == want


def test_mutations_in_one_batch_each(eng, oracle):
    """600 seeded mutations under another identity"""
    verify = model.verifier(oracle)
    me = Node(oracle, 89).pub
    muts = mutated(oracle, 600, 151, me)
    for proto in (GOSSIP, REPAIR):
        pkts = [p for _, pr, p in muts if pr == proto]
        want = [model.judge(verify, proto, p, me)[0] for p in pkts]
        assert eng.packets_host(proto, pkts, me).tolist() == want
