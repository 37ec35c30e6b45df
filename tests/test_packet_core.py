"""CPU: fd_ed25519_hip_packet_plan (fd_packet_core.h through the library, no
GPU) against the test-side model of the gossip and repair handlers' rules
(tests/packet_model.py) and against the reference decoders' own verdicts
(tests/golden/packets.npz): the fixture, one case per rule edge, and seeded
mutations."""
import collections
import ctypes

import pytest

import packet_model as model
from packet_util import GOSSIP, REPAIR, Node, fixture, mutated, rule_cases


def ed():
    from firedancer_amd import ed25519
    return ed25519


def planned(proto, p, self_key):
    """the library's (code, (key, signature, message) or None) in the model's terms"""
    code, pl = ed().packet_plan(proto, p, self_key)
    if code != model.OK:
        assert not any(int(pl[f]) for f in ("key_off", "sig_off", "msg0_off", "msg0_sz", "msg1_off", "msg1_sz"))
        return code, None
    k, s, a, an, b, bn = (int(pl[f]) for f in ("key_off", "sig_off", "msg0_off", "msg0_sz", "msg1_off", "msg1_sz"))
    assert max(k + 32, s + 64, a + an, b + bn) <= len(p)
    return code, (p[k:k + 32], p[s:s + 64], p[a:a + an] + p[b:b + bn])


def test_constants_match_the_header():
    e = ed()
    assert (e.PACKET_OK, e.PACKET_ERR_PARSE, e.PACKET_UNSUPPORTED, e.PACKET_ERR_SIGNATURE, e.PACKET_NOT_FOR_SELF) == \
        (model.OK, model.ERR_PARSE, model.UNSUPPORTED, model.ERR_SIGNATURE, model.NOT_FOR_SELF)
    assert (e.PROTO_GOSSIP, e.PROTO_REPAIR_SERV, e.PACKET_MAX) == (GOSSIP, REPAIR, model.MAX)
    assert e.packet_work_bytes(3, 1000) == 110 * 3 + 1024 and e.packet_work_bytes(0, 0) == 16
    assert e.packet_work_bytes(1, 1008) == 110 + 1024 and e.packet_work_bytes(1, 1009) == 110 + 1040
    assert e.PACKET_PLAN_DTYPE.itemsize == 16


def test_fixture_agrees_with_the_reference_decoders(oracle):
    """every packet the reference judged: ERR_PARSE exactly when its decode
    fails or leaves bytes over -- but for gossip discriminants 0..2, which get
    UNSUPPORTED with no look at their CRDS values, whatever the decoder
    makes of them --, its discriminant, and for prunes its encoder's sign
    data as the planned message"""
    verify = model.verifier(oracle)
    self_key, packets = fixture()
    assert 2000 <= len(packets) <= 5000
    seen, ms = collections.Counter(), set()
    for f in packets:
        proto, p = f["proto"], f["pkt"]
        assert len(p) <= model.MAX
        got = planned(proto, p, self_key)
        assert got == model.signed(proto, p, self_key), p.hex()
        disc = int(ed().packet_plan(proto, p, self_key)[1]["disc"])
        if proto == GOSSIP and len(p) >= 4 and disc <= 2:
            assert got[0] == model.UNSUPPORTED
        else:
            assert (got[0] == model.ERR_PARSE) == (not f["decodes"]), (proto, p.hex())
        if f["decodes"]:
            assert disc == f["disc"]
        if f["sign_data"] is not None and got[0] == model.OK:
            assert got[1][2] == f["sign_data"] and disc == 3
            ms.add((len(p) - 180) // 32)
        assert (f["sign_data"] is not None) == (proto == GOSSIP and f["decodes"] and f["disc"] == 3)
        code = model.judge(verify, proto, p, self_key)[0]
        seen[(proto, disc if f["decodes"] else None, code)] += 1
    assert ms == set(range(33))
    for proto in (GOSSIP, REPAIR):   # every discriminant 0..13 reaches both decoders, and both wrap values the prune rule
        assert {int.from_bytes(f["pkt"][:4], "little") for f in packets if f["proto"] == proto and len(f["pkt"]) >= 4} >= \
            set(range(14))
    assert {2 ** 59 + 1, 2 ** 64 - 1} <= {int.from_bytes(f["pkt"][68:76], "little") for f in packets if f["proto"] == GOSSIP}
    # a valid packet of every judged kind, every unjudged kind, and every code
    for key in [(GOSSIP, 3, 0), (GOSSIP, 4, 0), (GOSSIP, 5, 0), (REPAIR, 8, 0), (REPAIR, 9, 0), (REPAIR, 10, 0)] + \
            [(REPAIR, d, model.UNSUPPORTED) for d in (0, 1, 2, 3, 4, 5, 6, 7, 11)]:
        assert seen[key] >= 1, key
    assert {c for _, _, c in seen} == {model.OK, model.ERR_PARSE, model.UNSUPPORTED, model.ERR_SIGNATURE, model.NOT_FOR_SELF}


def test_rule_edges(oracle):
    verify = model.verifier(oracle)
    for name, proto, p, self_key, want in rule_cases(oracle):
        got = planned(proto, p, self_key)
        assert got == model.signed(proto, p, self_key), name
        code = got[0]
        if code == model.OK:   # the model's verify of what the library planned
            key, sig, msg = got[1]
            code = model.ERR_SIGNATURE if verify(msg, sig, key) != 0 else model.OK
        assert code == want, (name, code, want)
        assert code == model.judge(verify, proto, p, self_key)[0], name
    assert {w for _, _, _, _, w in rule_cases(oracle)} == \
        {model.OK, model.ERR_PARSE, model.UNSUPPORTED, model.ERR_SIGNATURE, model.NOT_FOR_SELF}


def test_mutations(oracle):
    """2,000 seeded mutations: the model's plan for each, and at least 50 in
    each of the five codes"""
    verify = model.verifier(oracle)
    self_key = Node(oracle, 89).pub
    classes = collections.Counter()
    for name, proto, p in mutated(oracle, 2000, 97, self_key):
        got = planned(proto, p, self_key)
        assert got == model.signed(proto, p, self_key), (name, p.hex())
        classes[model.judge(verify, proto, p, self_key)[0]] += 1
    print(dict(classes))
    for c in (model.OK, model.ERR_PARSE, model.UNSUPPORTED, model.ERR_SIGNATURE, model.NOT_FOR_SELF):
        assert classes[c] >= 50, (c, dict(classes))


def test_bad_arguments_and_no_byte_past_the_packet():
    from firedancer_amd.ed25519 import _lib
    plan = ctypes.create_string_buffer(16)
    key = bytes(32)
    assert _lib.fd_ed25519_hip_packet_plan(GOSSIP, None, 0, key, plan) == model.ERR_PARSE
    assert _lib.fd_ed25519_hip_packet_plan(REPAIR, None, 160, key, plan) == model.ERR_PARSE
    assert _lib.fd_ed25519_hip_packet_plan(GOSSIP, b"", 0, key, plan) == model.ERR_PARSE
    for proto in (-1, 2, 255):
        assert _lib.fd_ed25519_hip_packet_plan(proto, bytes(132), 132, key, plan) == -22   # FD_ED25519_HIP_ERR_INVAL
        with pytest.raises(ValueError):
            ed().packet_plan(proto, bytes(132), key)
    assert _lib.fd_ed25519_hip_packet_plan(GOSSIP, bytes(132), 132, None, plan) == -22
    assert _lib.fd_ed25519_hip_packet_plan(GOSSIP, bytes(132), 132, key, None) == -22
