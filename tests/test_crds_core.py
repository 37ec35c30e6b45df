"""CPU: fd_ed25519_hip_crds_count and _crds_plan (fd_crds_core.h through the
library, no GPU) against the test-side model of fd_gossip_recv_crds_value's
rules (tests/crds_model.py) and against the reference decoders' and encoders'
own account (tests/golden/crds.npz): the fixture, one case per rule edge of
each variant, seeded mutations, and the bound on the values of one packet."""
import collections
import ctypes

import crds_model as model
from crds_util import PUSH, Peer, fixture, mutated, packet, rule_cases, u32, u64

CODES = (model.OK, model.UNSUPPORTED, model.ERR_SIGNATURE, model.OWN)


def ed():
    from firedancer_amd import ed25519
    return ed25519


def planned(p, self_key):
    """the library's (packet code, [(discriminant, pre, key, signature, message, value bytes)]) in the model's terms"""
    code, vals = ed().crds_plan(p, self_key)
    assert ed().crds_count(p) == len(vals) and (code == model.OK or not len(vals))
    out = []
    for v in vals:
        s, k, m, n = (int(v[f]) for f in ("sig_off", "key_off", "msg_off", "msg_sz"))
        assert m == s + 64 and max(k + 32, m + n) <= len(p) and int.from_bytes(p[m:m + 4], "little") == int(v["disc"])
        out.append((int(v["disc"]), int(v["pre"]), p[k:k + 32], p[s:s + 64], p[m:m + n], p[s:m + n]))
    return code, out


def test_constants_match_the_header():
    e = ed()
    assert (e.CRDS_OK, e.CRDS_ERR_PARSE, e.CRDS_BAD_RESERVATION, e.CRDS_UNSUPPORTED, e.CRDS_ERR_SIGNATURE, e.CRDS_OWN) == \
        (model.OK, model.ERR_PARSE, model.BAD_RESERVATION, model.UNSUPPORTED, model.ERR_SIGNATURE, model.OWN)
    assert (e.CRDS_VAL_MAX, e.PACKET_MAX) == (model.VAL_MAX, model.MAX)
    assert e.crds_work_bytes(0, 0) == 16 and e.crds_work_bytes(3, 7) == 114 * 7 + 3 + 16
    assert e.CRDS_VAL_DTYPE.itemsize == 16 and e.CRDS_VAL_DTYPE.fields["pre"][1] == 12


def test_fixture_agrees_with_the_reference_decoders_and_encoders(oracle):
    """every packet the reference judged: ERR_PARSE exactly when its decode
    fails or leaves bytes over (but for message discriminants 0, 3, 4, 5,
    UNSUPPORTED unread), its crds_len as the count, every value's data
    discriminant -- and the planned message against the bytes
    fd_crds_data_encode wrote: equal for every value the plan lets through to
    a verify, different for every one it gives UNSUPPORTED"""
    verify = model.verifier(oracle)
    self_key, packets = fixture()
    assert 1500 <= len(packets) <= 5000
    pkt_codes, val_codes, compared = collections.Counter(), collections.Counter(), 0
    lens, discs, data_discs, ok_discs = set(), set(), set(), set()
    for f in packets:
        p = f["pkt"]
        assert len(p) <= model.MAX
        got = planned(p, self_key)
        assert got == model.signed(p, self_key), p.hex()
        disc = int.from_bytes(p[:4], "little") if len(p) >= 4 else None
        discs.add(disc)
        if disc in (0, 3, 4, 5):
            assert got[0] == model.UNSUPPORTED
        else:
            assert (got[0] == model.ERR_PARSE) == (not f["decodes"]), p.hex()
        if got[0] == model.OK:
            assert len(got[1]) == f["crds_len"] == len(f["vals"])
            lens.add(f["crds_len"])
            for (d, pre, _, _, msg, _), (ref_disc, enc, equal) in zip(got[1], f["vals"]):
                assert d == ref_disc
                assert equal == (msg == enc)                      # the generator's flag is about these bytes
                assert equal == (pre != model.UNSUPPORTED) or pre == model.OWN, (d, pre, equal)
                assert equal == (d != 11)
                if pre == model.OK:
                    assert msg == enc                             # what reaches a verify is what the reference would hash
                ok_discs.add(d)
                compared += 1
        else:
            assert not f["vals"] or disc not in (1, 2)
        if disc in (1, 2) and len(p) >= 112:                      # the data discriminants tried, at the first value's place
            data_discs.add(int.from_bytes(p[108:112], "little"))
        code, judged = model.judge(verify, p, self_key)
        pkt_codes[code] += 1
        val_codes.update(v[0] for v in judged)
    assert compared == sum(len(f["vals"]) for f in packets if int.from_bytes(f["pkt"][:4], "little") in (1, 2)) >= 1000
    assert lens == set(range(model.VAL_MAX + 1)) and ok_discs == set(range(12))
    assert discs >= set(range(14)) and data_discs >= set(range(14))
    assert {2 ** 59 + 1, 2 ** 64 - 1} <= {int.from_bytes(f["pkt"][36:44], "little") for f in packets}
    print(dict(pkt_codes), dict(val_codes))
    for c in (model.OK, model.ERR_PARSE, model.UNSUPPORTED):
        assert pkt_codes[c] >= 50, (c, dict(pkt_codes))
    for c in CODES:
        assert val_codes[c] >= 50, (c, dict(val_codes))


def test_rule_edges(oracle):
    verify = model.verifier(oracle)
    seen = set()
    for name, p, self_key, want_pkt, want_vals in rule_cases(oracle):
        got = planned(p, self_key)
        assert got == model.signed(p, self_key), name
        codes = tuple(pre or (model.ERR_SIGNATURE if verify(msg, sig, key) != 0 else model.OK)
                      for _, pre, key, sig, msg, _ in got[1])     # the model's verify of what the library planned
        assert (got[0], codes) == (want_pkt, want_vals), (name, got[0], codes)
        judged = model.judge(verify, p, self_key)
        assert (judged[0], tuple(v[0] for v in judged[1])) == (want_pkt, want_vals), name
        seen |= {want_pkt} | set(want_vals)
    assert seen == {model.OK, model.ERR_PARSE, model.UNSUPPORTED, model.ERR_SIGNATURE, model.OWN}


def test_mutations(oracle):
    """2,000 further seeded mutations: the model's plan for each, and at least
    50 in each packet code and each value code"""
    verify = model.verifier(oracle)
    me = Peer(oracle, 239)
    pkt_codes, val_codes = collections.Counter(), collections.Counter()
    for name, p in mutated(oracle, 2000, 241, me):
        got = planned(p, me.pub)
        assert got == model.signed(p, me.pub), (name, p.hex())
        code, judged = model.judge(verify, p, me.pub)
        pkt_codes[code] += 1
        val_codes.update(v[0] for v in judged)
    print(dict(pkt_codes), dict(val_codes))
    for c in (model.OK, model.ERR_PARSE, model.UNSUPPORTED):
        assert pkt_codes[c] >= 50, (c, dict(pkt_codes))
    for c in CODES:
        assert val_codes[c] >= 50, (c, dict(val_codes))


def test_val_max_holds(oracle):
    """a packet of VAL_MAX smallest values decodes, one more cannot fit, and
    no variant encodes shorter than the one the bound is derived from"""
    pr = Peer(oracle, 251)
    small = pr.version(6)
    assert 64 + len(small) == 115 == min(64 + len(d) for _, d in pr.every_variant())
    assert model.VAL_MAX == (model.MAX - 44) // 115
    p = packet(pr, [small] * model.VAL_MAX)
    assert len(p) <= model.MAX and ed().crds_count(p) == model.VAL_MAX and model.walk(p)[0] == model.OK
    more = u32(PUSH) + pr.pub + u64(model.VAL_MAX + 1) + p[44:] + p[44:44 + 115]
    assert len(more) > model.MAX
    for q in (more, more[:model.MAX]):
        assert ed().crds_count(q) == 0 and ed().crds_plan(q, pr.pub)[0] == model.ERR_PARSE == model.walk(q)[0]
    assert ed().crds_plan(p, pr.pub)[1]["pre"].tolist() == [model.OWN] * model.VAL_MAX


def test_bad_arguments_and_no_byte_past_the_packet():
    from firedancer_amd.ed25519 import _lib
    vals = ctypes.create_string_buffer(16 * 10)
    code, key = ctypes.c_byte(1), bytes(32)
    assert _lib.fd_ed25519_hip_crds_count(None, 0) == 0 and _lib.fd_ed25519_hip_crds_count(None, 200) == 0
    assert _lib.fd_ed25519_hip_crds_plan(None, 200, key, vals, 10, ctypes.byref(code)) == 0 and code.value == model.ERR_PARSE
    assert _lib.fd_ed25519_hip_crds_plan(bytes(200), 200, None, vals, 10, ctypes.byref(code)) == -22   # FD_ED25519_HIP_ERR_INVAL
    p = u32(PUSH) + bytes(32) + u64(0)
    assert _lib.fd_ed25519_hip_crds_plan(p, len(p), key, None, 0, ctypes.byref(code)) == 0 and code.value == model.OK
    assert _lib.fd_ed25519_hip_crds_plan(p, len(p), key, None, 0, None) == 0
