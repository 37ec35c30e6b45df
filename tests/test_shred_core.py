"""CPU: fd_ed25519_hip_shred_root (fd_shred_core.h through the library, no
GPU) against the test-side model of the resolver's rules
(tests/shred_model.py): the reference's captured shreds, one case per rule
edge, and seeded mutations."""
import collections

import shred_model as model
from shred_util import every_depth, fixture, mutated, rule_cases


def ed():
    from firedancer_amd import ed25519
    return ed25519


def test_codes_match_the_header():
    e = ed()
    assert (e.SHRED_OK, e.SHRED_ERR_PARSE, e.SHRED_UNSUPPORTED, e.SHRED_ERR_HEADER, e.SHRED_ERR_SIGNATURE) == \
        (model.OK, model.ERR_PARSE, model.UNSUPPORTED, model.ERR_HEADER, model.ERR_SIGNATURE)
    assert e.shred_work_bytes(3) == 110 * 3 + 16


def test_fixture_roots(oracle):
    """all 480 captured shreds: the model's root, which the leader's key
    signed; 7 FEC sets"""
    shreds, pub = fixture()
    assert len(shreds) == 480 and sorted(collections.Counter(len(s) for s in shreds).items()) == [(1203, 240), (1228, 240)]
    assert collections.Counter(s[0x40] for s in shreds) == {0x86: 192, 0x46: 192, 0x87: 48, 0x47: 48}
    roots = set()
    for s in shreds:
        code, root = ed().shred_root(s)
        assert (code, root) == model.root(s) and code == 0
        assert oracle.oracle_ed25519_verify(root, 32, s[:64], pub, 0) == 0
        roots.add(root)
    assert len(roots) == 7


def test_rule_edges(oracle):
    verify = model.verifier(oracle)
    cases, pub = rule_cases(oracle)
    for name, s, want in cases:
        got = ed().shred_root(s)
        assert got == model.root(s), name
        assert got[0] == want, (name, got[0], want)
        if want == model.OK:   # the builder signed the root the model derived
            assert model.judge(verify, s, pub)[0] == model.OK, name
    seen = {w for _, _, w in cases}
    assert seen == {model.OK, model.ERR_PARSE, model.UNSUPPORTED, model.ERR_HEADER}


def test_every_depth(oracle):
    verify = model.verifier(oracle)
    shreds, pub = every_depth(oracle)
    assert {(s[0x40] & 0xF0, s[0x40] & 0xF) for s in shreds} == {(0x80, d) for d in range(16)} | {(0x40, d) for d in range(1, 16)}
    for s in shreds:
        assert ed().shred_root(s) == model.root(s)
        assert model.judge(verify, s, pub)[0] == model.OK


def test_mutations(oracle):
    """2,000 mutated fixture shreds: the model's code and root for each, and
    every reject class reached"""
    verify = model.verifier(oracle)
    _, pub = fixture()
    classes = collections.Counter()
    for s in mutated():
        code, root = model.judge(verify, s, pub)
        got = ed().shred_root(s)
        assert got == model.root(s), s.hex()
        classes[code] += 1
    print(dict(classes))
    for c in (model.ERR_PARSE, model.UNSUPPORTED, model.ERR_HEADER, model.ERR_SIGNATURE):
        assert classes[c] >= 50, (c, dict(classes))


def test_no_byte_is_needed_past_the_shred():
    """an absent shred and an empty one"""
    import ctypes
    from firedancer_amd.ed25519 import _lib
    root = ctypes.create_string_buffer(32)
    assert _lib.fd_ed25519_hip_shred_root(None, 0, root) == model.ERR_PARSE
    assert _lib.fd_ed25519_hip_shred_root(None, 1203, root) == model.ERR_PARSE
    assert ed().shred_root(b"") == (model.ERR_PARSE, None)
