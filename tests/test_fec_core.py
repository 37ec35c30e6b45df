"""fd_ed25519_hip_fec_root (fd_fec_core.h on the host: the rules, the tree and
the proofs the device's tree kernel runs) against the test-side model
(fec_model: hashlib) -- on the reference's captured FEC sets, on every tree
shape and on every rule with its priority.  No GPU."""
import random

import pytest

import fec_model as model
import fec_util as util


@pytest.fixture(scope="module")
def ed():
    from firedancer_amd import ed25519
    return ed25519


def test_captured_sets_reproduce_the_capture(ed, oracle):
    """signatures and proofs blanked, the rebuilt trees give every proof of
    the capture and the roots its signatures sign"""
    from shred_util import fixture
    sets = util.captured_sets()
    assert [len(s) for s in sets] == [64] * 6 + [96] and sum(len(s) for s in sets) == 480
    verified = 0
    for st in sets:
        depth = model.depth_of(len(st))
        assert depth == (6 if len(st) == 64 else 7)
        code, root, proofs = ed.fec_root(util.blank(st))
        assert (code, root, proofs) == model.tree(util.blank(st)) and code == 0
        for s, proof in zip(st, proofs):
            at = model.proof_at(s, depth)
            assert s[at:at + 20 * depth] == proof
            assert ed.shred_root(s) == (0, root)
            verified += 1
        assert model.sign(oracle, root, util.private_key()) == st[0][:64]
        assert oracle.oracle_ed25519_verify(root, 32, st[0][:64], fixture()[1], 0) == 0
    assert verified == 480


def test_depth_of_every_leaf_count(ed):
    for cnt in range(1, 135):
        want = 0 if cnt == 1 else (cnt - 1).bit_length()
        assert ed.fec_depth(cnt) == model.depth_of(cnt) == want
    assert [model.depth_of(c) for c in (1, 2, 3, 4, 5, 64, 65, 128, 129, 134)] == [0, 1, 2, 2, 3, 6, 7, 7, 8, 8]


@pytest.mark.parametrize("cnt", util.SHAPES)
def test_tree_shapes(ed, cnt):
    """the root and all proofs at every leaf count where the tree's shape
    changes; the proofs walk back to the root by the shred front's rules"""
    st = util.make_set(random.Random(1000 + cnt), cnt)
    code, root, proofs = ed.fec_root(st)
    assert (code, root, proofs) == model.tree(st) and code == 0
    assert len(proofs) == cnt and all(len(p) == 20 * model.depth_of(cnt) for p in proofs)
    _, sealed, _, _ = model.seal(None, st, None)
    for s in sealed:
        nz = b"\x01" + s[1:]   # the shred front rejects an all-zero signature, which random bytes are not
        assert ed.shred_root(nz) == (0, root)


def test_data_and_code_splits(ed):
    """the split between data and parity shreds moves the leaf sizes, not the tree"""
    rng = random.Random(7)
    for cnt, data_cnt in ((2, 1), (68, 67), (68, 1), (134, 67), (40, 39), (40, 8)):
        st = util.make_set(rng, cnt, data_cnt=data_cnt)
        assert ed.fec_root(st) == model.tree(st) and model.tree(st)[0] == 0


def test_every_rule_and_its_priority(ed):
    cases = util.bad_sets()
    names = {n for n, _, _ in cases}
    assert {"cnt_0", "cnt_135", "unsupported_then_parse", "parse_then_unsupported", "set_then_parse", "unsupported_then_set",
            "one_shred_parse_first", "one_shred_unsupported_before_set"} <= names
    for name, st, want in cases:
        assert ed.fec_root(st) == (want, None, None), name


def test_zero_signature_is_no_rejection(ed):
    st = util.blank(util.make_set(random.Random(11), 4))
    assert all(s[:64] == bytes(64) for s in st)
    assert ed.fec_root(st)[0] == 0 and ed.shred_root(st[0])[0] == ed.SHRED_ERR_HEADER


def test_mutated_sets(ed):
    seen = set()
    for st in util.mutated_sets()[:600]:
        want = model.tree(list(st))
        assert ed.fec_root(list(st)) == want
        seen.add(want[0])
    assert seen == {0, model.ERR_PARSE, model.UNSUPPORTED, model.ERR_SET}


def test_python_mirror(ed):
    assert (ed.FEC_OK, ed.FEC_ERR_PARSE, ed.FEC_UNSUPPORTED, ed.FEC_ERR_SET) == (0, -16, -18, -19)
    assert ed.FEC_ERR_SET == ed.SHRED_ERR_HEADER and ed.FEC_SET_MAX == 134
    assert ed.fec_work_bytes(262144, 4096) == 140 * 4096 + 4 * 262144 + 16
