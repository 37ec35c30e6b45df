"""fd_ed25519_hip_poh and fd_ed25519_hip_poh_prepare (fd_poh_core.h on the
host: the rules the device's kernels run and the block walk) against the
test-side model (poh_model: hashlib) and against the reference's own output
(tests/golden/poh.npz, and the batch the captured shreds carry).  No GPU."""
import random
import struct

import numpy as np
import pytest

import poh_model as model
import poh_util as util


@pytest.fixture(scope="module")
def ed():
    from firedancer_amd import ed25519
    return ed25519


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_codes_are_the_public_ones(ed):
    assert (ed.POH_ERR_PARSE, ed.POH_UNSUPPORTED, ed.POH_ERR_HASH) == (-16, -18, -25)
    assert (model.ERR_PARSE, model.UNSUPPORTED, model.ERR_HASH) == (-16, -18, -25)
    assert ed.POH_HASH_CNT_CEIL == model.CEIL == 1 << 17
    assert b"proof of history" in ed.library().fd_ed25519_hip_strerror(-25)


def test_model_reproduces_the_reference():
    g = util.golden()
    assert int(g["cases"]) == 1536
    for s in range(1, 131):
        assert model.root([x.tobytes() for x in g["sigs"][:s]]) == g["roots"][s - 1].tobytes(), s
    assert tuple(int(k) for k in g["append_k"]) == util.KS
    for k, out in zip(g["append_k"], g["append_out"]):
        assert model.append(g["append_in"].tobytes(), int(k)) == out.tobytes(), k
    for a, r, out in zip(g["mix_in"], g["mix_root"], g["mix_out"]):
        assert model.sha(a.tobytes() + r.tobytes()) == out.tobytes()
    d, verdicts, states, kinds = util.fixture_microblocks()
    assert set(kinds) == set(util.KINDS)
    codes, got = d.want()
    assert np.array_equal(codes, verdicts) and np.array_equal(got, states)
    assert all((v == 0) == (k in ("good", "hash_cnt_0_txns", "hash_cnt_1_txns", "hash_cnt_0_tick"))
               for v, k in zip(verdicts, kinds))


def test_every_signature_count_of_the_fixture(ed):
    """the first S seeded signatures, S = 1..130: the state of a microblock
    whose in state is zero and whose k is 0 is SHA256( 0 || root )"""
    g = util.golden()
    sigs = b"".join(x.tobytes() for x in g["sigs"])
    hdr = struct.pack("<Q", 1) + bytes(32) + struct.pack("<Q", 1)
    buf = bytes(32) + hdr + sigs
    n = 130
    first = np.zeros(n + 1, np.uint32)
    codes, states = ed.poh_verify(buf, [32] * n, [0] * n, first, [80 + 64 * j for j in range(130)])
    assert set(codes.tolist()) == {model.ERR_PARSE}       # transactions and no signature
    # one descriptor per S: the range [0, S) cannot be said with one sig_first array, so one call each
    for s in range(1, 131):
        codes, states = ed.poh_verify(buf, [32], [0], [0, s], [80 + 64 * j for j in range(130)])
        assert codes[0] == model.ERR_HASH
        assert states[0].tobytes() == model.sha(bytes(32) + g["roots"][s - 1].tobytes()), s


def test_every_k_of_the_fixture(ed):
    g = util.golden()
    for k, out in zip(g["append_k"], g["append_out"]):
        buf = g["append_in"].tobytes() + struct.pack("<Q", int(k)) + out.tobytes() + struct.pack("<Q", 0)
        codes, states = ed.poh_verify(buf, [32], [0], [0, 0], [])
        assert codes[0] == 0 and states[0].tobytes() == out.tobytes(), k


def test_fixture_microblocks(ed):
    d, verdicts, states, _ = util.fixture_microblocks()
    codes, got = ed.poh_verify(*d.args())
    assert np.array_equal(codes, verdicts) and np.array_equal(got, states)


def test_shapes_and_broken_ones(ed):
    d = util.shapes()
    assert same(ed.poh_verify(*d.args()), d.want())
    assert set(d.want()[0].tolist()) == {0}
    b, touched = util.broken(d)
    want = b.want(4096)
    assert same(ed.poh_verify(*b.args(), hash_cnt_max=4096), want)
    assert {model.ERR_PARSE, model.UNSUPPORTED, model.ERR_HASH} == set(want[0][touched].tolist())
    rest = [i for i in range(d.n) if i not in touched]
    assert not want[0][rest].any()


def test_captured_batch(ed):
    g, blk = util.golden(), util.captured_block()
    code, hdr, inn, first, sig = ed.poh_prepare(blk)
    want = model.walk(blk)
    assert code == 0 and len(hdr) == 64 and len(sig) == 1280
    assert (list(hdr), list(inn), list(first), list(sig)) == want[1:]
    assert all(int(inn[i]) == int(hdr[i - 1]) + 8 for i in range(1, 64))
    d = util.captured()
    codes, states = ed.poh_verify(*d.args())
    assert not codes[1:].any()
    assert np.array_equal(codes, g["cap_verdict"]) and np.array_equal(states, g["cap_state"])
    # the capture's first microblock chains from the zero hash; from any other it does not
    assert codes[0] == 0
    other = util.describe(blk, b"\x01" + bytes(31))
    codes, _ = ed.poh_verify(*other.args())
    assert codes.tolist() == [model.ERR_HASH] + [0] * 63


def one(hash_cnt, txn_cnt, n_sig, hdr_hash=bytes(32)):
    """a lone microblock: in state at 0, header at 32, signatures from 80"""
    buf = bytes(32) + struct.pack("<Q", hash_cnt) + hdr_hash + struct.pack("<Q", txn_cnt) + bytes(64 * n_sig)
    return buf, [32], [0], [0, n_sig], [80 + 64 * j for j in range(n_sig)]


def test_rule_priority(ed):
    huge = (1 << 64) - 1
    # parse before unsupported: a hash count over the bound in a descriptor that is wrong
    for buf, hdr, inn, first, sig in (one(huge, 0, 1), one(huge, 1, 0)):
        assert ed.poh_verify(buf, hdr, inn, first, sig, hash_cnt_max=16)[0][0] == model.ERR_PARSE
    buf, hdr, inn, first, sig = one(huge, 1, 1)
    assert ed.poh_verify(buf, hdr, inn, first, [len(buf) - 63], hash_cnt_max=16)[0][0] == model.ERR_PARSE
    assert ed.poh_verify(buf, [len(buf) - 47], inn, first, sig, hash_cnt_max=16)[0][0] == model.ERR_PARSE
    assert ed.poh_verify(buf, hdr, [len(buf) - 31], first, sig, hash_cnt_max=16)[0][0] == model.ERR_PARSE
    assert ed.poh_verify(buf, hdr, inn, [1, 0], sig, hash_cnt_max=16)[0][0] == model.ERR_PARSE
    assert ed.poh_verify(buf, hdr, inn, [0, 2], sig, hash_cnt_max=16)[0][0] == model.ERR_PARSE
    # unsupported before hash: the header's hash is wrong too
    codes, states = ed.poh_verify(buf, hdr, inn, first, sig, hash_cnt_max=16)
    assert codes[0] == model.UNSUPPORTED and not states.any()
    # offsets that would wrap
    assert ed.poh_verify(buf, [huge - 8], inn, first, sig)[0][0] == model.ERR_PARSE
    assert ed.poh_verify(buf, hdr, inn, first, [huge - 8])[0][0] == model.ERR_PARSE


@pytest.mark.parametrize("txn_cnt", [0, 1])
def test_bound_at_k_minus_1_k_and_k_plus_1(ed, txn_cnt):
    k = 37
    hash_cnt = k + (1 if txn_cnt else 0)
    state = model.append(bytes(32), k)
    if txn_cnt:
        state = model.mixin(state, [bytes(64)])
    args = one(hash_cnt, txn_cnt, txn_cnt, state)
    assert ed.poh_verify(*args, hash_cnt_max=k - 1)[0][0] == model.UNSUPPORTED
    for bound in (k, k + 1):
        codes, states = ed.poh_verify(*args, hash_cnt_max=bound)
        assert codes[0] == 0 and states[0].tobytes() == state


def test_a_hash_count_of_all_ones_returns_at_once(ed):
    huge = (1 << 64) - 1
    for txn_cnt in (0, 1):
        assert ed.poh_verify(*one(huge, txn_cnt, txn_cnt))[0][0] == model.UNSUPPORTED
        assert ed.poh_verify(*one(huge, txn_cnt, txn_cnt), hash_cnt_max=0)[0][0] == model.UNSUPPORTED
    with pytest.raises(ed.HipError):
        ed.poh_verify(*one(1, 0, 0), hash_cnt_max=(1 << 17) + 1)
    assert ed.poh_verify(*one(1, 0, 0), hash_cnt_max=1 << 17)[0][0] == model.ERR_HASH


def check_walk(ed, blk, first_in_off=0):
    want = model.walk(blk, first_in_off)
    got = ed.poh_prepare(blk, first_in_off)
    assert got[0] == want[0]
    if want[0] == 0:
        assert [list(map(int, x)) for x in got[1:]] == [list(x) for x in want[1:]]
    return want[0]


def test_prepare_on_truncations(ed):
    blk = util.captured_block()
    seen = set()
    for cut in util.truncation_cuts(blk):
        seen.add(check_walk(ed, blk[:cut]))
        assert (model.walk(blk[:cut])[0] == 0) == (cut in (0, len(blk))), cut
    assert seen == {0, model.ERR_PARSE}


def test_prepare_on_hostile_counts_and_junk(ed):
    blk = util.captured_block()
    for cnt in (0, 1 << 63, (1 << 64) - 1, 65):
        assert check_walk(ed, struct.pack("<Q", cnt) + blk[8:]) == model.ERR_PARSE
    assert check_walk(ed, struct.pack("<Q", 63) + blk[8:]) == model.ERR_PARSE     # the 64th is junk: no batch count parses
    for junk in (b"\0", bytes(7), bytes(8), struct.pack("<Q", 1), struct.pack("<Q", 1) + bytes(47)):
        assert check_walk(ed, blk + junk) == model.ERR_PARSE
    assert check_walk(ed, blk + struct.pack("<Q", 1) + bytes(48)) == 0             # a tick of hash_cnt 0: a second batch
    assert check_walk(ed, b"") == 0
    # a transaction count the bytes cannot hold
    rng = random.Random(281)
    mb, _ = util.make_microblock(rng, bytes(32), 2, 3)
    for txn_cnt in (1 << 63, (1 << 64) - 1, 4):
        bad = bytearray(struct.pack("<Q", 1) + mb)
        struct.pack_into("<Q", bad, 8 + 0x28, txn_cnt)
        assert check_walk(ed, bytes(bad)) == model.ERR_PARSE


def test_prepare_on_two_batches(ed):
    rng = random.Random(283)
    in_state = bytes(rng.getrandbits(8) for _ in range(32))
    blk = util.two_batches(rng, in_state)
    assert check_walk(ed, blk, first_in_off=12345) == 0
    code, hdr, inn, first, sig = ed.poh_prepare(blk, 12345)
    assert len(hdr) == 5 and int(inn[0]) == 12345
    assert [int(x) for x in inn[1:]] == [int(h) + 8 for h in hdr[:-1]]          # across the batch boundary too
    assert int(hdr[3]) - int(hdr[2]) == 48 + 8                                   # the second batch's count between
    assert first.tolist() == [0, 2, 2, 2, 3, 15]
    d = util.describe(blk, in_state)
    codes, states = ed.poh_verify(*d.args())
    assert not codes.any() and same((codes, states), d.want())


def test_mutated_blocks(ed):
    blocks = util.mutated(400)
    seen = {check_walk(ed, b) for b in blocks}
    assert seen == {0, model.ERR_PARSE}
