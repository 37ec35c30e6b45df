"""GPU: shredding entry batches (fd_ed25519_hip_shredder_host / _front_dev /
_dev, include/fd_ed25519_hip.h Part 2j) against the reference's captured
shreds, the reference shredder's own sets (tests/golden/shredder.npz) and the
test-side model (shredder_model on reedsol_model and fec_model).  A small
engine: compact tables, 512-signature chunks."""
import numpy as np
import pytest

import fec_model
import fec_util
import poh_util
import shredder_model as model
import shredder_util as util
from shred_util import fixture

pytestmark = pytest.mark.gpu


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
def capture_sets(eng, ed):
    """the capture's batch through shredder_host with the capture's key"""
    blk = poh_util.captured_block()
    return eng.shredder_host([blk], [ed.shredder_desc(block_complete=1)], fec_util.private_key())


def test_capture(eng, capture_sets):
    """480 shreds byte for byte from the batch, the key and five numbers; every one passes the shred front"""
    codes, sets, roots, sigs = capture_sets
    assert codes.tolist() == [0] and [len(s) for s in sets] == [64] * 6 + [96]
    assert tuple(tuple(s) for s in sets) == fec_util.captured_sets()
    flat = [s for st in sets for s in st]
    assert len(flat) == 480 and sorted(flat) == sorted(fixture()[0])
    assert all(sigs[k].tobytes() == st[0][:64] for k, st in enumerate(sets))
    front, _ = eng.shreds_host(flat, fixture()[1])
    assert len(front) == 480 and not front.any()


def fixture_batches():
    """every batch of the fixture with its descriptor and digests, in one list"""
    return [b for case in util.fixture_cases() for b in case]


def test_fixture_host(eng, ed, oracle):
    """every fixture case through shredder_host: without keys the reference's
    shreds (its signer wrote zeros), by digest; with a key per batch the
    model's"""
    bs = fixture_batches()
    descs = [util.ed_desc(ed, b[1]) for b in bs]
    codes, sets, roots, sigs = eng.shredder_host([b[0] for b in bs], descs, None)
    assert not codes.any() and sigs is None
    assert [(sum(s[0x40] & 0xF0 == 0x80 for s in st), sum(s[0x40] & 0xF0 == 0x40 for s in st)) for st in sets] == \
        [dp for b in bs for dp in b[3]]
    assert util.digests(sets) == [d for b in bs for d in b[4]]
    small = bs[:5]
    keys = util.keys(331, len(small))
    codes, sets, roots, sigs = eng.shredder_host([b[0] for b in small], descs[:5], keys)
    want = [st for b, k in zip(small, keys) for st in model.shred(oracle, b[0], b[1], k)]
    assert not codes.any() and sets == want
    assert [r.tobytes() for r in roots] == [fec_model.tree(st)[1] for st in want]
    assert [s.tobytes() for s in sigs] == [st[0][:64] for st in want]


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_fixture_placement_and_guard(eng, ed, oracle, lead):
    """every fixture batch in one front_dev call, the batches from byte `lead`
    of buf on and 3 guard bytes apart, the shreds 1229 bytes apart from byte
    16 + lead: the guard-filled buffers afterwards are the model's layout --
    gaps, parity regions and tails unchanged --, and fec_parity_dev and
    fec_seal_dev over the same arrays give the reference's shreds (no keys)
    or the model's (keys)"""
    bs = fixture_batches()
    batches, descs = [b[0] for b in bs], [b[1] for b in bs]
    res = util.Reservation([len(b) for b in batches])
    out = util.run_front(eng, ed, batches, descs, res, base_off=16 + lead, stride=1229, lead=lead)
    try:
        starts = [int(o) for o in out["shred_off"][:res.n]]
        assert {o % 4 for o in starts} == {0, 1, 2, 3} and {o % 16 for o in starts} == set(range(16))
        fronts = [model.front(b, d) for b, d in zip(batches, descs)]
        util.assert_layout(out, util.expect_layout(out, res, fronts, [0] * len(bs)), parity_untouched=True)
        with_keys = lead % 2 == 1
        batch_keys = util.keys(337 + lead, len(bs)) if with_keys else [None] * len(bs)
        set_keys = [k for b, k in zip(batches, batch_keys) for _ in range(model.count(len(b))[0])] if with_keys else None
        pcodes, scodes, got = util.parity_and_seal(eng, ed, out, set_keys)
        assert not any(pcodes) and not any(scodes)
        done = [model.shred(oracle, b, d, k) for b, d, k in zip(batches, descs, batch_keys)]
        if not with_keys:
            assert [util.digests(sets) for sets in done] == [b[4] for b in bs]
        out["shreds"] = got
        util.assert_layout(out, util.expect_layout(out, res, done, [0] * len(bs)))
    finally:
        util.free(out)


GOOD = (1, 1016, 9136, 63681)


def test_mixed_batches(eng, ed, oracle):
    """good batches of 1, 1016, 9136 and 63681 bytes with a zero-size batch, a
    batch that leaves buf, wrong reservations and a shred_first_b that runs
    backwards among them, the two-set batch right behind the backwards entry:
    their codes, nothing written for them, FEC_ERR_SET from the parity and the
    seal for their sets -- FEC_ERR_PARSE for the first set of a wrong
    reservation of 1 to 134 shreds, which cannot be an empty range between two
    good batches -- and every good batch as if alone"""
    sizes = [1, 0, 1016, 130000, 9136, 1016, 1016, 63681, 1016, 1]
    #           ^zero    ^leaves buf   ^60 shreds (20 are right), ^backwards  ^1 set, 17 shreds
    batches = [model.seeded_batch(347 + b, sz) for b, sz in enumerate(sizes)]
    descs = [model.desc(slot=9, data_idx=1000 * b, parity_idx=2000 * b, version=b, reference_tick=b, block_complete=b & 1)
             for b in range(len(sizes))]
    res = util.Reservation(sizes, reserve={8: (1, 17)})
    assert res.shred_first_b == [0, 18, 18, 38, 302, 335, 355, 375, 505, 522, 540]
    # batch 5 holds [335, 395), batch 6 [395, 375) and batch 7 its own 130 behind it; nobody writes [335, 375)
    res.shred_first_b[6] = 395
    bad = model.BAD_RESERVATION
    want_codes = [0, model.ERR_BATCH, 0, model.ERR_BATCH, 0, bad, bad, 0, bad, 0]
    assert want_codes == [model.judge(sz if b != 3 else 1 << 30, 0, 1 << 20, res.set_first_b[b], res.set_first_b[b + 1], res.n_set,
                                      res.shred_first_b[b], res.shred_first_b[b + 1], res.n) for b, sz in enumerate(sizes)]
    out = util.run_front(eng, ed, batches, descs, res, base_off=17, stride=1230, lead=1, leave=(3,))
    try:
        fronts = [model.front(b, d) if not c else None for b, d, c in zip(batches, descs, want_codes)]
        util.assert_layout(out, util.expect_layout(out, res, fronts, want_codes), parity_untouched=True)
        pcodes, scodes, got = util.parity_and_seal(eng, ed, out)
        want_sets = []
        for b, c in enumerate(want_codes):
            sets = res.set_first_b[b + 1] - res.set_first_b[b]
            want_sets += [0 if not c else fec_model.ERR_PARSE if b in (5, 8) else fec_model.ERR_SET] * sets
        # the four sets of the batch that leaves buf (264 shreds, then empty ranges) and the backwards range [395, 375)
        assert model.count(130000)[0] == 4 and want_sets.count(fec_model.ERR_SET) == 5
        assert pcodes == want_sets and scodes == want_sets
        done = [model.shred(oracle, b, d, None) if not c else None for b, d, c in zip(batches, descs, want_codes)]
        out["shreds"] = got
        util.assert_layout(out, util.expect_layout(out, res, done, want_codes))
    finally:
        util.free(out)


def test_first_b_that_runs_backwards(eng, ed, oracle):
    """a shred_first_b that runs backwards and a set_first_b that leaves
    [0, n_set): BAD_RESERVATION for the batches it spoils, nothing written for
    them, their sets rejected by the parity and the seal, and the batch in
    front of them as if alone"""
    sizes = [1, 1016, 9136]
    batches = [model.seeded_batch(353 + b, sz) for b, sz in enumerate(sizes)]
    descs = [model.desc(slot=2, data_idx=7 * b) for b in range(3)]
    res = util.Reservation(sizes)
    assert res.shred_first_b == [0, 18, 38, 71] and res.set_first_b == [0, 1, 2, 3]
    hfb = [0, 18, 10, 71]       # batch 1 runs backwards, batch 2 holds 61 shreds for its 33
    out = util.run_front(eng, ed, batches, descs, res, shred_first_b=hfb)
    try:
        codes = [model.judge(sz, 0, 1 << 20, res.set_first_b[b], res.set_first_b[b + 1], 3, hfb[b], hfb[b + 1], 71)
                 for b, sz in enumerate(sizes)]
        assert codes == [0, model.BAD_RESERVATION, model.BAD_RESERVATION]
        assert out["batch_out"][:3].tolist() == codes
        assert out["set_first"][:4].tolist() == [0, 18, 10, 71]
        assert out["shred_sz"][:71].tolist() == [1203] + [1228] * 17 + [0] * 53
        pcodes, scodes, got = util.parity_and_seal(eng, ed, out)
        assert pcodes[0] == 0 and scodes[0] == 0 and all(pcodes[1:]) and all(scodes[1:])
        res1 = util.Reservation(sizes)
        want = util.expect_layout(out, res1, [model.shred(oracle, batches[0], descs[0], None), None, None], codes)
        assert got == want["shreds"]
    finally:
        util.free(out)
    sfb = [0, 1, 5, 3]          # batch 1 leaves [0, n_set), batch 2 runs backwards
    out = util.run_front(eng, ed, batches, descs, res, set_first_b=sfb)
    try:
        assert out["batch_out"][:3].tolist() == [0, model.BAD_RESERVATION, model.BAD_RESERVATION]
        assert out["shred_sz"][:71].tolist() == [1203] + [1228] * 17 + [0] * 53
        assert (out["shred_off"][18:] == 0x5A5A5A5A5A5A5A5A).all() and out["set_first"][3] == 71
        pcodes, scodes, got = util.parity_and_seal(eng, ed, out)
        assert pcodes[0] == 0 and scodes[0] == 0 and all(pcodes[1:]) and all(scodes[1:])
        assert got == want["shreds"]
    finally:
        util.free(out)


def test_composition(eng, ed, oracle):
    """shredder_dev -- front, parity and seal on one stream, one sync -- gives
    what the three calls give: the model's finished shreds under each batch's
    key, roots and signatures per set, with a rejected batch among them"""
    sizes = [63681, 1, 0, 9136, 1016]
    batches = [model.seeded_batch(359 + b, sz) for b, sz in enumerate(sizes)]
    descs = [model.desc(slot=4, data_idx=300 * b, parity_idx=400 * b, block_complete=1) for b in range(len(sizes))]
    keys = util.keys(367, len(sizes))
    res = util.Reservation(sizes)
    codes = [0, 0, model.ERR_BATCH, 0, 0]
    for privs in (keys, None):
        out = util.run_front(eng, ed, batches, descs, res, base_off=32, stride=1228, privs=privs, seal=True)
        try:
            done = [model.shred(oracle, b, d, k if privs else None) if not c else None for b, d, k, c in zip(batches, descs, keys, codes)]
            util.assert_layout(out, util.expect_layout(out, res, done, codes))
            sets = [st for x in done if x for st in x]
            assert out["set_out"].tolist() == [0] * res.n_set + [util.GUARD] * out["tail"]
            assert out["roots"].tobytes() == b"".join(fec_model.tree(st)[1] for st in sets) + bytes([util.GUARD] * 32 * out["tail"])
            if privs:
                assert out["sigs"].tobytes() == b"".join(st[0][:64] for st in sets) + bytes([util.GUARD] * 64 * out["tail"])
        finally:
            util.free(out)


@pytest.mark.parametrize("nb", [1, 257])
def test_edge_counts(eng, ed, nb):
    """nb batches of 1 byte, 18 shreds each, chained in one slot"""
    batches = [bytes([b & 0xFF]) for b in range(nb)]
    descs = [model.desc(slot=1, data_idx=b, parity_idx=17 * b, block_complete=b == nb - 1) for b in range(nb)]
    codes, sets, roots, sigs = eng.shredder_host(batches, [util.ed_desc(ed, d) for d in descs], None)
    assert not codes.any() and len(sets) == nb and all(len(st) == 18 for st in sets)
    assert sets == [st for b, d in zip(batches, descs) for st in model.shred(None, b, d, None)]


@pytest.mark.parametrize("nb", [1, 3])
def test_host_with_zero_size_batches_alone(eng, ed, nb):
    """shredder_host on batches of no bytes and nothing else: every batch its
    own code, no set, and the call itself succeeds (no pass runs)"""
    for privs in (None, fec_util.private_key()):
        codes, sets, roots, sigs = eng.shredder_host([b""] * nb, [ed.shredder_desc(slot=3)] * nb, privs)
        assert codes.tolist() == [model.ERR_BATCH] * nb == [-19] * nb
        assert sets == [] and len(roots) == 0 and (sigs is None or len(sigs) == 0)


def test_host_zero_size_batches_among_good_ones(eng, ed):
    """... and in front of, between and behind good batches they take no set and change no other batch's shreds"""
    batches = [b"", b"\x07", b"", b"", model.seeded_batch(379, 1016), b""]
    descs = [model.desc(slot=5, data_idx=40 * b, parity_idx=50 * b) for b in range(len(batches))]
    codes, sets, roots, sigs = eng.shredder_host(batches, [util.ed_desc(ed, d) for d in descs], None)
    assert codes.tolist() == [model.ERR_BATCH, 0, model.ERR_BATCH, model.ERR_BATCH, 0, model.ERR_BATCH]
    assert sets == model.shred(None, batches[1], descs[1], None) + model.shred(None, batches[4], descs[4], None)


def test_two_host_passes(eng, ed):
    """more than one pass of shredder_host (16,384 shreds), the boundary
    inside a batch of 700,000 bytes (20 sets of 64 and one of 134): 112
    batches of 63,679 bytes (134 shreds each), the large one, two more -- by
    digest against the model"""
    sizes = [63679] * 112 + [700000] + [63679] * 2
    assert model.count(700000) == (21, 707, 707) and model.count(63679) == (1, 67, 67)
    assert 112 * 134 + 20 * 64 < 16384 < 112 * 134 + 20 * 64 + 134
    rng_batches = [model.seeded_batch(373 + b, sz) for b, sz in enumerate(sizes)]
    descs, D = [], 0
    for sz in sizes:
        descs.append(model.desc(slot=6, data_idx=D, parity_idx=D, version=77, reference_tick=3))
        D += model.count(sz)[1]
    codes, sets, roots, sigs = eng.shredder_host(rng_batches, [util.ed_desc(ed, d) for d in descs], None)
    assert not codes.any() and sum(len(st) for st in sets) == 114 * 134 + 1414
    want = [st for b, d in zip(rng_batches, descs) for st in model.shred(None, b, d, None)]
    assert util.digests(sets) == util.digests(want)


def test_other_direction(eng, capture_sets):
    """fec_recover_host on shredder-made sets with every other slot erased,
    then the seal without keys for the proofs: the sets again"""
    _, sets, _, _ = capture_sets
    erased = [[j % 2 for j in range(len(st))] for st in sets]
    holed = [[bytes(len(s)) if e else s for s, e in zip(st, er)] for st, er in zip(sets, erased)]
    codes, got = eng.fec_recover_host(holed, erased)
    assert not codes.any()
    codes, got, _, _ = eng.fec_seal_host(got, None)
    assert not codes.any() and [[bytes(s) for s in st] for st in got] == sets


def host_with_keys(eng, ed, oracle, sizes, seed):
    """shredder_host on seeded batches of these sizes chained in one slot, a
    key per batch, by digest against the model: shreds, roots, signatures"""
    batches = [model.seeded_batch(seed + b, sz) for b, sz in enumerate(sizes)]
    descs, D = [], 0
    for sz in sizes:
        descs.append(model.desc(slot=6, data_idx=D, parity_idx=D, version=77, reference_tick=3))
        D += model.count(sz)[1]
    keys = util.keys(seed, len(sizes))
    codes, sets, roots, sigs = eng.shredder_host(batches, [util.ed_desc(ed, d) for d in descs], keys)
    want = [st for b, d, k in zip(batches, descs, keys) if b for st in model.shred(oracle, b, d, k)]
    assert codes.tolist() == [0 if sz else model.ERR_BATCH for sz in sizes]
    assert [len(st) for st in sets] == [len(st) for st in want]
    assert util.digests(sets) == util.digests(want)
    assert util.digests([[r.tobytes() for r in roots]]) == util.digests([[fec_model.tree(st)[1] for st in want]])
    assert util.digests([[s.tobytes() for s in sigs]]) == util.digests([[st[0][:64] for st in want]])


def test_host_pass_ends_in_front_of_a_batch_with_keys(eng, ed, oracle):
    """the first pass of shredder_host stops exactly in front of a batch --
    122 batches of 63,679 bytes are 16,348 shreds, and the next 134 do not
    fit -- with a batch of no bytes at the boundary: the second pass starts
    at a batch that is not the call's first, and signs with that batch's key"""
    assert model.count(63679) == (1, 67, 67) and 122 * 134 <= 16384 < 123 * 134
    host_with_keys(eng, ed, oracle, [63679] * 122 + [0, 63679], 383)


def test_two_host_passes_with_keys(eng, ed, oracle):
    """the sizes of test_two_host_passes: the second pass starts inside batch
    112, whose key both passes sign with"""
    assert 112 * 134 + 20 * 64 < 16384 < 112 * 134 + 20 * 64 + 134
    host_with_keys(eng, ed, oracle, [63679] * 112 + [700000] + [63679] * 2, 389)
