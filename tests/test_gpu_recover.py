"""GPU: recovering received FEC sets (fd_ed25519_hip_fec_recover_host / _dev,
include/fd_ed25519_hip.h Part 2h) against the test-side model (recover_model:
the Lagrange formula over the first d received slots), the reference
decoder's own output (tests/golden/reedsol_recover.npz) and, with the seal
without keys (Part 2f) and the shred front (Part 2c) behind it, against the
reference's captured shreds.  A small engine: compact tables, 512-signature
chunks."""
import random

import numpy as np
import pytest

import fec_model
import fec_util
import recover_model as model
import recover_util as util
import reedsol_model as rs
from recover_util import back_to_back, expect, run_dev, written_d
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


def check_host(eng, sets, masks, want=None):
    want = expect(sets, masks) if want is None else want
    codes, got = eng.fec_recover_host([list(s) for s in sets], masks)
    assert codes.tolist() == [w[0] for w in want]
    for k, w in enumerate(want):
        assert [bytes(s) for s in got[k]] == list(w[1]), k
    return want


def seal_and_verify(eng, sets):
    """fec_seal_host without keys (proofs only), then shreds_host under the capture's leader"""
    codes, got, _, sigs = eng.fec_seal_host(sets, None)
    assert not codes.any() and sigs is None
    flat = [bytes(s) for st in got for s in st]
    front, _ = eng.shreds_host(flat, fixture()[1])
    return flat, front


def test_capture_end_to_end(eng):
    """half of every captured set's slots zeroed whole: recover, seal without keys, verify under the capture's
    leader -- the reference's own 480 shreds byte for byte and 480 zeros"""
    cases = util.captured("mixed")
    whole = [s for _, _, st in cases for s in st]
    assert [len(st) for _, st, _ in cases] == [64] * 6 + [96] and sum(sum(m) for m, _, _ in cases) == 240
    codes, got = eng.fec_recover_host([st for _, st, _ in cases], [m for m, _, _ in cases])
    assert not codes.any()
    sealed, front = seal_and_verify(eng, got)
    assert sealed == whole and sorted(sealed) == sorted(fixture()[0]) and len(sealed) == 480
    assert len(front) == 480 and not front.any()


def test_capture_with_a_flipped_parity_byte(eng, ed):
    """one byte of a received parity region flipped: ERR_CORRUPT when more than d are received; with exactly d
    received the set is recovered, and the shred front then rejects it"""
    mask, _, whole = util.captured("mixed")[0]
    j = max(i for i in range(64) if not mask[i])
    assert j >= 32
    bad = list(whole)
    bad[j] = bad[j][:0x200] + bytes([bad[j][0x200] ^ 1]) + bad[j][0x201:]
    one_more = list(mask)
    one_more[mask.index(1)] = 0
    codes, got = eng.fec_recover_host([model.erase(bad, one_more), model.erase(bad, mask)], [one_more, mask])
    assert codes.tolist() == [ed.FEC_ERR_CORRUPT, 0] and got[0] == model.erase(bad, one_more)
    assert (0, got[1]) == model.fill(model.erase(bad, mask), mask)
    sealed, front = seal_and_verify(eng, [got[1]])
    assert sealed != list(whole) and (front == ed.SHRED_ERR_SIGNATURE).all() and len(front) == 64


def test_every_fixture_case(eng):
    """every case of the reference decoder's fixture, carried by real shreds, through _host and, packed back to
    back so slots fall on every byte alignment, through _dev"""
    cases = util.fixture_sets()
    sets, masks, want = [c[2] for c in cases], [c[1] for c in cases], [c[3] for c in cases]
    assert len(cases) == 644 and {w[0] for w in want} == {0, model.ERR_SET, model.ERR_PARTIAL, model.ERR_CORRUPT}
    for (kind, mask, st, w, ret, rec) in cases:
        no_code = all(mask[j] or st[j][0x40] & 0xF0 == 0x80 for j in range(len(st)))
        assert w[0] == (model.ERR_SET if no_code else model.REF_CODES[ret])
    check_host(eng, sets, masks, want)
    off = run_dev(eng, sets, masks, back_to_back, want)
    # received and erased, data and code slots all start at every alignment
    seen = {(o % 4, j < written_d(st, m) if any(x == 0 and s[0x40] & 0xF0 == 0x40 for s, x in zip(st, m)) else None, bool(m[j]))
            for (st, m), base in zip(zip(sets, masks), util.flat_npy(sets)) for j, o in enumerate(off[base:base + len(st)])}
    assert seen >= {(a, data, er) for a in range(4) for data in (True, False) for er in (True, False)}


def test_every_d(eng):
    """a received set of every d with the shredder's p, the extremes and the shallow sets: every depth 1..8"""
    splits, masks, received, _ = util.every_d()
    assert {fec_model.depth_of(d + p) for d, p in splits} == set(range(1, 9))
    want = check_host(eng, received, masks)
    assert not any(w[0] for w in want)
    run_dev(eng, received, masks, back_to_back, want)


def test_dev_spread_starts(eng):
    """device-resident input, slot i at byte i mod 16 of a 16-byte line: no byte outside rule 12's changes, rejected
    sets included"""
    rule = {c[0]: c for c in util.rule_cases()}
    picked = [rule[n] for n in ("good_3_of_6", "corrupt_last_byte", "recovered_slot", "all_but_one_erased_is_partial",
                                "erased_code_slot_too_short", "proof_byte_is_not_compared")]
    sets, masks = [c[2] for c in picked], [c[1] for c in picked]
    splits, m2, received, _ = util.every_d()
    for k in (0, 31, 66, 70, 72):      # 1 + 17, 32 + 32, 67 + 67, 67 + 67 again (the extreme), 2 + 3
        sets.append(received[k])
        masks.append(m2[k])
    for m, st, _ in util.captured("mixed")[5:]:
        sets.append(st)
        masks.append(m)
    want = expect(sets, masks)
    assert [w[0] for w in want][:6] == [0, model.ERR_CORRUPT, model.ERR_SET, model.ERR_PARTIAL, model.ERR_PARSE, 0]
    run_dev(eng, sets, masks, lambda i, end: end + (i - end) % 16 + (16 if i % 5 == 0 else 0), want)


def test_rule_cases_among_good_ones(eng):
    """every rule case has the model's code and its bytes unchanged, every neighbour is recovered"""
    rng = random.Random(263)
    sets, masks, codes = [], [], []
    for name, mask, st, code in util.rule_cases():
        cnt = rng.choice((3, 7, 64))
        d = rng.randrange(1, cnt)
        good = rs.fill(fec_util.make_set(rng, cnt, data_cnt=d))[1]
        gm = util.random_mask(rng, cnt, cnt - d)
        if all(gm[d:]):
            gm = gm[:-1] + (0,)
        sets += [st, tuple(model.erase(good, gm))]
        masks += [mask, gm]
        codes += [code, 0]
    for name, st, code in fec_util.bad_sets():
        sets.append(tuple(st))
        masks.append((0,) * len(st))
        codes.append(code)
    want = check_host(eng, sets, masks)
    assert [w[0] for w in want] == codes
    assert {0, model.ERR_PARSE, model.UNSUPPORTED, model.ERR_SET, model.ERR_PARTIAL, model.ERR_CORRUPT} == set(codes)
    run_dev(eng, sets, masks, back_to_back, want)


def test_set_first_that_is_no_prefix_sum(eng):
    """ranges that run backwards or leave [0, n): ERR_SET, nothing touched, the other sets recovered"""
    rng = random.Random(269)
    full = [rs.fill(fec_util.make_set(rng, c, data_cnt=d))[1] for c, d in ((3, 1), (5, 2), (2, 1))]
    ms = [(1, 0, 1), (0, 1, 1, 0, 1), (1, 0)]
    a, b, c = (model.erase(s, m) for s, m in zip(full, ms))
    flat, fm = a + b + c, [x for m in ms for x in m]      # n = 10
    first = [0, 3, 8, 3, 9, 11, 8, 10]     # a, b, backwards, (3..9: wrong depth), leaves n, backwards, c
    want_codes = [0, 0, model.ERR_SET, model.ERR_SET, model.ERR_SET, model.ERR_SET, 0]
    want_flat = [s for st, m in zip((a, b, c), ms) for s in model.fill(st, m)[1]]
    # what comes back is the full sets but for the proofs (the seal's) and the idx of a recovered code shred
    P = {3: rs.region(3), 5: rs.region(5), 2: rs.region(2)}
    for st, m, got in zip(full, ms, (model.fill(x, y)[1] for x, y in zip((a, b, c), ms))):
        for j, (w, g) in enumerate(zip(st, got)):
            at = 0x40 if w[0x40] & 0xF0 == 0x80 else 0x59
            assert g[at:at + P[len(st)]] == w[at:at + P[len(st)]] and (m[j] or g == w)
    assert want_flat != flat
    codes, got = eng.fec_recover_flat(flat, fm, first)
    assert codes.tolist() == want_codes and got == want_flat

    sets = [flat[first[k]:first[k + 1]] if want_codes[k] == 0 else [] for k in range(7)]
    masks = [fm[first[k]:first[k + 1]] if want_codes[k] == 0 else [] for k in range(7)]
    want = [model.fill(s, m) if want_codes[k] == 0 else (model.ERR_SET, []) for k, (s, m) in enumerate(zip(sets, masks))]
    run_dev(eng, sets, masks, back_to_back, want, set_first=first)


@pytest.mark.parametrize("n_set", [1, 2, 63, 64, 65, 255, 256, 257])
def test_set_counts(eng, n_set):
    """sets of 2+1 and 1+2 slots, one slot erased"""
    rng = random.Random(271 + n_set)
    sets, masks = [], []
    for k in range(n_set):
        d = 1 + (k + n_set) % 2
        st = rs.fill(fec_util.make_set(rng, 3, data_cnt=d))[1]
        m = tuple(int(j == k % 2) for j in range(3))       # slot 0 or 1: a code shred stays
        sets.append(model.erase(st, m))
        masks.append(m)
    want = check_host(eng, sets, masks)
    assert not any(w[0] for w in want)
    run_dev(eng, sets, masks, back_to_back, want)


def test_recover_seal_verify_on_one_stream(eng, ed):
    """fec_recover_dev, fec_seal_dev without keys and shreds_dev over the same device arrays, one synchronisation"""
    cases = util.captured("mixed")[4:]
    sets, masks = [st for _, st, _ in cases], [m for m, _, _ in cases]
    whole = [s for _, _, st in cases for s in st]
    flat = [s for st in sets for s in st]
    n, n_set = len(flat), len(sets)
    buf, off = bytearray(16), []
    for s in flat:
        off.append(len(buf))
        buf += s
    buf += bytes(64)
    d_buf = eng.alloc(len(buf)).upload(np.frombuffer(bytes(buf), np.uint8))
    d_off = eng.alloc(8 * n).upload(np.array(off, np.uint64))
    d_sz = eng.alloc(4 * n).upload(np.array([len(s) for s in flat], np.uint32))
    d_er = eng.alloc(n).upload(np.array([x for m in masks for x in m], np.uint8))
    d_first = eng.alloc(4 * (n_set + 1)).upload(util.flat_npy(sets).astype(np.uint32))
    d_keys = eng.alloc(32 * n).upload(np.frombuffer(bytes(fixture()[1]) * n, np.uint8))
    d_work, d_swork = eng.alloc(ed.fec_work_bytes(n, n_set)), eng.alloc(ed.shred_work_bytes(n))
    d_rout = eng.alloc(n_set).upload(np.full(n_set, 0x55, np.int8))
    d_sout = eng.alloc(n_set).upload(np.full(n_set, 0x55, np.int8))
    d_vout = eng.alloc(n).upload(np.full(n, 0x55, np.int8))
    eng.fec_recover_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, d_er.ptr, n_set, d_first.ptr, d_rout.ptr)
    eng.fec_seal_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, n_set, d_first.ptr, None, d_work.ptr, d_sout.ptr)
    eng.shreds_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, d_keys.ptr, d_swork.ptr, d_vout.ptr)
    eng.sync()
    got = d_buf.download(np.uint8, len(buf)).tobytes()
    rout, sout, vout = (b.download(np.int8, k).tolist() for b, k in ((d_rout, n_set), (d_sout, n_set), (d_vout, n)))
    for b in (d_buf, d_off, d_sz, d_er, d_first, d_keys, d_work, d_swork, d_rout, d_sout, d_vout):
        b.free()
    assert rout == [0] * n_set and sout == [0] * n_set and vout == [0] * n
    after = bytearray(buf)
    for o, s in zip(off, whole):
        after[o:o + len(s)] = s
    assert got == bytes(after)


def test_two_host_passes(eng):
    """more slots than one pass of fec_recover_host stages (16,384), the pass boundary inside the batch and not at
    a multiple of a set: the capture's sets repeated, half of each erased"""
    cases = util.captured("mixed")
    order = [6] + [k % 6 for k in range(300)]            # 96 + 300 x 64 = 19,296 slots
    assert sum(len(cases[b][1]) for b in order) == 19296 and (16384 - 96) % 64
    codes, got = eng.fec_recover_host([cases[b][1] for b in order], [cases[b][0] for b in order])
    assert not codes.any()
    want = [model.fill(st, m)[1] for m, st, _ in cases]
    assert all(got[k] == want[b] for k, b in enumerate(order))
