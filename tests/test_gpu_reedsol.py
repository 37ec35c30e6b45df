"""GPU: the Reed-Solomon parity of a leader's FEC sets
(fd_ed25519_hip_fec_parity_host / _dev, include/fd_ed25519_hip.h Part 2g)
against the test-side model (reedsol_model: log and exp tables, the Lagrange
product) and, with the seal behind it (Part 2f), against the reference's
captured shreds.  A small engine: compact tables, 512-signature chunks."""
import random

import numpy as np
import pytest

import fec_model
import fec_util
import reedsol_model as rs
import reedsol_util as util
from reedsol_util import back_to_back, expect, run_dev
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


def check_host(eng, sets, want=None):
    want = expect(sets) if want is None else want
    codes, got = eng.fec_parity_host([list(s) for s in sets])
    assert codes.tolist() == [w[0] for w in want]
    for k, w in enumerate(want):
        assert [bytes(s) for s in got[k]] == list(w[1]), k
    return want


def test_capture_end_to_end(eng):
    """the capture's parity regions, signatures and proofs blanked: parity,
    then seal with the capture's key -- the reference's own 480 shreds, byte
    for byte, from data shreds and headers alone"""
    sets = fec_util.captured_sets()
    assert [len(s) for s in sets] == [64] * 6 + [96]
    blanked = [rs.blank_parity(fec_util.blank(s)) for s in sets]
    assert all(b[:64] == bytes(64) for s in blanked for b in s)
    assert sum(b[0x59:0x59 + 979] == bytes(979) for s in blanked for b in s) == 240
    codes, filled = eng.fec_parity_host(blanked)
    assert not codes.any()
    codes, got, roots, sigs = eng.fec_seal_host(filled, fec_util.private_key())
    assert not codes.any()
    sealed = [bytes(s) for st in got for s in st]
    assert sealed == [s for st in sets for s in st]
    assert sorted(sealed) == sorted(fixture()[0]) and len(sealed) == 480
    front, _ = eng.shreds_host(sealed, fixture()[1])
    assert len(front) == 480 and not front.any()


def test_every_d(eng):
    """one set of every d with the shredder's p, the extremes and the shallow
    sets -- every depth 1..8 and so every P -- through _host and, packed back
    to back so shreds fall on every byte alignment, through _dev"""
    splits, sets, filled = util.every_d()
    assert [d for d, _ in splits[:67]] == list(range(1, 68)) and splits[67:71] == util.EXTREMES
    assert {fec_model.depth_of(d + p) for d, p in splits} == set(range(1, 9))
    want = [(0, w) for w in filled]
    check_host(eng, sets, want)
    off = run_dev(eng, sets, back_to_back, want)
    # data and code shreds both start at every alignment
    flat = [s for st in sets for s in st]
    assert {(o % 4, s[0x40] & 0xF0) for o, s in zip(off, flat)} == {(a, t) for a in range(4) for t in (0x80, 0x40)}


def test_dev_spread_starts(eng):
    """device-resident input, shred i at byte i mod 16 of a 16-byte line"""
    rng = random.Random(167)
    sets = [fec_util.make_set(rng, cnt, data_cnt=d) for cnt, d in ((5, 2), (33, 16), (64, 32), (3, 1), (16, 9))]
    sets.append(rs.blank_parity(list(fec_util.captured_sets()[6])))
    want = expect(sets)
    assert not any(w[0] for w in want) and want[-1][1] == list(fec_util.captured_sets()[6])
    run_dev(eng, sets, lambda i, end: end + (i - end) % 16 + (16 if i % 5 == 0 else 0), want)


def test_rejected_sets_among_good_ones(eng):
    """every old and new rule case has the model's code and its bytes
    unchanged, every neighbour is encoded"""
    rng = random.Random(173)
    bad = util.all_bad_sets()
    assert {w for _, _, w in bad} == {fec_model.ERR_PARSE, fec_model.UNSUPPORTED, fec_model.ERR_SET}
    assert {"cnt_0", "cnt_135", "swapped_data", "variant_0x93", "truncated_data", "data_only", "code_only",
            "data_cnt_minus_one_same_place", "code_cnt_plus_one", "code_between_data", "data_68_code_1",
            "parse_then_data_cnt"} <= {n for n, _, _ in bad}
    sets = [fec_util.make_set(rng, 4)]
    for _, s, _ in bad:
        cnt = rng.choice((2, 3, 7, 64))
        sets += [s, fec_util.make_set(rng, cnt, data_cnt=rng.randrange(1, cnt))]
    want = check_host(eng, sets)
    assert [w[0] for w in want] == [0] + [c for _, _, w in bad for c in (w, 0)]
    assert all(w[1] == [bytes(x) for x in s] for w, s in zip(want, sets) if w[0])
    run_dev(eng, sets, back_to_back, want)


def test_set_first_that_is_no_prefix_sum(eng):
    """ranges that run backwards or leave [0, n): ERR_SET, nothing touched,
    the other sets encoded"""
    rng = random.Random(179)
    a, b, c = fec_util.make_set(rng, 3), fec_util.make_set(rng, 5), fec_util.make_set(rng, 2)
    flat = a + b + c                       # n = 10
    first = [0, 3, 8, 3, 9, 11, 8, 10]     # a, b, backwards, (3..9: wrong depth), leaves n, backwards, c
    want_codes = [0, 0, fec_model.ERR_SET, fec_model.ERR_SET, fec_model.ERR_SET, fec_model.ERR_SET, 0]
    want_flat = [s for st in (a, b, c) for s in rs.fill(st)[1]]
    assert want_flat != flat
    codes, got = eng.fec_parity_flat(flat, first)
    assert codes.tolist() == want_codes and got == want_flat

    # device-resident: the same set_first against the same three sets
    sets = [flat[first[k]:first[k + 1]] if want_codes[k] == 0 else [] for k in range(7)]
    want = [(0, rs.fill(s)[1]) if want_codes[k] == 0 else (fec_model.ERR_SET, []) for k, s in enumerate(sets)]
    run_dev(eng, sets, back_to_back, want, set_first=first)


@pytest.mark.parametrize("n_set", [1, 2, 63, 64, 65, 255, 256, 257])
def test_set_counts(eng, n_set):
    """sets of 2+1 and 1+2 shreds"""
    rng = random.Random(181 + n_set)
    sets = [fec_util.make_set(rng, 3, data_cnt=1 + (k + n_set) % 2) for k in range(n_set)]
    want = check_host(eng, sets)
    assert not any(w[0] for w in want)


def test_parity_then_seal_on_one_stream(eng, ed, oracle):
    """fec_parity_dev, then fec_seal_dev over the same device arrays with no
    synchronisation between them"""
    rng = random.Random(191)
    sets = [fec_util.make_set(rng, cnt, data_cnt=d) for cnt, d in ((64, 32), (3, 2), (40, 8), (134, 67))]
    sets.insert(2, list(util.rule_cases()[4][1]))   # code_cnt_plus_one: the parity rejects it, the seal takes it
    privs = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in sets]
    filled = expect(sets)
    assert [w[0] for w in filled] == [0, 0, fec_model.ERR_SET, 0, 0]
    sealed = [fec_model.seal(oracle, w[1], privs[k]) for k, w in enumerate(filled)]
    assert not any(w[0] for w in sealed)
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
    d_first = eng.alloc(4 * (n_set + 1)).upload(np.cumsum([0] + [len(s) for s in sets]).astype(np.uint32))
    d_privs = eng.alloc(32 * n_set).upload(np.frombuffer(b"".join(privs), np.uint8))
    d_work = eng.alloc(ed.fec_work_bytes(n, n_set))
    d_pout = eng.alloc(n_set).upload(np.full(n_set, 0x55, np.int8))
    d_sout = eng.alloc(n_set).upload(np.full(n_set, 0x55, np.int8))
    eng.fec_parity_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, n_set, d_first.ptr, d_pout.ptr)
    eng.fec_seal_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, n_set, d_first.ptr, d_privs.ptr, d_work.ptr, d_sout.ptr)
    eng.sync()
    got = d_buf.download(np.uint8, len(buf)).tobytes()
    pout, sout = d_pout.download(np.int8, n_set).tolist(), d_sout.download(np.int8, n_set).tolist()
    for b in (d_buf, d_off, d_sz, d_first, d_privs, d_work, d_pout, d_sout):
        b.free()
    assert pout == [w[0] for w in filled] and sout == [0] * n_set
    after = bytearray(buf)
    for o, s in zip(off, (s for w in sealed for s in w[1])):
        after[o:o + len(s)] = s
    assert got == bytes(after)


def test_two_host_passes(eng):
    """more shreds than one pass of fec_parity_host stages (16,384), the pass
    boundary inside the batch and not at a multiple of a set: the capture's
    sets repeated"""
    base = [list(s) for s in fec_util.captured_sets()]
    blanked = [rs.blank_parity(s) for s in base]
    order = [6] + [k % 6 for k in range(300)]            # 96 + 300 x 64 = 19,296 shreds
    assert sum(len(base[b]) for b in order) == 19296 and (16384 - 96) % 64
    codes, got = eng.fec_parity_host([blanked[b] for b in order])
    assert not codes.any()
    assert all(got[k] == base[b] for k, b in enumerate(order))
