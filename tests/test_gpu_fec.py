"""GPU: sealing a leader's FEC sets (fd_ed25519_hip_fec_seal_host / _dev,
include/fd_ed25519_hip.h Part 2f) against the test-side model of the
shredder's tree (fec_model: hashlib and the CPU oracle's sign), and every
sealed shred back through the shred front (Part 2c).  A small engine:
compact tables, 512-signature chunks."""
import random

import numpy as np
import pytest

import fec_model as model
import fec_util as util
from fec_util import back_to_back, check_front, check_outputs, expect, run_dev
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
def keys(oracle):
    """two leaders: (private, public)"""
    rng = random.Random(73)
    privs = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(2)]
    return [(p, model.public_key(oracle, p)) for p in privs]


def check_host(eng, oracle, sets, privs, pubs):
    want = expect(oracle, sets, privs)
    codes, got, roots, sigs = eng.fec_seal_host(sets, privs)
    check_outputs(want, codes, roots, sigs)
    for k, w in enumerate(want):
        assert [bytes(s) for s in got[k]] == w[1], k
    if privs is not None:
        check_front(eng, want, pubs)
    return want


def test_capture_round_trip(eng, oracle):
    """blank the capture's signatures and proofs, seal with the capture's
    key: the reference's own 480 shreds, byte for byte"""
    sets = util.captured_sets()
    assert [len(s) for s in sets] == [64] * 6 + [96]
    blanked = [util.blank(s) for s in sets]
    assert all(b[:64] == bytes(64) for s in blanked for b in s)
    codes, got, roots, sigs = eng.fec_seal_host(blanked, util.private_key())
    assert not codes.any()
    sealed = [bytes(s) for st in got for s in st]
    assert sealed == [s for st in sets for s in st]
    assert sorted(sealed) == sorted(fixture()[0]) and len(sealed) == 480
    assert all(sigs[k].tobytes() == sets[k][0][:64] for k in range(7))
    front, _ = eng.shreds_host(sealed, fixture()[1])
    assert len(front) == 480 and not front.any()


def test_shapes(eng, ed, oracle, keys):
    """one set of every leaf count, two leaders, through _host and, packed
    back to back so shreds fall on every byte alignment, through _dev"""
    sets = util.shape_sets()
    assert [len(s) for s in sets] == list(util.SHAPES)
    privs, pubs = [keys[k % 2][0] for k in range(len(sets))], [keys[k % 2][1] for k in range(len(sets))]
    want = check_host(eng, oracle, sets, privs, pubs)
    assert not any(w[0] for w in want)
    starts, end = set(), 16
    for s in (s for st in sets for s in st):
        starts.add(end % 4)
        end += len(s)
    assert starts == {0, 1, 2, 3}
    run_dev(eng, ed, oracle, sets, privs, pubs, back_to_back)


def test_dev_spread_starts(eng, ed, oracle, keys):
    """device-resident input, shred i at byte i mod 16 of a 16-byte line"""
    rng = random.Random(83)
    sets = [util.make_set(rng, cnt) for cnt in (5, 33, 64, 3, 16)] + [util.blank(util.captured_sets()[6])]
    privs = [keys[k % 2][0] for k in range(len(sets))]
    privs[-1] = util.private_key()
    pubs = [model.public_key(oracle, p) for p in privs]
    run_dev(eng, ed, oracle, sets, privs, pubs, lambda i, end: end + (i - end) % 16 + (16 if i % 5 == 0 else 0))


@pytest.mark.parametrize("n_set", [1, 2, 63, 64, 65, 255, 256, 257])
def test_set_counts(eng, oracle, keys, n_set):
    """around the sign and scatter kernels' 256-lane blocks"""
    rng = random.Random(89 + n_set)
    sets = [util.make_set(rng, 2 + (k + n_set) % 2) for k in range(n_set)]
    privs, pubs = [keys[k % 2][0] for k in range(n_set)], [keys[k % 2][1] for k in range(n_set)]
    check_host(eng, oracle, sets, privs, pubs)


def test_rejected_sets_among_good_ones(eng, ed, oracle, keys):
    """every bad set has the model's code and its bytes unchanged, every
    neighbour is sealed"""
    rng = random.Random(97)
    bad = util.bad_sets()
    assert {w for _, _, w in bad} == {model.ERR_PARSE, model.UNSUPPORTED, model.ERR_SET}
    assert {"cnt_0", "cnt_135", "depth_nibble_low", "swapped_data", "duplicate_index", "variant_0x93",
            "truncated_data"} <= {n for n, _, _ in bad}
    sets = [util.make_set(rng, 4)]
    for _, s, _ in bad:
        sets += [s, util.make_set(rng, rng.choice((2, 3, 7, 64)))]
    privs, pubs = [keys[k % 2][0] for k in range(len(sets))], [keys[k % 2][1] for k in range(len(sets))]
    want = check_host(eng, oracle, sets, privs, pubs)
    assert [w[0] for w in want] == [0] + [c for _, _, w in bad for c in (w, 0)]
    run_dev(eng, ed, oracle, sets, privs, pubs, back_to_back)


def test_set_first_that_is_no_prefix_sum(eng, ed, oracle, keys):
    """ranges that run backwards or leave [0, n): ERR_SET, nothing touched,
    the other sets sealed"""
    rng = random.Random(101)
    a, b, c = util.make_set(rng, 3), util.make_set(rng, 5), util.make_set(rng, 2)
    flat = a + b + c                       # n = 10
    first = [0, 3, 8, 3, 9, 11, 8, 10]     # a, b, backwards, (3..9: wrong depth), leaves n, backwards, c
    ranges = list(zip(first[:-1], first[1:]))
    privs = [keys[k % 2][0] for k in range(len(ranges))]
    codes, got, roots, sigs = eng.fec_seal_flat(flat, first, privs)
    assert codes.tolist() == [0, 0, model.ERR_SET, model.ERR_SET, model.ERR_SET, model.ERR_SET, 0]
    want = [model.seal(oracle, s, privs[k]) for k, s in ((0, a), (1, b), (6, c))]
    assert got == [s for w in want for s in w[1]]
    assert [roots[k].tobytes() for k in (0, 1, 6)] == [w[2] for w in want] and not roots[2:6].any() and not sigs[2:6].any()

    # device-resident: the same set_first against the same three sets
    want = run_dev_with_first(eng, ed, oracle, flat, first, privs)
    assert want == [0, 0, model.ERR_SET, model.ERR_SET, model.ERR_SET, model.ERR_SET, 0]


def run_dev_with_first(eng, ed, oracle, flat, first, privs):
    """_dev with a caller-made set_first; returns the codes after checking
    that the shreds of no rejected range changed and the rest match the model"""
    n, n_set = len(flat), len(first) - 1
    buf = bytearray(16)
    off = []
    for s in flat:
        off.append(len(buf))
        buf += s
    buf += bytes(64)
    d_buf = eng.alloc(len(buf)).upload(np.frombuffer(bytes(buf), np.uint8))
    d_off = eng.alloc(8 * n).upload(np.array(off, np.uint64))
    d_sz = eng.alloc(4 * n).upload(np.array([len(s) for s in flat], np.uint32))
    d_first = eng.alloc(4 * (n_set + 1)).upload(np.array(first, np.uint32))
    d_privs = eng.alloc(32 * n_set).upload(np.frombuffer(b"".join(privs), np.uint8))
    d_work = eng.alloc(ed.fec_work_bytes(n, n_set))
    d_out = eng.alloc(n_set).upload(np.full(n_set, 0x55, np.int8))
    eng.fec_seal_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, n_set, d_first.ptr, d_privs.ptr, d_work.ptr, d_out.ptr)
    eng.sync()
    got, out = d_buf.download(np.uint8, len(buf)).tobytes(), d_out.download(np.int8, n_set).tolist()
    for b in (d_buf, d_off, d_sz, d_first, d_privs, d_work, d_out):
        b.free()
    after = bytearray(buf)
    for k in range(n_set):
        if out[k] == 0:
            _, sealed, _, _ = model.seal(oracle, flat[first[k]:first[k + 1]], privs[k])
            for i, s in zip(range(first[k], first[k + 1]), sealed):
                after[off[i]:off[i] + len(s)] = s
    assert got == bytes(after)
    return out


def test_without_keys(eng, ed, oracle, keys):
    """privs None: proofs and roots, bytes [0, 64) of every shred as they were"""
    rng = random.Random(103)
    sets = [util.make_set(rng, cnt) for cnt in (1, 6, 64, 65)] + [util.bad_sets()[3][1]]
    want = check_host(eng, oracle, sets, None, None)
    assert [w[0] for w in want] == [0, 0, 0, 0, model.ERR_SET]
    assert all(w[1][j][:64] == s[j][:64] for w, s in zip(want, sets) for j in range(len(s)))
    run_dev(eng, ed, oracle, sets, None, None, back_to_back)


def test_two_host_passes(eng, oracle, keys):
    """more shreds than one pass of fec_seal_host stages (16,384), the pass
    boundary inside the batch and not at a multiple of a set: the capture's
    sets repeated under two keys"""
    base = [util.blank(s) for s in util.captured_sets()]
    order = [6] + [k % 6 for k in range(300)]            # 96 + 300 x 64 = 19,296 shreds
    privs = [keys[k % 2][0] for k in range(len(order))]
    pubs = [keys[k % 2][1] for k in range(len(order))]
    once = {}
    for k, b in enumerate(order):
        if (b, k % 2) not in once:
            once[(b, k % 2)] = model.seal(oracle, base[b], privs[k])
    want = [once[(b, k % 2)] for k, b in enumerate(order)]
    assert sum(len(w[1]) for w in want) == 19296 and (16384 - 96) % 64
    codes, got, roots, sigs = eng.fec_seal_host([base[b] for b in order], privs)
    check_outputs(want, codes, roots, sigs)
    assert all(got[k] == want[k][1] for k in range(len(order)))
    check_front(eng, want, pubs)
