"""GPU: the workgroup reductions of the FEC-set kernels across waves.  "The
first failing slot decides" is an LDS atomicMin over up to 134 lanes in three
waves (fd_ed25519_fec.hip, fd_ed25519_reedsol.hip, fd_ed25519_recover.hip),
and the recover kernel reduces its first received code shred and its first
received slot the same way; the CPU build of the shared rules has none of it.
Sets of 134 and 65 slots with two failing slots of different codes in
different waves (tests/fec_wave_util.py, whose conditions
tests/test_fec_wave_cases.py checks without a device), each between two good
sets in one launch, in a guard buffer packed back to back: the codes and every
byte of the buffer are the model's.  A small engine: compact tables,
512-signature chunks."""
import random

import pytest

import fec_model
import fec_util
import fec_wave_util as wave
import recover_model
import recover_util
import reedsol_model as rs
import reedsol_util

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


def test_seal_first_failing_slot_across_waves(eng, ed, oracle):
    """every broken set keeps its bytes and has the lower slot's code; every neighbour is sealed under its key"""
    rng = random.Random(373)
    cases = wave.order_sets("seal")
    sets = wave.between_good(rng, [list(st) for _, _, st, _ in cases], lambda: fec_util.make_set(rng, rng.choice((3, 7, 64))))
    privs = [rng.randbytes(32) for _ in sets]
    pubs = [fec_model.public_key(oracle, p) for p in privs]
    want = fec_util.run_dev(eng, ed, oracle, sets, privs, pubs, fec_util.back_to_back)
    assert [w[0] for w in want] == [0] + [c for _, _, _, code in cases for c in (code, 0)]


def test_parity_first_failing_slot_across_waves(eng):
    rng = random.Random(379)
    cases = wave.order_sets("parity")

    def good():
        cnt = rng.choice((3, 7, 64))
        return fec_util.make_set(rng, cnt, data_cnt=rng.randrange(1, cnt))

    sets = wave.between_good(rng, [list(st) for _, _, st, _ in cases], good)
    want = reedsol_util.expect(sets)
    assert [w[0] for w in want] == [0] + [c for _, _, _, code in cases for c in (code, 0)]
    assert all(w[1] == [bytes(x) for x in s] for w, s in zip(want, sets) if w[0])
    reedsol_util.run_dev(eng, sets, reedsol_util.back_to_back, want)


def good_received(rng):
    cnt = rng.choice((3, 7, 64))
    d = rng.randrange(1, cnt)
    full = rs.fill(fec_util.make_set(rng, cnt, data_cnt=d))[1]
    m = recover_util.random_mask(rng, cnt, cnt - d)
    if all(m[d:]):
        m = m[:-1] + (0,)
    return tuple(recover_model.erase(full, m)), m


def test_recover_first_failing_slot_across_waves_and_stages(eng):
    """the seal's pairs, and a failure of the first stage of the judge against one of the second in both orders"""
    rng = random.Random(383)
    cases = wave.recover_order_sets()
    sets, masks, codes = [], [], []
    for lo, hi, _, _, mask, st, code in cases:
        g, gm = good_received(rng)
        sets += [g, st]
        masks += [gm, mask]
        codes += [0, code]
    g, gm = good_received(rng)
    sets.append(g); masks.append(gm); codes.append(0)
    want = recover_util.expect(sets, masks)
    assert [w[0] for w in want] == codes
    recover_util.run_dev(eng, sets, masks, recover_util.back_to_back, want)
    pick = list(range(0, len(sets), 5))
    codes_h, got = eng.fec_recover_host([list(sets[k]) for k in pick], [masks[k] for k in pick])
    assert codes_h.tolist() == [codes[k] for k in pick]
    assert all([bytes(s) for s in got[i]] == list(want[k][1]) for i, k in enumerate(pick))


def test_recover_first_code_shred_and_first_received_slot_beyond_wave_0(eng):
    """the first received code shred in wave 2, that shred failing a set rule, the first received slot (the
    signature's source) in wave 1, and recovered code shreds whose idx wraps below zero"""
    cases = wave.recover_reductions()
    assert [c[0] for c in cases] == ["code_shreds_from_128", "first_code_shred_fails_a_set_rule", "all_data_erased",
                                     "code_idx_wraps_below_zero"]
    sets, masks, want = [c[2] for c in cases], [c[1] for c in cases], [c[3] for c in cases]
    assert [w[0] for w in want] == [0, wave.SET, 0, 0]
    recover_util.run_dev(eng, sets, masks, recover_util.back_to_back, want)
    codes, got = eng.fec_recover_host([list(s) for s in sets], masks)
    assert codes.tolist() == [w[0] for w in want]
    assert all([bytes(s) for s in got[k]] == list(w[1]) for k, w in enumerate(want))
