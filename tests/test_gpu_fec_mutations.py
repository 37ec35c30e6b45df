"""GPU: the seeded mutations of the FEC-set and proof-of-history fronts on
the device (the shred, packet, CRDS and transaction fronts run theirs there
already): the first 600 of fec_util.mutated_sets() through fec_seal_dev and
fec_parity_dev, recover_util.mutated(600) through fec_recover_dev, each packed
back to back in one guard buffer that is compared whole with the model's
bytes, and poh_util.mutated(400) through poh_blocks_host.  The code classes
the mutators must keep producing are counted by the models alone
(tests/fec_wave_util.py, checked without a device by
tests/test_fec_wave_cases.py)."""
import random

import numpy as np
import pytest

import fec_model
import fec_util
import fec_wave_util as wave
import recover_util
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


@pytest.mark.parametrize("with_keys", [False, True])
def test_seal_mutated_sets_on_the_device(eng, ed, oracle, with_keys):
    """without keys: proofs and roots of the sets the rules pass, every other byte as it was; with two leaders'
    keys: the signatures too, and every sealed shred back through the shred front"""
    sets = [list(s) for s in wave.mutated_sets()]
    privs = pubs = None
    if with_keys:
        rng = random.Random(389)
        two = [rng.randbytes(32) for _ in range(2)]
        privs = [two[k % 2] for k in range(len(sets))]
        pubs = [fec_model.public_key(oracle, p) for p in two] * (len(sets) // 2)
    want = fec_util.run_dev(eng, ed, oracle, sets, privs, pubs, fec_util.back_to_back)
    assert [w[0] for w in want] == list(wave.mutated_codes("seal"))


def test_parity_mutated_sets_on_the_device(eng):
    sets = [list(s) for s in wave.mutated_sets()]
    want = reedsol_util.expect(sets)
    assert [w[0] for w in want] == list(wave.mutated_codes("parity"))
    reedsol_util.run_dev(eng, sets, reedsol_util.back_to_back, want)


def test_recover_mutated_sets_on_the_device(eng):
    cases = recover_util.mutated(600)
    want = [c[2] for c in cases]
    assert [w[0] for w in want] == list(wave.mutated_codes("recover"))
    recover_util.run_dev(eng, [c[1] for c in cases], [c[0] for c in cases], recover_util.back_to_back, want)


def test_poh_mutated_blocks(eng):
    """hash_cnt_max 4,096: a mutated hash count above it is UNSUPPORTED and no chain runs long"""
    blocks, ins, codes, bad, last = wave.mutated_blocks(4096)
    got_codes, got_bad, got_last = eng.poh_blocks_host(list(blocks), list(ins), hash_cnt_max=4096)
    differ = np.nonzero(got_codes != np.array(codes, np.int8))[0]
    assert not len(differ), (differ[:8].tolist(), got_codes[differ[:8]].tolist())
    assert got_bad.tolist() == list(bad)
    assert [x.tobytes() for x in got_last] == list(last)
