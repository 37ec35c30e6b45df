"""GPU: one flipped bit per set through the compare phase of the recover
kernel (fd_ed25519_recover.hip's rc_rows<false>): ERR_CORRUPT comes from a
per-lane difference that any of 256 lanes ORs into an LDS flag, over passes of
32 compared rows, groups of eight rows and passes of 256 columns, with a mask
on the three-byte last column.  The flips of tests/fec_wave_util.py sit in
every wave of columns, in every row pass, at the edges of the groups of eight
and in the second column pass; its geometry and the model's codes are checked
without a device by tests/test_fec_wave_cases.py.  Every set keeps its bytes
but the recovered ones: the whole guard buffer is compared."""
import pytest

import fec_wave_util as wave
import recover_util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from firedancer_amd import ed25519
    e = ed25519.Engine(0, max_chunk=512, compact=True)
    yield e
    e.close()


def check_host(eng, sets, masks, want):
    codes, got = eng.fec_recover_host([list(s) for s in sets], masks)
    assert codes.tolist() == [w[0] for w in want]
    assert all([bytes(s) for s in got[k]] == list(w[1]) for k, w in enumerate(want))


def test_compared_rows_and_columns(eng):
    """2 + 67, nothing erased: 90 sets with a flip in a compared row, ERR_CORRUPT; three with a flip in the first
    proof byte, 0"""
    grid = wave.sweep_grid()
    sets, masks = [c[4] for c in grid], [c[3] for c in grid]
    want = [(c[5], list(c[4])) for c in grid]        # nothing erased: no byte changes (fec_wave_util asserts the model's)
    assert [w[0] for w in want] == [wave.CORRUPT] * 90 + [0] * 3
    recover_util.run_dev(eng, sets, masks, recover_util.back_to_back, want)
    pick = list(range(0, 93, 7)) + [90, 92]
    check_host(eng, [sets[k] for k in pick], [masks[k] for k in pick], [want[k] for k in pick])


def test_shared_group_second_column_pass_and_basis(eng):
    """erased rows in the last compared group of eight, columns 256..264, and a flip in a basis slot per wave of
    columns; the unflipped sets are recovered"""
    rest = wave.sweep_rest()
    sets, masks = [c[2] for c in rest], [c[1] for c in rest]
    want = recover_util.expect(sets, masks)
    assert [w[0] for w in want] == [c[3] for c in rest] and sum(c[3] == wave.CORRUPT for c in rest) == 16
    recover_util.run_dev(eng, sets, masks, recover_util.back_to_back, want)
    pick = [0, 1, 2, 3, 4, 5, 14, 15, 18]
    check_host(eng, [sets[k] for k in pick], [masks[k] for k in pick], [want[k] for k in pick])
