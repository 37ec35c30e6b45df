"""The conditions under which the cases of tests/fec_wave_util.py mean what
they say, checked without a device: every builder asserts its own conditions
where it builds (the model's codes, the coverage of the listed slots, rows and
bytes, the geometry of the sets, the code counts of the seeded mutations, the
255 coefficient values); this module runs the builders and states the counts
the GPU modules rely on."""
import pytest

import fec_wave_util as wave
import recover_model


@pytest.mark.parametrize("front", ["seal", "parity"])
def test_rule_order_sets(front):
    """16 sets: six pairs in a set of 134 and two in a set of 65, both assignments; the set's code is the lower
    slot's own, the two codes differ, and each code wins and loses somewhere"""
    cases = wave.order_sets(front)
    assert len(cases) == 16 and {len(st) for _, _, st, _ in cases} == {134, 65}
    assert all(lo < hi < len(st) for lo, hi, st, _ in cases)
    assert {(lo // 64, hi // 64) for lo, hi, _, _ in cases} == {(0, 1), (0, 2), (1, 2)}


def test_recover_rule_order_sets():
    """the same pairs on received sets, and two stage mixes a pair"""
    cases = wave.recover_order_sets()
    assert len(cases) == 32
    mixes = [c for c in cases if (c[2], c[3]) != ("one", "one")]
    assert len(mixes) == 16 and sum(c[2] == "one" for c in mixes) == 8
    assert {c[3] for c in mixes if c[2] == "one"} | {c[2] for c in mixes if c[3] == "one"} == {"short", "data_behind_d", "code_cnt_off"}


def test_recover_reductions():
    """what the model says of the three reduction cases and of the wrap"""
    cases = {name: (mask, st, want) for name, mask, st, want in wave.recover_reductions()}
    assert cases["code_shreds_from_128"][2][0] == 0 and cases["all_data_erased"][2][0] == 0
    assert cases["first_code_shred_fails_a_set_rule"][2][0] == wave.SET
    # the rules pass a set whose recovered code shreds' idx wraps: the case is in
    assert cases["code_idx_wraps_below_zero"][2][0] == 0


def test_sweep():
    """the model's codes, the (row, byte) coverage and the geometry of the corruption sweep"""
    grid, rest = wave.sweep_grid(), wave.sweep_rest()
    assert [c[5] for c in grid] == [wave.CORRUPT] * 90 + [0] * 3
    codes = {name: code for name, _, _, code in rest}
    assert [n for n, c in codes.items() if c == 0] == ["group_unflipped", "col2_unflipped", "col2_row_3_proof_byte"]
    assert len(rest) == 3 + 12 + 4 and set(codes.values()) == {0, recover_model.ERR_CORRUPT}


@pytest.mark.parametrize("front", ["seal", "parity", "recover"])
def test_mutation_counts(front):
    """every code class of the first 600 seeded mutations, by the model alone"""
    assert wave.count(list(wave.mutated_codes(front))) == wave.MUTATION_COUNTS[front]


def test_mutated_blocks():
    blocks, ins, codes, bad, last = wave.mutated_blocks()
    assert len(blocks) == 400 and {0, -16, -25} <= set(codes)


def test_gf256_cases():
    c, x, want = wave.product_rows()
    assert len(c) == 65536 and int(want[256 + 1]) & 0xFF == 1 and not want[:256].any()
    assert len(wave.coef_cases()) == 50
