"""fd_ed25519_hip_fec_parity (fd_reedsol_core.h on the host: the rules and the
code the device's parity kernel runs) against the test-side model
(reedsol_model: log and exp tables, the Lagrange product) and against the
reference encoder's own output (tests/golden/reedsol.npz, and the parity
shreds of the captured FEC sets).  No GPU."""
import pytest

import fec_model
import fec_util
import reedsol_model as rs
import reedsol_util as util


@pytest.fixture(scope="module")
def ed():
    from firedancer_amd import ed25519
    return ed25519


def test_field():
    assert rs.EXP[:9] == [1, 2, 4, 8, 16, 32, 64, 128, 0x1D] and sorted(rs.EXP[:255]) == list(range(1, 256))
    assert all(rs.mul(a, rs.inv(a)) == 1 for a in range(1, 256))
    assert rs.mul(0x80, 2) == 0x1D and rs.mul(7, 0) == 0


def test_model_reproduces_the_reference_for_every_d():
    g = util.golden()
    assert g["data"].shape == (67, 32) and g["parity"].shape == (67, 67, 32) and int(g["cases"]) == 402
    assert [util.shredder_p(d) for d in (1, 2, 31, 32, 33, 67)] == [17, 18, 32, 32, 33, 67]
    data = [g["data"][i].tobytes() for i in range(67)]
    for d in range(1, 68):
        assert rs.encode(data[:d], 67) == [g["parity"][d - 1][j].tobytes() for j in range(67)], d


def test_rows_do_not_depend_on_p():
    """M_d's row j is the same in every (d, p): the parity of (d, p) is the first p rows of (d, 67)"""
    for d in (1, 2, 32, 33, 67):
        assert len(rs.row(d, 66)) == d and all(rs.row(d, j) for j in range(67))
    # one data shred: every parity shred repeats it
    assert all(rs.row(1, j) == (1,) for j in range(67))


def test_library_against_the_fixture(ed):
    """the library's encoder on sets whose data shreds carry the fixture's
    bytes behind their headers, 0x20 into the protected region: the reference's parity there"""
    g = util.golden()
    splits, sets, _ = util.every_d()
    for (d, p), st in zip(splits, sets):
        st = [bytes(s[:0x60]) + g["data"][i].tobytes() + bytes(s[0x80:]) if i < d else s for i, s in enumerate(st)]
        code, got = ed.fec_parity(st)
        assert code == 0
        for j in range(p):
            assert got[d + j][0x79:0x79 + 32] == g["parity"][d - 1][j].tobytes(), (d, j)


def test_library_against_the_model_for_every_d(ed):
    splits, sets, want = util.every_d()
    assert len(sets) == 74 and splits[67:71] == util.EXTREMES
    assert {fec_model.depth_of(d + p) for d, p in splits} == set(range(1, 9))
    for (d, p), st, w in zip(splits, sets, want):
        code, got = ed.fec_parity(list(st))
        assert code == 0 and got == list(w), (d, p)
        # exactly the parity regions changed
        P = ed.fec_parity_region(d + p)
        assert P == rs.region(d + p) and P % 4 == 3
        assert all(a == b for a, b in zip(got[:d], st[:d]))
        assert all(a[:0x59] == b[:0x59] and a[0x59 + P:] == b[0x59 + P:] and len(a) == 1228 for a, b in zip(got[d:], st[d:]))


def test_captured_sets_reproduce_the_capture(ed):
    """the parity regions of the 7 captured sets blanked and refilled: the
    reference's own 240 code shreds, byte for byte"""
    sets = fec_util.captured_sets()
    refilled = 0
    for st in sets:
        st = list(st)
        d = sum(s[0x40] & 0xF0 == 0x80 for s in st)
        assert (len(st), d) in ((64, 32), (96, 48)) and rs.region(len(st)) == (1019 if d == 32 else 999)
        blanked = rs.blank_parity(st)
        assert blanked != st and blanked[:d] == st[:d]
        assert ed.fec_parity(blanked) == (0, st) and rs.fill(blanked) == (0, st)
        refilled += len(st) - d
    assert refilled == 240


def test_old_rules_keep_their_codes(ed):
    for name, st, want in fec_util.bad_sets():
        assert rs.parity_code(st) == want, name
        assert ed.fec_parity(st) == (want, [bytes(s) for s in st]), name


def test_new_rules(ed):
    cases = util.rule_cases()
    names = {n for n, _, _, _ in cases}
    assert {"data_only", "code_only", "data_cnt_plus_one", "data_cnt_minus_one_same_place", "code_cnt_plus_one",
            "code_cnt_minus_one", "code_between_data", "data_68_code_1"} <= names
    # the cases that only the parity's own rules reject
    assert sum(seal_passes for _, _, _, seal_passes in cases) >= 5
    for name, st, want, _ in cases:
        assert want != 0
        assert ed.fec_parity(list(st)) == (want, list(st)), name


def test_priority(ed):
    """an earlier shred's parse error wins over a later data_cnt mismatch, and the other way round"""
    by_name = {n: (list(s), w) for n, s, w, _ in util.rule_cases()}
    assert by_name["parse_then_data_cnt"][1] == fec_model.ERR_PARSE
    assert by_name["code_cnt_then_parse"][1] == fec_model.ERR_SET
    assert by_name["unsupported_then_code_cnt"][1] == fec_model.UNSUPPORTED
    for name in ("parse_then_data_cnt", "code_cnt_then_parse", "code_cnt_then_unsupported", "unsupported_then_code_cnt"):
        st, want = by_name[name]
        assert ed.fec_parity(st) == (want, st), name


def test_mutated_sets(ed):
    seen = set()
    for st in fec_util.mutated_sets()[:400]:
        want = rs.fill(list(st))
        assert ed.fec_parity(list(st)) == want
        seen.add(want[0])
    assert seen == {0, fec_model.ERR_PARSE, fec_model.UNSUPPORTED, fec_model.ERR_SET}


def test_python_mirror(ed):
    assert [ed.fec_parity_region(c) for c in (2, 3, 64, 96, 134)] == [1119, 1099, 1019, 999, 979]
    assert ed.fec_parity([]) == (ed.FEC_ERR_SET, [])
    from firedancer_amd import tile
    assert tile.ABI_VERSION == 16
