"""fd_ed25519_hip_fec_recover (fd_reedsol_core.h's rules 9-12 on the host: the
rules and the code the device's recover kernel runs) against the test-side
model (recover_model: the Lagrange formula over the first d received slots)
and against the reference decoder's own output
(tests/golden/reedsol_recover.npz, and the captured FEC sets).  No GPU."""
import collections
import ctypes
import struct

import pytest

import fec_model
import fec_util
import recover_model as model
import recover_util as util
import reedsol_model as rs


@pytest.fixture(scope="module")
def ed():
    from firedancer_amd import ed25519
    return ed25519


def test_model_reproduces_the_reference_decoder():
    g = util.golden()
    cases = util.fixture_cases()
    assert int(g["cases"]) == 644 == len(cases)
    kinds = collections.Counter(c[0] for c in cases)
    assert set(kinds) == set(util.KINDS) and kinds["p_erased"] == 71 and kinds["all_data_erased"] == 70
    assert {(c[1], c[2]) for c in cases} >= {(1, 1), (1, 67), (67, 1), (67, 67)} | {(d, d) for d in range(33, 68)}
    assert {c[1] for c in cases if c[0] == "p_erased"} == set(range(1, 68))
    # a second accumulator pass and exactly one, of erased and of compared targets
    erased_counts = {sum(c[3]) for c in cases if c[6] == 0}
    compared = {c[1] + c[2] - sum(c[3]) - c[1] for c in cases if c[6] == 0}
    assert {32, 33, 67} <= erased_counts and {32, 33, 67} <= compared
    for kind, d, p, mask, bad, at, ret, rec in cases:
        before = util.fixture_slots(d, p, mask, bad, at)
        code, after = model.recover(before, mask, d)
        assert code == model.REF_CODES[ret], (kind, d, p)
        assert (kind == "partial") == (ret == -2) and ("flip" in kind) == (ret == -1)
        if ret == 0:
            assert [after[j] for j in range(d + p) if mask[j]] == rec, (kind, d, p)
            assert all(after[j] == before[j] for j in range(d + p) if not mask[j])


def test_library_against_model_and_fixture(ed):
    """every fixture case carried by real shreds, the fixture's bytes 0x20 into every protected region: the
    reference's return value (a set none of whose code shreds is received is ERR_SET before the decoder is asked,
    rule 10) and the reference's recovered bytes"""
    seen = collections.Counter()
    for kind, mask, st, want, ret, rec in util.fixture_sets():
        cnt = len(st)
        got = ed.fec_recover(list(st), mask)
        assert got == want, kind
        no_code = all(mask[j] or st[j][0x40] & 0xF0 == 0x80 for j in range(cnt))
        assert got[0] == (model.ERR_SET if no_code else model.REF_CODES[ret]), kind
        seen[got[0]] += 1
        if got[0] == 0:
            d = struct.unpack_from("<H", next(s for j, s in enumerate(st) if not mask[j] and s[0x40] & 0xF0 == 0x40), 0x53)[0]
            at = [model.region_at(j, d) + util.AT for j in range(cnt)]
            assert [got[1][j][at[j]:at[j] + 32] for j in range(cnt) if mask[j]] == rec, kind
    assert set(seen) == {0, model.ERR_SET, model.ERR_PARTIAL, model.ERR_CORRUPT} and seen[model.ERR_CORRUPT] == 284


def test_library_for_every_d_at_every_depth(ed):
    splits, masks, received, full = util.every_d()
    assert len(splits) == 74 and {fec_model.depth_of(d + p) for d, p in splits} == set(range(1, 9))
    for (d, p), mask, st, whole in zip(splits, masks, received, full):
        assert sum(mask) == p and all(s == bytes(len(s)) for s, m in zip(st, mask) if m)
        code, got = ed.fec_recover(list(st), mask)
        assert (code, got) == model.fill(list(st), mask) and code == 0, (d, p)
        # exactly rule 12's bytes changed: signature, code header, region; the proof stays zero
        assert util.changed_bytes_ok(st, got, mask, d), (d, p)
        P, first = rs.region(d + p), mask.index(0)
        for j in range(d + p):
            if not mask[j]:
                continue
            assert got[j][:64] == whole[first][:64]
            if j < d:
                assert got[j][0x40:0x40 + P] == whole[j][0x40:0x40 + P] and got[j][0x40 + P:] == bytes(1203 - 0x40 - P)
            else:
                # these sets' code shreds carry random idx fields: a recovered one gets the first received one's base
                ref = next(s for i, s in enumerate(st) if i >= d and not mask[i])
                idx = struct.unpack_from("<I", ref, 0x49)[0] - struct.unpack_from("<H", ref, 0x57)[0] + j - d
                want = whole[j][0x40:0x49] + struct.pack("<I", idx & 0xFFFFFFFF) + whole[j][0x4D:0x59 + P]
                assert got[j][0x40:0x59 + P] == want and got[j][0x59 + P:] == bytes(1228 - 0x59 - P)


@pytest.mark.parametrize("which", ["data", "parity", "mixed"])
def test_captured_sets_come_back(ed, which):
    """the 7 captured sets with p of their slots zeroed whole: fec_recover, then fec_root's proofs into the
    recovered slots -- the capture's 480 shreds byte for byte, signatures and proofs included"""
    total = 0
    for mask, st, whole in util.captured(which):
        assert sum(mask) == len(st) // 2 and whole != st
        code, got = ed.fec_recover(st, mask)
        if which == "parity":
            assert (code, got) == (model.ERR_SET, st)      # no code shred received: the resolver could not either
            m2 = mask[:-1] + (0,)                          # ... with one code shred it can
            st = model.erase(whole, m2)
            code, got = ed.fec_recover(st, m2)
            mask = m2
        assert code == 0
        rcode, _, proofs = ed.fec_root(got)
        assert rcode == 0
        depth = fec_model.depth_of(len(got))
        for j, s in enumerate(got):
            if mask[j]:
                at = fec_model.proof_at(s, depth)
                assert s[at:at + 20 * depth] == bytes(20 * depth)
                got[j] = s[:at] + proofs[j] + s[at + 20 * depth:]
        assert got == whole
        total += len(got)
    assert total == 480


def test_rules(ed):
    cases = util.rule_cases()
    names = {c[0] for c in cases}
    assert {"no_code_shred_received", "erased_data_slot_too_short", "erased_code_slot_too_short", "data_cnt_plus_one",
            "data_cnt_minus_one", "data_shred_at_or_behind_d", "partial_against_a_later_parse_error",
            "no_code_shred_before_partial", "erased_parse_then_code_cnt", "code_cnt_then_erased_parse",
            "corrupt_first_byte", "corrupt_last_byte", "corrupt_header_byte_of_a_basis_data_shred",
            "corrupt_before_rule_11", "recovered_slot", "recovered_version", "recovered_parent_off", "recovered_idx",
            "received_code_version_differs"} <= names
    assert {c[3] for c in cases} == {0, model.ERR_PARSE, model.UNSUPPORTED, model.ERR_SET, model.ERR_PARTIAL, model.ERR_CORRUPT}
    for name, mask, st, want in cases:
        code, got = ed.fec_recover(list(st), mask)
        assert code == want, name
        if want:
            assert got == list(st), name           # every nonzero code leaves every byte as it was
        else:
            assert (code, got) == model.fill(list(st), mask), name


def test_old_rules_keep_their_codes(ed):
    """fd_fec_core.h's rule cases with nothing erased"""
    for name, st, want in fec_util.bad_sets():
        mask = (0,) * len(st)
        assert model.fill(st, mask)[0] == want, name
        assert ed.fec_recover(st, mask) == (want, [bytes(s) for s in st]), name


def test_mutated_sets(ed):
    seen = set()
    for mask, st, want in util.mutated(400):
        assert ed.fec_recover(list(st), mask) == want
        seen.add(want[0])
    # under the model alone, with util.MUTATION_SEED
    assert seen == {0, model.ERR_PARSE, model.UNSUPPORTED, model.ERR_SET, model.ERR_PARTIAL, model.ERR_CORRUPT}


def test_python_mirror(ed):
    assert (ed.FEC_ERR_PARTIAL, ed.FEC_ERR_CORRUPT) == (model.ERR_PARTIAL, model.ERR_CORRUPT) == (-23, -24)
    assert ed.fec_recover([], []) == (ed.FEC_ERR_SET, [])
    ed._lib.fd_ed25519_hip_strerror.restype = ctypes.c_char_p
    texts = [ed._lib.fd_ed25519_hip_strerror(c) for c in (ed.FEC_ERR_PARTIAL, ed.FEC_ERR_CORRUPT)]
    assert all(t.startswith(b"FEC set: ") for t in texts) and texts[0] != texts[1]
    from firedancer_amd import tile
    assert tile.ABI_VERSION == 16
