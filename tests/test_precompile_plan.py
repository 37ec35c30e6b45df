"""The host side of the Ed25519 precompile path (fd_ed25519_hip_precompile_count
and _plan: the walk the device's stage kernel runs, compiled from the same
fd_precompile_core.h) against the test-side model (precompile_model.walk,
built on the reference's compiled parser).  No GPU."""
import pytest

import precompile_model as model
from precompile_util import max_entries_txn, mutated, rule_cases
from txn_util import ref_lib


@pytest.fixture(scope="module")
def ref():
    lib = ref_lib()
    if lib is None:
        pytest.skip("oracle/_ref not built")
    return lib


@pytest.fixture(scope="module")
def ed():
    from firedancer_amd import ed25519
    return ed25519


def check(ed, ref, payload):
    """count, plan and codes equal the model's; returns the model's walk"""
    w = model.walk(ref, payload)
    ents, code, instr = ed.precompile_plan(payload)
    got = [tuple(int(e[f]) for f in ("instr", "sig_off", "pub_off", "msg_off", "msg_sz", "pre")) for e in ents]
    if w is None:
        assert (ed.precompile_count(payload), got, code, instr) == (0, [], ed.PRECOMPILE_PARSE_FAILED, 0xFF)
        return None
    want, hdr_instr = w
    assert ed.precompile_count(payload) == len(want)
    assert got == want
    assert (code, instr) == ((ed.PRECOMPILE_ERR_INSTR_DATA_SIZE if hdr_instr != 0xFF else 0), hdr_instr)
    return w


def test_codes_are_the_references(ed):
    assert (ed.PRECOMPILE_ERR_SIGNATURE, ed.PRECOMPILE_ERR_DATA_OFFSET, ed.PRECOMPILE_ERR_INSTR_DATA_SIZE) == (-3, -4, -5)
    assert (model.PARSE_FAILED, model.BAD_RESERVATION) == (ed.PRECOMPILE_PARSE_FAILED, ed.PRECOMPILE_BAD_RESERVATION)
    assert ed.PRECOMPILE_ENT_MAX == (1232 - 2) // 14


def test_rule_edges(ed, ref, oracle):
    """One transaction per rule edge; and the expectations the cases were
    built for, so a case that stopped reaching its edge is noticed."""
    seen = {}
    for name, payload in rule_cases(oracle):
        seen[name] = (check(ed, ref, payload), model.judge(ref, payload))
    code = {name: j[0] for name, (_, j) in seen.items()}
    for name in ("data_sz0_d0", "data_sz1_d0", "data_sz2_d1", "data_sz3_d0", "data_sz15_d1", "cnt0_sz16", "cnt0_sz40",
                 "table_one_short"):
        assert code[name] == -5, name
    for name in ("data_sz2_d0", "table_exact", "pad_byte_nonzero", "idx_this", "idx_own", "idx_other", "msg_sz0",
                 "msg_sz0_at_end", "msg_overlaps_pub", "two_entries_one_sig", "other_program_same_data",
                 "other_program_bad_header", "id_listed_other_named", "no_ed25519_account", "instr64_lookup63",
                 "legacy_two_entries", "v0_luts", "bound_eq_s", "bound_eq_p", "bound_eq_m"):
        assert code[name] == 0, name
    for name in [f"idx_{k}_{w}" for k in ("instr_cnt", "fffe") for w in "spm"] + [f"bound_over_{w}" for w in "spm"]:
        assert code[name] == -4, name
    for name in ("msg_overlaps_sig", "v0_bad_sig"):
        assert code[name] == -3, name
    for name in ("rejected_trailing", "rejected_truncated", "rejected_empty"):
        assert code[name] == model.PARSE_FAILED and seen[name][0] is None, name
    assert seen["prio_sig_then_offset"][1][:2] == (-3, 0) and seen["prio_offset_then_sig"][1][:2] == (-4, 0)
    assert seen["prio_second_instr_fails"][1][:2] == (-3, 2) and seen["prio_both_instr_fail"][1][:2] == (-3, 0)
    assert seen["prio_header_then_sig"][1][:2] == (-5, 0) and seen["prio_sig_then_header"][1][:2] == (-3, 0)
    assert len(seen["two_entries_one_sig"][0][0]) == 2 and len(seen["instr64_lookup63"][0][0]) == 1
    assert seen["other_program_same_data"][0] == ([], 0xFF) and seen["data_sz2_d0"][0] == ([], 0xFF)


def test_most_entries_of_one_payload(ed, ref, oracle):
    payload, n = max_entries_txn(oracle)
    assert len(payload) <= 1232 and 64 < n <= ed.PRECOMPILE_ENT_MAX
    assert n == 68   # one signer, two accounts, one aliased 97-byte (sig, key, message)
    ents, hdr = check(ed, ref, payload)
    assert len(ents) == n and len(set(e[1:] for e in ents)) == 1 and hdr == 0xFF


def test_mutations(ed, ref, oracle):
    """About 2,000 structural mutations of valid precompile transactions:
    count, plan and codes equal the model's on every one."""
    muts = mutated(oracle)
    assert len(muts) >= 2000
    kinds = {"rejected": 0, "header": 0, "offset": 0, "clean": 0}
    for p in muts:
        w = check(ed, ref, p)
        kinds["rejected" if w is None else "header" if w[1] != 0xFF else
              "offset" if any(e[5] for e in w[0]) else "clean"] += 1
    assert all(v >= 20 for v in kinds.values()), kinds
