"""Hostile input to the Ed25519 precompile walk: fd_precompile_core.h and
fd_txn_parse_core.h compiled with a stand-alone main
(tests/precompile_walk_main.c) under ASan and UBSan, run on mutated
precompile transactions held in heap blocks of exactly their size.  A
program of its own: nothing is loaded into this interpreter."""
import struct
import subprocess

import pytest

import san_build
from precompile_util import max_entries_txn, mutated, rule_cases


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    return san_build.build("precompile_walk_main.c", tmp_path_factory.mktemp("precompile_walk") / "precompile_walk")


def test_walk_of_hostile_payloads_is_clean_and_agrees_with_the_library(walker, oracle, tmp_path):
    from firedancer_amd import ed25519 as ed
    payloads = mutated(oracle) + [p for _, p in rule_cases(oracle)] + [max_entries_txn(oracle)[0]]
    # and every prefix of one valid precompile transaction
    whole = dict(rule_cases(oracle))["legacy_two_entries"]
    payloads += [whole[:k] for k in range(len(whole))]
    path = tmp_path / "payloads.bin"
    path.write_bytes(struct.pack("<I", len(payloads)) + b"".join(struct.pack("<I", len(p)) + p for p in payloads))
    r = subprocess.run([walker, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(payloads)
    for p, line in zip(payloads, lines):
        ents, code, instr = ed.precompile_plan(p)
        h = 0
        for e in ents:
            h = (h * 1000003 + int(e["instr"]) + 3 * (int(e["pre"]) & 0xFF) + 5 * int(e["sig_off"]) + 7 * int(e["pub_off"])
                 + 11 * int(e["msg_off"]) + 13 * int(e["msg_sz"])) & (2**64 - 1)
        assert line.split() == [str(ed.precompile_count(p)), str(len(ents)), str(code), str(instr), str(h)], (p.hex(), line)
