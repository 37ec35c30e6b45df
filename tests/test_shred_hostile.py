"""Hostile input to the shred rules and hashes: fd_shred_core.h compiled with a
stand-alone main (tests/shred_walk_main.c) under ASan and UBSan, run on
mutated, rule-edge and truncated shreds held in heap blocks of exactly their
size.  A program of its own: nothing is loaded into this interpreter."""
import struct
import subprocess

import pytest

import san_build
from shred_util import every_depth, fixture, mutated, rule_cases


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    return san_build.build("shred_walk_main.c", tmp_path_factory.mktemp("shred_walk") / "shred_walk")


def test_walk_of_hostile_shreds_is_clean_and_agrees_with_the_library(walker, oracle, tmp_path):
    from firedancer_amd import ed25519 as ed
    shreds = list(mutated()) + [s for _, s, _ in rule_cases(oracle)[0]] + every_depth(oracle)[0]
    # and every prefix of one captured data shred and of one code shred's header
    data = next(s for s in fixture()[0] if len(s) == 1203)
    code = next(s for s in fixture()[0] if len(s) == 1228)
    shreds += [data[:k] for k in range(len(data))] + [code[:k] for k in range(0x50, 0x60)] + [code[:1227]]
    path = tmp_path / "shreds.bin"
    path.write_bytes(struct.pack("<I", len(shreds)) + b"".join(struct.pack("<I", len(s)) + s for s in shreds))
    r = subprocess.run([walker, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(shreds)
    for s, line in zip(shreds, lines):
        c, root = ed.shred_root(s)
        assert line.split() == [str(c), root.hex() if root else "-"], (s[:0x60].hex(), line)
