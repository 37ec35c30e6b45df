"""Hostile input to the FEC set rules, the tree and the proofs: fd_fec_core.h
compiled with a stand-alone main (tests/fec_walk_main.c) under ASan and UBSan,
run on the captured sets, every tree shape, rule-breaking, mutated and
truncated sets whose shreds are held in heap blocks of exactly their size.  A
program of its own: nothing is loaded into this interpreter."""
import random
import struct
import subprocess

import pytest

import fec_util as util
import san_build


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    return san_build.build("fec_walk_main.c", tmp_path_factory.mktemp("fec_walk") / "fec_walk")


def test_walk_of_hostile_sets_is_clean_and_agrees_with_the_library(walker, tmp_path):
    from firedancer_amd import ed25519 as ed
    sets = [list(s) for s in util.captured_sets()] + [util.blank(s) for s in util.captured_sets()[5:]]
    sets += util.shape_sets() + [s for _, s, _ in util.bad_sets()] + [list(s) for s in util.mutated_sets()]
    # one shred of a small set cut at every header byte and around both sizes, first and last in the set
    rng = random.Random(107)
    base = util.make_set(rng, 4)
    for j in (0, 3):
        for k in list(range(0, 0x5C)) + [600, 1201, 1202, 1203, 1226, 1227]:
            sets.append(base[:j] + [base[j][:k]] + base[j + 1:])
    assert len(sets) > 2200
    path = tmp_path / "sets.bin"
    path.write_bytes(struct.pack("<I", len(sets)) + b"".join(
        struct.pack("<I", len(st)) + b"".join(struct.pack("<I", len(s)) + bytes(s) for s in st) for st in sets))
    r = subprocess.run([walker, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(sets)
    codes = set()
    for st, line in zip(sets, lines):
        code, root, proofs = ed.fec_root(st)
        codes.add(code)
        want = [str(code), root.hex(), b"".join(proofs).hex() or "-"] if code == 0 else [str(code), "-", "-"]
        assert line.split() == want, (len(st), line[:100])
    assert codes == {0, -16, -18, -19}
