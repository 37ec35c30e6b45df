"""Hostile input to the parity's rules and its encoder: fd_reedsol_core.h
compiled with a stand-alone main (tests/reedsol_walk_main.c) under ASan and
UBSan, run on the captured sets, a set of every number of data shreds, the
old and new rule cases, mutated and truncated sets whose shreds are held in
heap blocks of exactly their size.  A program of its own: nothing is loaded
into this interpreter."""
import random
import struct
import subprocess

import pytest

import fec_util
import reedsol_model as rs
import reedsol_util as util
import san_build


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    return san_build.build("reedsol_walk_main.c", tmp_path_factory.mktemp("reedsol_walk") / "reedsol_walk")


def test_walk_of_hostile_sets_is_clean_and_agrees_with_the_model(walker, tmp_path):
    sets = [list(s) for s in fec_util.captured_sets()] + [rs.blank_parity(list(s)) for s in fec_util.captured_sets()[5:]]
    sets += [list(s) for s in util.every_d()[1]] + [s for _, s, _ in util.all_bad_sets()]
    sets += [list(s) for s in fec_util.mutated_sets()]
    assert len(fec_util.mutated_sets()) == 2000
    # one shred of a small set cut at every header byte and around both sizes: a data and a code shred
    rng = random.Random(193)
    base = fec_util.make_set(rng, 4)
    for j in (0, 3):
        for k in list(range(0, 0x5C)) + [600, 1201, 1202, 1203, 1226, 1227]:
            sets.append(base[:j] + [base[j][:k]] + base[j + 1:])
    assert len(sets) > 2200
    fin, fout = tmp_path / "sets.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<I", len(sets)) + b"".join(
        struct.pack("<I", len(st)) + b"".join(struct.pack("<I", len(s)) + bytes(s) for s in st) for st in sets))
    r = subprocess.run([walker, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw, at, codes = fout.read_bytes(), 0, set()
    for k, st in enumerate(sets):
        code, = struct.unpack_from("<i", raw, at)
        at += 4
        want, filled = rs.fill(st)
        assert code == want, k
        codes.add(code)
        if code == 0:
            size = sum(len(s) for s in st)
            assert raw[at:at + size] == b"".join(filled), k
            at += size
    assert at == len(raw) and codes == {0, -16, -18, -19}
