"""Hostile input to the recovery's rules and its decoder: fd_reedsol_core.h
compiled with a stand-alone main (tests/recover_walk_main.c) under ASan and
UBSan, run on the fixture's cases, a received set of every number of data
shreds, the captured sets with half of their slots erased, the rule cases,
mutated and truncated sets whose slots are held in heap blocks of exactly their
size.  A program of its own: nothing is loaded into this interpreter."""
import random
import struct
import subprocess

import pytest

import fec_util
import recover_model as model
import recover_util as util
import reedsol_model as rs
import san_build


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    return san_build.build("recover_walk_main.c", tmp_path_factory.mktemp("recover_walk") / "recover_walk")


def test_walk_of_hostile_sets_is_clean_and_agrees_with_the_model(walker, tmp_path):
    sets = [(mask, st, want) for _, mask, st, want, _, _ in util.fixture_sets()]
    _, masks, received, _ = util.every_d()
    sets += [(m, st, None) for m, st in zip(masks, received)]
    sets += [(m, st, None) for which in ("data", "parity", "mixed") for m, st, _ in util.captured(which)]
    sets += [(m, st, None) for _, m, st, _ in util.rule_cases()]
    sets += [((0,) * len(st), st, None) for _, st, _ in fec_util.bad_sets()]
    mutated = util.mutated()
    assert len(mutated) == 2000
    sets += list(mutated)
    # one slot of a small set cut at every header byte and around both sizes, received and erased: a data and a
    # code slot
    rng = random.Random(251)
    base = rs.fill(fec_util.make_set(rng, 4))[1]
    for j in (0, 3):
        for k in list(range(0, 0x5C)) + [600, 1201, 1202, 1203, 1226, 1227]:
            for mask in ((0, 0, 0, 0), tuple(int(i == j) for i in range(4)), tuple(int(i == 1) for i in range(4))):
                sets.append((mask, base[:j] + [base[j][:k]] + base[j + 1:], None))
    assert len(sets) > 3300
    fin, fout = tmp_path / "sets.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<I", len(sets)) + b"".join(
        struct.pack("<I", len(st)) + b"".join(struct.pack("<BI", 1 if e else 0, len(s)) + bytes(s) for s, e in zip(st, mask))
        for mask, st, _ in sets))
    r = subprocess.run([walker, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw, at, codes = fout.read_bytes(), 0, set()
    for k, (mask, st, want) in enumerate(sets):
        code, = struct.unpack_from("<i", raw, at)
        at += 4
        want, filled = model.fill(list(st), mask) if want is None else want
        assert code == want, k
        codes.add(code)
        if code == 0:
            size = sum(len(s) for s in st)
            assert raw[at:at + size] == b"".join(filled), k
            at += size
    assert at == len(raw) and codes == {0, -16, -18, -19, -23, -24}
