"""Hostile input to the shredder's core: fd_shredder_core.h compiled with a
stand-alone main (tests/shredder_walk_main.c) under ASan and UBSan, run on
every fixture case and on 2,000 seeded descriptors and sizes, with the batch
and every shred in heap blocks of exactly their size, and on seeded batch
judgements.  A program of its own: nothing is loaded into this interpreter."""
import random
import struct
import subprocess

import pytest

import san_build
import shredder_model as model
import shredder_util as util

EDGES = (1, 2, 954, 955, 956, 974, 975, 976, 994, 995, 996, 1014, 1015, 1016, 9135, 9136, 31839, 31840, 31841, 62400, 62401,
         63679, 63680, 63681, 95519, 95520, 95521)


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    return san_build.build("shredder_walk_main.c", tmp_path_factory.mktemp("shredder_walk") / "shredder_walk")


def pack_desc(d):
    return struct.pack("<QIIHHBBxx", d["slot"], d["data_idx"] & 0xFFFFFFFF, d["parity_idx"] & 0xFFFFFFFF, d["version"] & 0xFFFF,
                       d["parent_off"] & 0xFFFF, d["reference_tick"] & 0xFF, d["block_complete"] & 0xFF)


def test_walk_is_clean_and_agrees_with_the_model(walker, tmp_path):
    rng = random.Random(379)
    batches = [(b[0], b[1]) for case in util.fixture_cases() for b in case]
    for t in range(2000):
        sz = rng.choice(EDGES) if t % 4 == 0 else rng.randrange(1, 4000) if t % 4 == 1 else rng.randrange(1, 70000) if t % 40 else \
            rng.randrange(1, 200000)
        dsc = model.desc(rng.getrandbits(64), rng.getrandbits(32), rng.getrandbits(32), rng.getrandbits(16), rng.getrandbits(16),
                         rng.getrandbits(8), rng.getrandbits(8))
        batches.append((rng.randbytes(sz), dsc))
    batches.append((b"", model.desc()))
    assert len(batches) == 16 + 2000 + 1
    judgements = []
    for t in range(2000):
        sz = rng.choice((0, 1, 1016, 63679, 63680, 95520))
        sets, nd, npar = model.count(sz)
        s0, h0 = rng.randrange(0, 50), rng.randrange(0, 5000)
        j = [rng.randrange(0, 100000), sz, 100000 + rng.randrange(0, 100000), s0, s0 + sets, s0 + sets + rng.randrange(0, 3), h0,
             h0 + nd + npar, h0 + nd + npar + rng.randrange(0, 3)]
        if t % 3 == 1:
            j[rng.randrange(9)] = rng.choice((0, 1, 2**32 - 1, 2**64 - 1, rng.getrandbits(20)))
        elif t % 3 == 2:
            k = rng.randrange(9)
            j[k] = max(0, j[k] + rng.choice((-1, 1)))
        judgements.append(j)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<I", len(batches)) + b"".join(pack_desc(d) + struct.pack("<I", len(b)) + b for b, d in batches) +
                    struct.pack("<I", len(judgements)) + b"".join(struct.pack("<9Q", *j) for j in judgements))
    r = subprocess.run([walker, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw, at = fout.read_bytes(), 0
    for t, (b, d) in enumerate(batches):
        code, = struct.unpack_from("<i", raw, at)
        at += 4
        if not b:
            assert code == model.ERR_BATCH
            continue
        assert code == 0, t
        want = model.front(b, d)
        sets, nd, npar = struct.unpack_from("<III", raw, at)
        at += 12
        assert (sets, nd, npar) == model.count(len(b)) and sets == len(want)
        first = struct.unpack_from(f"<{sets + 1}I", raw, at)
        at += 4 * (sets + 1)
        assert list(first) == [sum(len(s) for s in want[:k]) for k in range(sets + 1)]
        for st in want:
            P = 1139 - 20 * (len(st) - 1).bit_length()
            for s in st:
                if len(s) == 1228:       # the parity region is not the front's: the block's fill comes back
                    s = s[:0x59] + b"\xa5" * P + s[0x59 + P:]
                assert raw[at:at + len(s)] == s, t
                at += len(s)
    got = struct.unpack_from(f"<{len(judgements)}i", raw, at)
    at += 4 * len(judgements)
    want = [model.judge(j[1], j[0], j[2], *j[3:]) for j in judgements]
    assert list(got) == want and {0, model.ERR_BATCH, model.BAD_RESERVATION} == set(want)
    assert at == len(raw)
