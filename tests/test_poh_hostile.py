"""Hostile input to the proof-of-history rules and the block walk:
fd_poh_core.h compiled with a stand-alone main (tests/poh_walk_main.c) under
ASan and UBSan, run on the fixture's microblocks, the captured batch, every
signature count and k, the rule cases, the captured batch and a two-batch
block cut at every byte of the first microblock and around every boundary
(the CPU test's cuts, all of them), hostile counts, and 2,000 seeded mutations
and truncations, every block in a heap block of exactly its size.  A program of its own: nothing is loaded into this interpreter."""
import random
import struct
import subprocess

import pytest

import poh_model as model
import poh_util as util
import san_build


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    return san_build.build("poh_walk_main.c", tmp_path_factory.mktemp("poh_walk") / "poh_walk")


def block_case(blk, in_state=bytes(32), bound=4096):
    return struct.pack("<BQ", 0, bound) + in_state + struct.pack("<I", len(blk)) + blk


def desc_case(d, bound=4096):
    return (struct.pack("<BQI", 1, bound, len(d.buf)) + d.buf + struct.pack("<I", d.n) + d.hdr_off.tobytes() +
            d.in_off.tobytes() + d.sig_first.tobytes() + struct.pack("<I", len(d.sig_off)) + d.sig_off.tobytes())


def test_walk_of_hostile_blocks_is_clean_and_agrees_with_the_model(walker, tmp_path):
    blk = util.captured_block()
    # the CPU test's cuts, every one: a read past a cut shows only here, where the block ends with its heap block
    cuts = util.truncation_cuts(blk)
    assert len(cuts) > 3700
    blocks = [blk, b""] + [blk[:c] for c in cuts]
    two = util.two_batches(random.Random(283), bytes(32))
    blocks += [two] + [two[:c] for c in util.truncation_cuts(two)]
    blocks += [struct.pack("<Q", cnt) + blk[8:] for cnt in (0, 1 << 63, (1 << 64) - 1, 63, 65)]
    blocks += [blk + junk for junk in (b"\0", bytes(8), struct.pack("<Q", 1) + bytes(47), struct.pack("<Q", 1) + bytes(48))]
    mutated = util.mutated()
    assert len(mutated) == 2000
    blocks += mutated
    huge = (1 << 64) - 1
    descs = [(util.fixture_microblocks()[0], 4096), (util.shapes(), 4096), (util.broken(util.shapes())[0], 4096),
             (util.captured(), 4096)]
    # the bound at k - 1, k, k + 1, and a hash count of all ones: UNSUPPORTED at once
    state = model.append(bytes(32), 37)
    lone = bytes(32) + struct.pack("<Q", 37) + state + struct.pack("<Q", 0)
    descs += [(util.Desc(lone, [32], [0], [0, 0], []), b) for b in (36, 37, 38)]
    for txn_cnt in (0, 1):
        buf = bytes(32) + struct.pack("<Q", huge) + bytes(32) + struct.pack("<Q", txn_cnt) + bytes(64)
        descs += [(util.Desc(buf, [32], [0], [0, txn_cnt], [80]), b) for b in (0, 4096, 1 << 17)]
    # offsets at the buffer's end and ones that would wrap
    for hdr_off, in_off, sig_off in ((len(lone) - 47, 0, 0), (32, len(lone) - 31, 0), (huge - 8, 0, 0), (32, huge, 0)):
        descs.append((util.Desc(lone, [hdr_off], [in_off], [0, 0], []), 4096))
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<I", len(blocks) + len(descs)) + b"".join(block_case(b) for b in blocks) +
                    b"".join(desc_case(d, b) for d, b in descs))
    r = subprocess.run([walker, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw, at, walk_codes, codes = fout.read_bytes(), 0, set(), set()

    def check(d, bound, k):
        nonlocal at
        want_codes, want_states = d.want(bound)
        for i in range(d.n):
            code, = struct.unpack_from("<b", raw, at)
            assert code == want_codes[i], (k, i)
            assert raw[at + 1:at + 33] == want_states[i].tobytes(), (k, i)
            codes.add(code)
            at += 33

    for k, b in enumerate(blocks):
        code, n = struct.unpack_from("<iI", raw, at)
        at += 8
        want = model.walk(b, first_in_off=-32)
        assert code == want[0], k
        walk_codes.add(code)
        if code == 0:
            assert n == len(want[1]), k
            check(util.describe(b, bytes(32)), 4096, k)
    for k, (d, bound) in enumerate(descs):
        check(d, bound, ("desc", k))
    assert at == len(raw) and walk_codes == {0, -16} and codes == {0, -16, -18, -25}
