"""CPU: the shredder's counts, plan and headers (fd_shredder_core.h through
fd_ed25519_hip_shredder_count and fd_ed25519_hip_shredder, include/
fd_ed25519_hip.h Part 2j) and the test-side model against the reference
shredder's own sets (tests/golden/shredder.npz) and, with the parity and the
seal behind them, against the reference's captured shreds."""
import fec_model
import fec_util
import poh_util
import shredder_model as model
import shredder_util as util
from shred_util import fixture


def ed():
    from firedancer_amd import ed25519
    return ed25519


def test_fixture_covers_every_edge():
    cases = util.fixture_cases()
    sizes = [len(b[0]) for c in cases for b in c]
    assert sizes[:13] == [1, 1015, 1016, 9135, 9136, 31840, 31841, 62400, 62401, 63679, 63680, 63681, 95520]
    assert [len(b[0]) for b in cases[13]] == [237320, 1016] and cases[13][1][1]["data_idx"] == 240
    assert cases[14][0][1]["data_idx"] == 0xFFFFFFF0 and cases[14][0][1]["parity_idx"] == 0xFFFFFFF0
    descs = [b[1] for c in cases for b in c]
    assert {d["block_complete"] for d in descs} == {0, 1} and {0, 63, 64} <= {d["reference_tick"] for d in descs}
    assert any(d["parent_off"] == 0x1FFFF for d in descs)


def test_model_and_host_shredder_against_the_reference():
    """every fixture case: the counts, every set's (d, p), the front's bytes
    from the library and the model, and the finished shreds' digests"""
    lib = ed()
    whole, at = util.whole_shreds(), 0
    for c, case in enumerate(util.fixture_cases()):
        for batch, dsc, counts, dp, digest in case:
            assert model.count(len(batch)) == counts == lib.shredder_count(len(batch))
            assert [(p[2], p[3]) for p in model.plan(len(batch))] == dp
            front = model.front(batch, dsc)
            code, got = lib.shredder(batch, util.ed_desc(lib, dsc))
            assert code == 0 and got == front, (c, len(batch))
            done = []
            for st in got:
                code, filled = lib.fec_parity(st)
                assert code == 0
                code, sealed, _, _ = fec_model.seal(None, filled, None)
                assert code == 0
                done.append(sealed)
            assert util.digests(done) == digest, (c, len(batch))
            assert util.blank_front(done) == front
            if c < 3:
                flat = [s for st in done for s in st]
                assert flat == whole[at:at + len(flat)]
                at += len(flat)
    assert at == len(whole)


def test_a_batch_of_no_bytes():
    lib = ed()
    assert lib.shredder_count(0) == (0, 0, 0) == model.count(0)
    assert lib.shredder(b"", lib.shredder_desc()) == (lib.SHREDDER_ERR_BATCH, [])


def test_count_against_the_model():
    lib = ed()
    for sz in range(1, 130001):
        assert lib.shredder_count(sz) == model.count(sz), sz


def last_set_edges():
    """the sizes r of a last set around which its data shred count steps, in
    each of the four branches: k whole payloads, one byte fewer and one more"""
    out = set()
    for lo, hi, per in ((1, 9135, 1015), (9136, 31840, 995), (31841, 62400, 975), (62401, 63679, 955)):
        out |= {lo, hi}
        for k in range(1, 68):
            out |= {r for r in (k * per - 1, k * per, k * per + 1) if lo <= r <= hi}
    return sorted(out)


def test_every_last_set_size_fills_its_shreds():
    """the library's shreds (fd_shredder_core_plan, _payload and the header
    writers through fd_ed25519_hip_shredder) at every size at which a last
    set's d steps: rule 3's payload, only the last data shred short, the size
    fields, the batch's bytes back in order, and the model's front"""
    lib = ed()
    edges = last_set_edges()
    # every d a last set can have: 62,400 bytes are 64 shreds of 975 and 62,401 are 66 of 955
    assert {model.split(r)[0] for r in edges} == set(range(1, 68)) - {65} and {1, 1015, 1016, 9135, 9136, 31840, 31841, 62400, 62401, 63679} <= set(edges)
    dsc = model.desc(slot=11, data_idx=5, parity_idx=9, version=2, parent_off=1, reference_tick=7, block_complete=1)
    for r in edges:
        batch = model.seeded_batch(r, r)
        code, sets = lib.shredder(batch, util.ed_desc(lib, dsc))
        assert code == 0 and len(sets) == 1, r
        data = [s for s in sets[0] if s[0x40] & 0xF0 == 0x80]
        d, p = len(data), len(sets[0]) - len(data)
        assert (d, p) == model.split(r) == lib.shredder_count(r)[1:], r
        payload = 1115 - 20 * fec_model.depth_of(d + p)
        carried = [int.from_bytes(s[0x56:0x58], "little") - 0x58 for s in data]
        assert carried[:-1] == [payload] * (d - 1) and 1 <= carried[-1] <= payload and sum(carried) == r, r
        assert b"".join(s[0x58:0x58 + n] for s, n in zip(data, carried)) == batch, r
        assert sets == model.front(batch, dsc), r


def test_the_capture(oracle):
    """the capture's batch, slot 0, version 0, block_complete 1, through
    ed.shredder, ed.fec_parity and the model's seal with the capture's key:
    the reference's 480 captured shreds byte for byte"""
    lib = ed()
    blk = poh_util.captured_block()
    assert len(blk) == 237320
    code, sets = lib.shredder(blk, lib.shredder_desc(slot=0, version=0, parent_off=0, reference_tick=0, block_complete=1))
    assert code == 0 and [len(s) for s in sets] == [64] * 6 + [96]
    done = []
    for st in sets:
        code, filled = lib.fec_parity(st)
        assert code == 0
        code, sealed, _, _ = fec_model.seal(oracle, filled, fec_util.private_key())
        assert code == 0
        done.append(tuple(sealed))
    assert tuple(done) == fec_util.captured_sets()
    flat = [s for st in done for s in st]
    assert len(flat) == 480 and sorted(flat) == sorted(fixture()[0])
