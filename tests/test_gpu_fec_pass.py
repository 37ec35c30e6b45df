"""GPU: the passes of the three FEC-set host wrappers (fd_ed25519_hip_fec_seal_host,
_fec_parity_host, _fec_recover_host; firedancer_amd/csrc/fd_fec_pass.h) where
the existing tests do not take them: a pass cut by the set bound and not by
the shred bound, and shreds at the edges of a staging slot -- one byte and
many bytes longer than FD_SHRED_MAX_SZ, which travel as their head, a code
shred shorter than its header, which travels zero-filled, an erased slot of
no bytes at all.  Through fec_seal_flat, fec_parity_flat and fec_recover_flat;
the codes and every byte afterwards are the models' (tests/fec_model.py,
reedsol_model.py, recover_model.py).  A small engine: compact tables,
512-signature chunks."""
import random

import pytest

import fec_model
import fec_util
import recover_model
import reedsol_model as rs

pytestmark = pytest.mark.gpu

FRONTS = ("seal", "parity", "recover")
PRIV = bytes(range(7, 39))
SET, PARSE = fec_model.ERR_SET, fec_model.ERR_PARSE


@pytest.fixture(scope="module")
def ed():
    from firedancer_amd import ed25519
    return ed25519


@pytest.fixture(scope="module")
def eng(ed):
    e = ed.Engine(0, max_chunk=512, compact=True)
    yield e
    e.close()


def good(front, rng, cnt, d, mask):
    """a set of d + (cnt - d) shreds the front accepts, as it goes in: for the
    recovery the parity filled and the slots of mask holding junk"""
    st = fec_util.make_set(rng, cnt, data_cnt=d)
    if front != "recover":
        return st
    full = rs.fill(st)[1]
    return [rng.randbytes(len(s)) if e else s for s, e in zip(full, mask)]


def model(front, oracle, shreds, mask):
    """(code, the shreds afterwards, root, signature) of one set"""
    if front == "seal":
        return fec_model.seal(oracle, shreds, PRIV)
    return (rs.fill(shreds) if front == "parity" else recover_model.fill(shreds, mask)) + (None, None)


def run_and_check(front, eng, oracle, sets, masks, set_first=None):
    """the sets through the front's *_flat against the model, set by set; -> the model's codes"""
    if set_first is None:
        set_first = [0]
        for s in sets:
            set_first.append(set_first[-1] + len(s))
    flat, flags = [x for s in sets for x in s], [x for m in masks for x in m]
    ranges = [flat[a:b] if a < b else [] for a, b in zip(set_first, set_first[1:])]
    range_masks = [flags[a:b] if a < b else [] for a, b in zip(set_first, set_first[1:])]
    want = [model(front, oracle, s, m) for s, m in zip(ranges, range_masks)]
    if front == "seal":
        codes, out, roots, sigs = eng.fec_seal_flat(flat, set_first, PRIV)
        fec_util.check_outputs(want, codes, roots, sigs)
    elif front == "parity":
        codes, out = eng.fec_parity_flat(flat, set_first)
    else:
        codes, out = eng.fec_recover_flat(flat, flags, set_first)
    assert codes.tolist() == [w[0] for w in want]
    for (a, b), w in zip(zip(set_first, set_first[1:]), want):
        assert out[a:b] == [bytes(x) for x in w[1]], (a, b, w[0])
    return [w[0] for w in want]


@pytest.mark.parametrize("front", FRONTS)
def test_pass_cut_by_the_set_bound(front, eng, oracle):
    """16,385 empty ranges, then a good set of 2 + 1: the first pass takes 16,384 sets and stages nothing, the
    second the last empty range and the good set"""
    rng = random.Random(401)
    mask = (1, 0, 0)
    st = good(front, rng, 3, 2, mask)
    codes = run_and_check(front, eng, oracle, [st], [mask], set_first=[0] * 16386 + [3])
    assert codes == [SET] * 16385 + [0]


def longer(rng, st, j, sz):
    """shred j of the set grown to sz bytes"""
    return [s + rng.randbytes(sz - len(s)) if i == j else s for i, s in enumerate(st)]


@pytest.mark.parametrize("front", FRONTS)
def test_shreds_at_the_edges_of_a_slot(front, eng, oracle):
    """sets of 3 + 2 whose first code shred has 1,229 and 4,000 bytes -- accepted, and rejected for another shred's
    depth -- and the front's own short slots, each between good sets: a rejected set keeps every byte, those past
    1,228 too, an accepted one every byte past 1,228, and the neighbours are processed"""
    rng = random.Random(409)
    masks = {"first": (1, 0, 0, 0, 1), "last": (0, 0, 0, 0, 1), "none": (0,) * 5}

    def make(mask="first"):
        return good(front, rng, 5, 3, masks[mask]), masks[mask]

    def wrong_depth(st):
        """data shred 1, received in every mask, with the proof depth of a smaller set: it parses, and fails rule 2"""
        return [s[:0x40] + bytes([s[0x40] ^ 1]) + s[0x41:] if i == 1 else s for i, s in enumerate(st)]

    sets, want = [], []

    def add(st_mask, code, edit=lambda st: st):
        sets.append((edit(st_mask[0]), st_mask[1]))
        want.append(code)

    add(make(), 0)
    add(make("last"), 0, lambda st: longer(rng, st, 3, 1229))
    add(make(), SET, lambda st: wrong_depth(longer(rng, st, 3, 4000)))
    add(make("last"), 0)
    add(make(), 0, lambda st: longer(rng, st, 3, 4000))
    add(make(), SET, lambda st: wrong_depth(longer(rng, st, 3, 1229)))
    if front == "parity":   # a code shred cut inside its header: it travels as 0x59 bytes, zero-filled
        add(make(), PARSE, lambda st: st[:4] + [st[4][:0x41]])
        add(make(), PARSE, lambda st: st[:3] + [st[3][:0x58]] + st[4:])
    if front == "recover":  # an erased slot of no bytes, and one a byte longer than its staging slot
        add(make(), PARSE, lambda st: st[:4] + [b""])
        add(make(), 0, lambda st: longer(rng, st, 4, 1229))
    add(make("none" if front == "recover" else "first"), 0)
    assert run_and_check(front, eng, oracle, [s for s, _ in sets], [m for _, m in sets]) == want
