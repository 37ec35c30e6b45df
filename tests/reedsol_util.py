"""Builds FEC sets for the parity tests: one set of every number of data shreds
with the parity count the reference's shredder gives it
(tests/golden/reedsol.npz records the shredder's table), the extremes, and the
sets that break one of fd_reedsol_core.h's rules -- each made once a process
and shared, with the model's answer beside it."""
import functools
import random
import struct

import numpy as np

import fec_model
import fec_util
import reedsol_model as rs
from conftest import load_golden


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("reedsol")


def shredder_p(d):
    """the parity shreds the reference's shredder makes for d data shreds"""
    return int(golden()["shredder_parity"][d])


EXTREMES = ((1, 1), (1, 67), (67, 1), (67, 67))
# the shredder's pairs start at 1 + 17, depth 5: sets of depth 2, 3 and 4, so that every P occurs
SHALLOW = ((1, 2), (2, 3), (5, 4))


@functools.lru_cache(maxsize=None)
def every_d():
    """((d, p), ...), (set, ...), (the set as the model fills it, ...): every
    d in 1..67 with the shredder's p, then the extremes, then the shallow sets"""
    rng = random.Random(151)
    splits = tuple((d, shredder_p(d)) for d in range(1, 68)) + EXTREMES + SHALLOW
    sets = tuple(tuple(fec_util.make_set(rng, d + p, data_cnt=d)) for d, p in splits)
    want = []
    for s in sets:
        code, filled = rs.fill(list(s))
        assert code == 0
        want.append(tuple(filled))
    return splits, sets, tuple(want)


def _edit(s, at, fmt, *v):
    s = bytearray(s)
    struct.pack_into(fmt, s, at, *v)
    return bytes(s)


@functools.lru_cache(maxsize=None)
def rule_cases():
    """((name, set, the code the rules give, whether fec_model's rules alone
    pass the set), ...): the sets that break one of the parity's own rules"""
    rng = random.Random(157)
    out = []

    def add(name, s, want, seal_passes):
        assert rs.parity_code(s) == want, (name, rs.parity_code(s), want)
        assert (fec_model.set_code(s) == 0) == seal_passes, name
        out.append((name, tuple(s), want, seal_passes))

    def good():
        return fec_util.make_set(rng, 6, data_cnt=3)

    add("data_only", fec_util.make_set(rng, 4, data_cnt=4), fec_model.ERR_SET, True)
    add("code_only", fec_util.make_set(rng, 4, data_cnt=0), fec_model.ERR_SET, False)
    s = good()
    s[4] = _edit(s[4], 0x53, "<H", 4)
    add("data_cnt_plus_one", s, fec_model.ERR_SET, False)            # the header's place moves with it: rule 2's
    s = good()
    s[4] = _edit(s[4], 0x53, "<HHH", 2, 3, 2)
    add("data_cnt_minus_one_same_place", s, fec_model.ERR_SET, True)   # 2 + 2 is still place 4: the parity's own rule
    s = good()
    s[5] = _edit(s[5], 0x55, "<H", 4)
    add("code_cnt_plus_one", s, fec_model.ERR_SET, True)
    s = good()
    s[3] = _edit(s[3], 0x55, "<H", 2)
    add("code_cnt_minus_one", s, fec_model.ERR_SET, True)
    s = fec_util.make_set(rng, 6, data_cnt=4)
    s[2] = _edit(s[4], 0x53, "<HHH", 2, 4, 0)
    add("code_between_data", s, fec_model.ERR_SET, True)
    add("data_68_code_1", fec_util.make_set(rng, 69, data_cnt=68), fec_model.ERR_SET, False)
    s = fec_util.make_set(rng, 70, data_cnt=2)
    add("data_2_code_68", s, fec_model.ERR_SET, False)
    # the first failing shred decides
    s = good()
    s[1] = s[1][:1202]
    s[4] = _edit(s[4], 0x53, "<HHH", 2, 3, 2)
    add("parse_then_data_cnt", s, fec_model.ERR_PARSE, False)
    s = good()
    s[3] = _edit(s[3], 0x55, "<H", 2)
    s[5] = s[5][:1227]
    add("code_cnt_then_parse", s, fec_model.ERR_SET, False)
    s = good()
    s[3] = _edit(s[3], 0x55, "<H", 2)
    s[4] = _edit(s[4] + bytes(25), 0x40, "<B", 0x63)
    add("code_cnt_then_unsupported", s, fec_model.ERR_SET, False)
    s = good()
    s[2] = _edit(_edit(s[2], 0x40, "<B", 0x93), 0x56, "<H", 0x58)
    s[3] = _edit(s[3], 0x55, "<H", 2)
    add("unsupported_then_code_cnt", s, fec_model.UNSUPPORTED, False)
    return tuple(out)


def all_bad_sets():
    """[(name, set, code)]: fd_fec_core.h's rule cases, which keep their codes, and the parity's own"""
    old = []
    for name, s, want in fec_util.bad_sets():
        assert rs.parity_code(s) == want, name
        old.append((name, list(s), want))
    return old + [(name, list(s), want) for name, s, want, _ in rule_cases()]


# ---- the device-resident run the GPU test modules share (fd_ed25519_hip_fec_parity_dev) ----

def expect(sets):
    """the model's (code, shreds) per set"""
    return [rs.fill(list(s)) for s in sets]


def run_dev(eng, sets, place, want=None, set_first=None):
    """fd_ed25519_hip_fec_parity_dev on a device-resident buffer of guard
    bytes in which place(i, end of the previous shred) says where shred i
    starts; the whole buffer afterwards must be the same layout of the
    model's shreds: guard bytes, headers, data shreds, signatures and proofs
    unchanged"""
    flat = [s for st in sets for s in st]
    n, n_set = len(flat), len(sets)
    if set_first is None:
        set_first = np.cumsum([0] + [len(s) for s in sets])
    want = expect(sets) if want is None else want
    flat_want = [s for w in want for s in w[1]]
    rng = random.Random(163)
    off, end = [], 0
    for i, s in enumerate(flat):
        off.append(place(i, end))
        assert off[-1] >= end
        end = off[-1] + len(s)
    size = end + 64
    guard = rng.randbytes(size)
    before, after = bytearray(guard), bytearray(guard)
    for o, s, w in zip(off, flat, flat_want):
        before[o:o + len(s)] = s
        after[o:o + len(s)] = w
    d_buf = eng.alloc(size).upload(np.frombuffer(bytes(before), np.uint8))
    d_off = eng.alloc(8 * n + 8).upload(np.array(off + [0], np.uint64))
    d_sz = eng.alloc(4 * n + 4).upload(np.array([len(s) for s in flat] + [0], np.uint32))
    d_first = eng.alloc(4 * (n_set + 1)).upload(np.array(set_first, np.uint32))
    d_out = eng.alloc(n_set + 8).upload(np.full(n_set + 8, 0x55, np.int8))
    eng.fec_parity_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, n_set, d_first.ptr, d_out.ptr)
    eng.sync()
    buf = d_buf.download(np.uint8, size).tobytes()
    out = d_out.download(np.int8, n_set + 8)
    for b in (d_buf, d_off, d_sz, d_first, d_out):
        b.free()
    assert (out[n_set:] == 0x55).all()   # nothing written past the n_set results
    assert out[:n_set].tolist() == [w[0] for w in want]
    if buf != bytes(after):
        at = next(i for i in range(size) if buf[i] != after[i])
        which = max((i for i in range(n) if off[i] <= at), default=-1)
        raise AssertionError(f"byte {at} of the buffer differs: shred {which} starts at {off[which] if which >= 0 else None}")
    return off


def back_to_back(i, end):
    return end + 16 if i == 0 else end
