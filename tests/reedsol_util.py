"""Builds FEC sets for the parity tests: one set of every number of data shreds
with the parity count the reference's shredder gives it
(tests/golden/reedsol.npz records the shredder's table), the extremes, and the
sets that break one of fd_reedsol_core.h's rules -- each made once a process
and shared, with the model's answer beside it."""
import functools
import random
import struct

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
