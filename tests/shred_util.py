"""Builds Merkle shreds for the shred tests: synthetic shreds of any
tree_depth, type and index with a valid leader signature (siblings are
picked at random and the walk goes up through them, so depths no real tree
yields are reachable), the rule-edge cases of fd_shred_core.h, and seeded
mutations of the reference's captured shreds (tests/golden/shreds.npz)."""
import functools
import random
import struct

import shred_model as model
from conftest import load_golden
from txn_util import Signer


@functools.lru_cache(maxsize=None)
def fixture():
    """(shreds, leader public key) of the reference's capture"""
    d = load_golden("shreds")
    buf, at, out = d["shreds"].tobytes(), 0, []
    for sz in d["sz"]:
        out.append(buf[at:at + int(sz)])
        at += int(sz)
    return out, d["pubkey"].tobytes()


class Leader:
    def __init__(self, oracle, seed):
        self.sg = Signer(oracle, seed)
        self.priv, self.pub = self.sg.key()
        self.rng = random.Random(seed)

    def shred(self, data, depth, in_type_idx, data_cnt=32, code_cnt=32, fec_set_idx=1000, size=None, variant=None,
              sz=None, sign=True):
        """A shred of the given type (data: True / False), tree_depth and
        index inside its FEC set, every other byte random, signed over the
        root the model derives -- when the model derives one."""
        rng = self.rng
        s = bytearray(rng.getrandbits(8) for _ in range((1203 if data else 1228) if sz is None else sz))
        head = bytearray(0x59)
        head[0x40] = ((0x80 if data else 0x40) | depth) if variant is None else variant
        struct.pack_into("<QIHI", head, 0x41, rng.getrandbits(40), (fec_set_idx + in_type_idx) & 0xFFFFFFFF if data
                         else rng.getrandbits(20), 0x1234, fec_set_idx)
        if data:
            struct.pack_into("<HBH", head, 0x53, 1, 0x3F, 0x58 + rng.randrange(1203 - 0x58 - 20 * depth + 1)
                             if size is None else size)
            head = head[:0x58]
        else:
            struct.pack_into("<HHH", head, 0x53, data_cnt, code_cnt, in_type_idx)
        n = min(len(head), len(s))
        s[0x40:n] = head[0x40:n]
        code, root = model.root(bytes(s))
        if sign and code == model.OK:
            s[:64] = self.sg.sign(root, self.priv, self.pub)
        return bytes(s)


@functools.lru_cache(maxsize=None)
def _rule_cases(oracle):
    ld = Leader(oracle, 41)
    c = []

    def add(name, s, want):
        c.append((name, s, want))

    z = bytearray(ld.shred(True, 6, 3))
    z[:64] = bytes(64)
    add("zero_signature", bytes(z), model.ERR_HEADER)
    for cnt, want in ((0, model.ERR_HEADER), (67, model.OK), (68, model.ERR_HEADER)):
        add(f"data_cnt_{cnt}", ld.shred(False, 8, 0, data_cnt=cnt), want)
        add(f"code_cnt_{cnt}", ld.shred(False, 8, 0, code_cnt=cnt), want)
    for data in (True, False):
        add(f"in_type_idx_66_{'data' if data else 'code'}", ld.shred(data, 8, 66), model.OK)
        add(f"in_type_idx_67_{'data' if data else 'code'}", ld.shred(data, 8, 67), model.ERR_HEADER)
    s = bytearray(ld.shred(True, 6, 0, fec_set_idx=500))
    struct.pack_into("<I", s, 0x49, 499)
    add("idx_below_fec_set_idx", bytes(s), model.ERR_HEADER)
    # shred_idx 0, 1, 2, 64 as data shreds, 133 as the last code shred behind 67 data shreds
    for shred_idx, need in ((0, 0), (1, 1), (2, 2), (64, 7), (133, 8)):
        for depth in (need, need - 1):
            if depth < 0:
                continue
            s = ld.shred(True, depth, shred_idx) if shred_idx < 67 else ld.shred(False, depth, 66, data_cnt=67)
            add(f"shred_idx_{shred_idx}_depth_{depth}", s, model.OK if depth == need else model.ERR_HEADER)
    for data in (True, False):
        add(f"tree_depth_0_{'data' if data else 'code'}", ld.shred(data, 0, 0, data_cnt=1), model.OK if data else model.ERR_HEADER)
        add(f"tree_depth_15_{'data' if data else 'code'}", ld.shred(data, 15, 5), model.OK)
    add("tree_depth_1_code", ld.shred(False, 1, 0, data_cnt=1), model.OK)
    fits = 1203 - 20 * 6
    for size, want in ((0x57, model.ERR_PARSE), (0x58, model.OK), (fits, model.OK), (fits + 1, model.ERR_PARSE)):
        add(f"data_size_{size:#x}", ld.shred(True, 6, 1, size=size), want)
    whole = ld.shred(True, 6, 2)
    add("data_sz_1202", whole[:1202], model.ERR_PARSE)
    add("data_sz_1203", whole, model.OK)
    add("data_sz_1300", whole + bytes(97), model.OK)
    whole = ld.shred(False, 6, 2)
    add("code_sz_1227", whole[:1227], model.ERR_PARSE)
    add("code_sz_1228", whole, model.OK)
    for variant in (0x96, 0x66, 0xB6, 0x76, 0xA5, 0x5A):
        add(f"variant_{variant:#x}", ld.shred(bool(variant & 0x80), 6, 1, size=0x58 + 100, variant=variant, sz=1228),
            model.UNSUPPORTED)
    for variant in (0x00, 0x16, 0x26, 0x36, 0xA4, 0xA6, 0x5B, 0x55, 0xC6, 0xD6, 0xE6, 0xFF):
        add(f"variant_{variant:#x}", ld.shred(bool(variant & 0x80), 6, 1, size=0x58 + 100, variant=variant, sz=1228),
            model.ERR_PARSE)
    assert len({n for n, _, _ in c}) == len(c)
    return tuple(c), ld.pub


def rule_cases(oracle):
    """((name, shred, the code the rule gives), ...), the leader's key"""
    return _rule_cases(oracle)


def every_depth(oracle):
    """a valid shred of every tree_depth 0..15 for both types, the key"""
    ld = Leader(oracle, 43)
    out = []
    for depth in range(16):
        top = min(66, (1 << depth) - 1)
        out.append(ld.shred(True, depth, ld.rng.randrange(top + 1)))
        if depth:   # a code shred sits behind at least one data shred: shred_idx >= 1
            data_cnt = ld.rng.randrange(1, min(67, (1 << depth) - 1) + 1)
            out.append(ld.shred(False, depth, ld.rng.randrange(min(66, (1 << depth) - 1 - data_cnt) + 1), data_cnt=data_cnt))
    return out, ld.pub


@functools.lru_cache(maxsize=None)
def mutated(count=2000, seed=47):
    """seeded mutations of fixture shreds, a quarter each: a bit flip in the
    header bytes 0x40..0x58, a bit flip anywhere, the variant byte replaced,
    a truncation"""
    shreds, _ = fixture()
    rng, out = random.Random(seed), []
    for k in range(count):
        s = bytearray(shreds[rng.randrange(len(shreds))])
        kind = k % 4
        if kind == 0:
            s[rng.randrange(0x40, 0x59)] ^= 1 << rng.randrange(8)
        elif kind == 1:
            s[rng.randrange(len(s))] ^= 1 << rng.randrange(8)
        elif kind == 2:
            s[0x40] = rng.choice([rng.randrange(256), (s[0x40] & 0xF0) | rng.randrange(16), 0x90 | (s[0x40] & 0xF),
                                  0x60 | (s[0x40] & 0xF), 0xB6, 0x76, 0xA5, 0x5A])
        else:
            del s[rng.randrange(len(s)):]
        out.append(bytes(s))
    return tuple(out)
