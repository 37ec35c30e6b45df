"""Builds FEC sets for the seal tests: the reference's captured sets
(tests/golden/shreds.npz) in tree order, sets of any leaf count with headers
that agree inside the set (random payload, parity and junk in the signature
and proof fields), the sets that break one rule of fd_fec_core.h, and seeded
mutations."""
import functools
import random
import struct

import numpy as np

import fec_model as model
from conftest import load_golden
from shred_util import fixture

# every leaf count at which the tree changes shape: one leaf, the powers of
# two and their neighbours (odd layers merge a node with itself), 96 (the
# capture's), 134 (the largest)
SHAPES = (1, 2, 3, 5, 7, 8, 9, 33, 63, 64, 65, 96, 127, 128, 129, 134)


@functools.lru_cache(maxsize=None)
def private_key():
    """the key that signed the capture"""
    return load_golden("fec")["privkey"].tobytes()


@functools.lru_cache(maxsize=None)
def captured_sets():
    """the capture's 7 FEC sets, each its shreds in tree order: the data
    shreds by index, then the code shreds by index"""
    sets = {}
    for s in fixture()[0]:
        fec, = struct.unpack_from("<I", s, 0x4F)
        is_code = s[0x40] & 0xF0 == 0x40
        pos = struct.unpack_from("<H", s, 0x57)[0] if is_code else struct.unpack_from("<I", s, 0x49)[0] - fec
        sets.setdefault(fec, []).append((is_code, pos, s))
    return tuple(tuple(s for _, _, s in sorted(v)) for _, v in sorted(sets.items()))


def blank(shreds):
    """signature and proof fields zeroed"""
    depth, out = model.depth_of(len(shreds)), []
    for s in shreds:
        s, at = bytearray(s), model.proof_at(s, depth)
        s[:64] = bytes(64)
        s[at:at + 20 * depth] = bytes(20 * depth)
        out.append(bytes(s))
    return out


def make_set(rng, cnt, data_cnt=None, fec_set_idx=None, depth=None):
    """cnt filled shreds in tree order, data_cnt of them data shreds (half,
    rounded up, unless given), everything the seal does not write random"""
    if data_cnt is None:
        data_cnt = max((cnt + 1) // 2, cnt - 67)
    code_cnt = cnt - data_cnt
    depth = model.depth_of(cnt) if depth is None else depth
    slot, version = rng.getrandbits(40), rng.getrandbits(16)
    fec = rng.getrandbits(20) if fec_set_idx is None else fec_set_idx
    out = []
    for j in range(cnt):
        data = j < data_cnt
        s = bytearray(rng.getrandbits(8) for _ in range(1203 if data else 1228))
        s[0x40] = (0x80 if data else 0x40) | depth
        if data:
            struct.pack_into("<QIHIHBH", s, 0x41, slot, (fec + j) & 0xFFFFFFFF, version, fec, 1, 0x3F,
                             0x58 + rng.randrange(1203 - 0x58 - 20 * depth + 1))
        else:
            struct.pack_into("<QIHIHHH", s, 0x41, slot, rng.getrandbits(20), version, fec, data_cnt, code_cnt, j - data_cnt)
        out.append(bytes(s))
    return out


def shape_sets(seed=61):
    """one set of every leaf count of SHAPES"""
    rng = random.Random(seed)
    return [make_set(rng, cnt) for cnt in SHAPES]


def _edit(s, at, fmt, *v):
    s = bytearray(s)
    struct.pack_into(fmt, s, at, *v)
    return bytes(s)


def bad_sets(seed=67):
    """[(name, set, the code the rules give)]: a set that breaks one rule,
    or two where the order of the rules shows"""
    rng = random.Random(seed)
    out = []

    def add(name, s, want):
        assert model.set_code(s) == want, (name, model.set_code(s), want)
        out.append((name, s, want))

    def good(cnt=6):
        return make_set(rng, cnt)

    add("cnt_0", [], model.ERR_SET)
    add("cnt_135", make_set(rng, 134) + [make_set(rng, 1)[0]], model.ERR_SET)
    s = good()
    s[2] = _edit(s[2], 0x40, "<B", 0x80 | 2)
    add("depth_nibble_low", s, model.ERR_SET)
    s = good()
    s[4] = _edit(s[4], 0x40, "<B", 0x40 | 4)
    add("depth_nibble_high_code", s, model.ERR_SET)
    add("depth_of_a_larger_set", make_set(rng, 4, depth=3), model.ERR_SET)
    s = good()
    s[1], s[2] = s[2], s[1]
    add("swapped_data", s, model.ERR_SET)
    s = good()
    s[3], s[4] = s[4], s[3]
    add("swapped_code", s, model.ERR_SET)
    s = good()
    s[2], s[3] = s[3], s[2]
    add("code_before_data", s, model.ERR_SET)
    s = good()
    s[2] = s[1]
    add("duplicate_index", s, model.ERR_SET)
    s = good()
    s[0] = _edit(s[0], 0x49, "<I", struct.unpack_from("<I", s[0], 0x4F)[0] - 1)
    add("idx_below_fec_set_idx", s, model.ERR_SET)
    for name, at, v in (("data_cnt_0", 0x53, 0), ("data_cnt_68", 0x53, 68), ("code_cnt_0", 0x55, 0), ("code_cnt_68", 0x55, 68)):
        s = good()
        s[5] = _edit(s[5], at, "<H", v)
        add(name, s, model.ERR_SET)
    for variant in (0x93, 0x63, 0xB3, 0x73, 0xA5, 0x5A):
        s = good()
        s[3] = _edit(s[3] + bytes(25), 0x40, "<B", variant)
        s[3] = _edit(s[3], 0x56, "<H", 0x58 + 100) if variant & 0x80 else s[3]
        add(f"variant_{variant:#x}", s, model.UNSUPPORTED)
    s = good()
    s[3] = _edit(s[3], 0x40, "<B", 0x23)
    add("variant_0x23", s, model.ERR_PARSE)
    s = good()
    s[1] = s[1][:1202]
    add("truncated_data", s, model.ERR_PARSE)
    s = good()
    s[5] = s[5][:1227]
    add("truncated_code", s, model.ERR_PARSE)
    s = good()
    s[0] = s[0][:0x40]
    add("truncated_before_variant", s, model.ERR_PARSE)
    s = good()
    s[2] = _edit(s[2], 0x56, "<H", 1203 - 20 * 3 + 1)
    add("data_size_into_proof", s, model.ERR_PARSE)
    # the first failing shred decides
    s = good()
    s[1] = _edit(_edit(s[1], 0x40, "<B", 0x93), 0x56, "<H", 0x58)   # unsupported
    s[4] = s[4][:1227]                          # parse
    add("unsupported_then_parse", s, model.UNSUPPORTED)
    s = good()
    s[1] = s[1][:1202]
    s[4] = _edit(s[4], 0x40, "<B", 0x63)
    add("parse_then_unsupported", s, model.ERR_PARSE)
    s = good()
    s[0], s[1] = s[1], s[0]                     # set rule at shred 0
    s[2] = s[2][:100]                           # parse at shred 2
    add("set_then_parse", s, model.ERR_SET)
    s = good()
    s[2] = _edit(_edit(s[2], 0x40, "<B", 0x93), 0x56, "<H", 0x58)
    s[3], s[4] = s[4], s[3]
    add("unsupported_then_set", s, model.UNSUPPORTED)
    # inside one shred: parse before unsupported before the set rules
    s = good()
    s[2] = _edit(s[2], 0x40, "<B", 0x95)[:1202]   # chained, wrong depth, wrong place: it does not parse
    s[1], s[2] = s[2], s[1]
    add("one_shred_parse_first", s, model.ERR_PARSE)
    s = good()
    s[2] = _edit(_edit(s[2], 0x40, "<B", 0x95), 0x56, "<H", 0x58)   # chained, wrong depth, wrong place: it parses
    s[1], s[2] = s[2], s[1]
    add("one_shred_unsupported_before_set", s, model.UNSUPPORTED)
    return out


@functools.lru_cache(maxsize=None)
def mutated_sets(count=2000, seed=71):
    """seeded mutations of captured and synthetic sets: a bit flip in one
    shred's header bytes 0x40..0x58, a bit flip anywhere, a variant byte
    replaced, a shred truncated, a shred dropped or doubled"""
    rng = random.Random(seed)
    pool = [list(s) for s in captured_sets()[:2]] + [make_set(rng, c) for c in (1, 2, 3, 5, 9, 17, 33)]
    out = []
    for k in range(count):
        s = list(pool[rng.randrange(len(pool))])
        j = rng.randrange(len(s))
        b, kind = bytearray(s[j]), k % 5
        if kind == 0:
            b[rng.randrange(0x40, 0x59)] ^= 1 << rng.randrange(8)
        elif kind == 1:
            b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
        elif kind == 2:
            b[0x40] = rng.choice([rng.randrange(256), (b[0x40] & 0xF0) | rng.randrange(16), 0x90 | (b[0x40] & 0xF),
                                  0x60 | (b[0x40] & 0xF), 0xA5, 0x5A])
        elif kind == 3:
            del b[rng.randrange(len(b)):]
        s[j] = bytes(b)
        if kind == 4:
            if rng.randrange(2):
                del s[j]
            else:
                s.insert(j, s[j])
        out.append(tuple(s))
    return tuple(out)


# ---- the device-resident run the GPU test modules share (fd_ed25519_hip_fec_seal_dev) ----

def expect(oracle, sets, privs):
    """the model's (code, shreds, root, signature) per set"""
    return [model.seal(oracle, s, None if privs is None else privs[k]) for k, s in enumerate(sets)]


def check_outputs(want, codes, roots, sigs):
    assert codes.tolist() == [w[0] for w in want]
    for k, (code, _, root, sig) in enumerate(want):
        assert roots[k].tobytes() == (root if code == 0 else bytes(32)), k
        if sigs is not None:
            assert sigs[k].tobytes() == (sig if code == 0 else bytes(64)), k


def check_front(eng, want, pubs):
    """every shred of a sealed set passes fd_ed25519_hip_shreds_host under its key"""
    shreds = [s for k, w in enumerate(want) if w[0] == 0 for s in w[1]]
    leaders = [pubs[k] for k, w in enumerate(want) if w[0] == 0 for _ in w[1]]
    codes, _ = eng.shreds_host(shreds, leaders)
    assert len(shreds) and not codes.any(), np.nonzero(codes)[0][:10]


def run_dev(eng, ed, oracle, sets, privs, pubs, place, set_first=None):
    """fd_ed25519_hip_fec_seal_dev on a device-resident buffer of guard bytes
    in which place(i, end of the previous shred) says where shred i starts;
    the whole buffer afterwards must be the same layout of the model's
    shreds: guard bytes before, between and after the shreds unchanged"""
    flat = [s for st in sets for s in st]
    n, n_set = len(flat), len(sets)
    if set_first is None:
        set_first = np.cumsum([0] + [len(s) for s in sets])
    want = expect(oracle, sets, privs)
    flat_want = [s for w in want for s in w[1]]
    rng = random.Random(79)
    off, end = [], 0
    for i, s in enumerate(flat):
        off.append(place(i, end))
        assert off[-1] >= end
        end = off[-1] + len(s)
    size = end + 64
    guard = bytes(rng.getrandbits(8) for _ in range(size))
    before, after = bytearray(guard), bytearray(guard)
    for o, s, w in zip(off, flat, flat_want):
        before[o:o + len(s)] = s
        after[o:o + len(s)] = w
    d_buf = eng.alloc(size).upload(np.frombuffer(bytes(before), np.uint8))
    d_off = eng.alloc(8 * n + 8).upload(np.array(off + [0], np.uint64))
    d_sz = eng.alloc(4 * n + 4).upload(np.array([len(s) for s in flat] + [0], np.uint32))
    d_first = eng.alloc(4 * (n_set + 1)).upload(np.array(set_first, np.uint32))
    d_privs = eng.alloc(32 * n_set).upload(np.frombuffer(b"".join(privs), np.uint8)) if privs is not None else None
    d_work = eng.alloc(ed.fec_work_bytes(n, n_set))
    d_out = eng.alloc(n_set + 8).upload(np.full(n_set + 8, 0x55, np.int8))
    d_roots = eng.alloc(32 * (n_set + 1)).upload(np.full(32 * (n_set + 1), 0x55, np.uint8))
    d_sigs = eng.alloc(64 * (n_set + 1)).upload(np.full(64 * (n_set + 1), 0x55, np.uint8))
    eng.fec_seal_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, n_set, d_first.ptr, d_privs.ptr if privs is not None else None, d_work.ptr,
                     d_out.ptr, d_roots.ptr, d_sigs.ptr if privs is not None else None)
    eng.sync()
    buf = d_buf.download(np.uint8, size).tobytes()
    out = d_out.download(np.int8, n_set + 8)
    roots = d_roots.download(np.uint8, 32 * (n_set + 1))
    sigs = d_sigs.download(np.uint8, 64 * (n_set + 1))
    for b in (d_buf, d_off, d_sz, d_first, d_privs, d_work, d_out, d_roots, d_sigs):
        if b is not None:
            b.free()
    # nothing written past the n_set results, nor into an output that was not given
    assert (out[n_set:] == 0x55).all() and (roots[32 * n_set:] == 0x55).all() and (sigs[64 * n_set:] == 0x55).all()
    if privs is None:
        assert (sigs == 0x55).all()
    check_outputs(want, out[:n_set], roots[:32 * n_set].reshape(n_set, 32),
                  sigs[:64 * n_set].reshape(n_set, 64) if privs is not None else None)
    if buf != bytes(after):
        at = next(i for i in range(size) if buf[i] != after[i])
        which = max((i for i in range(n) if off[i] <= at), default=-1)
        raise AssertionError(f"byte {at} of the buffer differs: shred {which} starts at {off[which] if which >= 0 else None}")
    if privs is not None:
        check_front(eng, want, pubs)
    return want


def back_to_back(i, end):
    return end + 16 if i == 0 else end
