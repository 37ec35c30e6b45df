"""Builds received FEC sets for the recovery tests: the fixture's cases
(tests/golden/reedsol_recover.npz) carried by real shreds, a set of every
number of data shreds with a seeded mask, the captured sets with a seeded p of
their slots erased, the sets that break one of fd_reedsol_core.h's rules 9-11,
and seeded mutations -- each made once a process and shared, with the model's
answer beside it."""
import functools
import random
import struct

import numpy as np

import fec_util
import recover_model as model
import reedsol_model as rs
import reedsol_util
from conftest import load_golden

# tests/golden/gen_reedsol_recover.py's KINDS
KINDS = ("p_erased", "all_data_erased", "all_parity_erased", "nothing_erased", "partial", "late_flip_d_plus_1",
         "late_flip_all_received", "basis_flip_d_plus_1", "basis_flip_all_received", "target_counts")
AT = 0x20   # where in the protected region the fixture's 32 bytes sit


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("reedsol_recover")


def random_mask(rng, cnt, n_erased):
    m = [0] * cnt
    for j in rng.sample(range(cnt), n_erased):
        m[j] = 1
    return tuple(m)


def fixture_cases():
    """[(kind, d, p, mask, corrupted slot or -1, byte, the reference's return, the slots it recovered)]"""
    g = golden()
    out = []
    for k in range(int(g["cases"])):
        d, p = int(g["d"][k]), int(g["p"][k])
        rec = [g["recovered"][i].tobytes() for i in range(int(g["rec_at"][k]), int(g["rec_at"][k + 1]))]
        out.append((KINDS[int(g["kind"][k])], d, p, tuple(int(x) for x in g["erased"][k][:d + p]), int(g["corrupt"][k]),
                    int(g["corrupt_at"][k]), int(g["ret"][k]), rec))
    return out


def fixture_slots(d, p, mask, bad, at):
    """the 32-byte slots of a fixture case as the reference's decoder got them"""
    g = reedsol_util.golden()
    word = [g["data"][i].tobytes() for i in range(d)] + [g["parity"][d - 1][j].tobytes() for j in range(p)]
    slots = [b"\xA5" * 32 if e else s for s, e in zip(word, mask)]
    if bad >= 0:
        slots[bad] = slots[bad][:at] + bytes([slots[bad][at] ^ 1]) + slots[bad][at + 1:]
    return slots


@functools.lru_cache(maxsize=None)
def _carrier(d, p):
    """a filled set of d + p real shreds whose data shreds carry reedsol.npz's data at AT of their regions"""
    rng = random.Random(211 * d + p)
    g = reedsol_util.golden()
    st = fec_util.make_set(rng, d + p, data_cnt=d)
    st = [s[:0x40 + AT] + g["data"][i].tobytes() + s[0x40 + AT + 32:] if i < d else s for i, s in enumerate(st)]
    code, filled = rs.fill(st)
    assert code == 0
    return tuple(filled)


@functools.lru_cache(maxsize=None)
def fixture_sets():
    """((kind, erased mask, the set as it is received, the model's (code, set after), the reference's return, the
    reference's recovered slots), ...): every fixture case carried by real shreds -- the fixture's bytes at AT of
    every region, the flip AT + byte into the corrupted slot's region"""
    out = []
    for kind, d, p, mask, bad, at, ret, rec in fixture_cases():
        st = list(_carrier(d, p))
        if bad >= 0:
            o = model.region_at(bad, d) + AT + at
            st[bad] = st[bad][:o] + bytes([st[bad][o] ^ 1]) + st[bad][o + 1:]
        st = model.erase(st, mask)
        out.append((kind, mask, tuple(st), model.fill(st, mask), ret, rec))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def every_d():
    """((d, p), ...), (erased mask, ...), (the received set, ...), (the full set, ...): reedsol_util.every_d()'s
    sets with their parity filled and a seeded p of their slots erased and zero-filled"""
    rng = random.Random(223)
    splits, _, full = reedsol_util.every_d()
    masks = tuple(random_mask(rng, d + p, p) for d, p in splits)
    return splits, masks, tuple(tuple(model.erase(s, m)) for s, m in zip(full, masks)), full


def captured(which):
    """[(erased mask, the received set, the capture's set)]: the 7 captured sets with p of their slots zeroed whole
    -- which: "data" (only data shreds; p = d), "parity", "mixed" """
    rng = random.Random({"data": 227, "parity": 229, "mixed": 233}[which])
    out = []
    for st in fec_util.captured_sets():
        cnt = len(st)
        d = cnt // 2
        if which == "data":
            m = (1,) * d + (0,) * d
        elif which == "parity":
            m = (0,) * d + (1,) * d
        else:
            m = random_mask(rng, cnt, d)
        out.append((m, model.erase(st, m), list(st)))
    return out


def _edit(s, at, fmt, *v):
    s = bytearray(s)
    struct.pack_into(fmt, s, at, *v)
    return bytes(s)


def _inconsistent(rng, field):
    """a set of 3 + 3 whose data shred 1 differs from data shred 0 in one header field, its parity computed over
    it: the leader's own set is inconsistent.  With data shred 1 erased it comes back as the leader made it."""
    st = fec_util.make_set(rng, 6, data_cnt=3)
    if field == "slot":
        st[1] = _edit(st[1], 0x41, "<Q", struct.unpack_from("<Q", st[1], 0x41)[0] ^ 1)
    elif field == "version":
        st[1] = _edit(st[1], 0x4D, "<H", struct.unpack_from("<H", st[1], 0x4D)[0] ^ 0x100)
    elif field == "parent_off":
        st[1] = _edit(st[1], 0x53, "<H", 2)
    elif field == "idx":
        st[1] = _edit(st[1], 0x49, "<I", struct.unpack_from("<I", st[1], 0x49)[0] + 1)
    # the parity over the set as it stands: the parity's own rules would not pass an idx out of place
    P = rs.region(6)
    par = rs.encode([s[0x40:0x40 + P] for s in st[:3]], 3)
    return st[:3] + [s[:0x59] + q + s[0x59 + P:] for s, q in zip(st[3:], par)]


@functools.lru_cache(maxsize=None)
def rule_cases():
    """((name, erased mask, the received set, the code the rules give), ...): the sets that break one of rules
    9-11, and the pairs in which the order of the rules shows"""
    rng = random.Random(239)
    out = []

    def add(name, st, mask, want):
        st = model.erase(st, mask)
        got = model.fill(st, mask)
        assert got[0] == want, (name, got[0], want)
        assert want == 0 or got[1] == st, name
        out.append((name, tuple(mask), tuple(st), want))

    def good():
        return rs.fill(fec_util.make_set(rng, 6, data_cnt=3))[1]

    add("good_3_of_6", good(), (1, 0, 1, 0, 1, 0), 0)
    add("no_code_shred_received", good(), (0, 0, 0, 1, 1, 1), model.ERR_SET)
    st = good()
    st[1] = st[1][:1202]
    add("erased_data_slot_too_short", st, (0, 1, 0, 0, 0, 1), model.ERR_PARSE)
    st = good()
    st[4] = st[4][:1227]
    add("erased_code_slot_too_short", st, (0, 1, 0, 0, 1, 0), model.ERR_PARSE)
    st = good()
    st[4] = st[4][:1203]
    add("erased_code_slot_of_a_data_shred_s_size", st, (0, 0, 1, 0, 1, 0), model.ERR_PARSE)
    st = good()
    st[4] = _edit(st[4], 0x53, "<HHH", 4, 3, 0)       # place 4 + 0: rule 2 passes it
    add("data_cnt_plus_one", st, (0, 1, 0, 0, 0, 1), model.ERR_SET)
    st = good()
    st[4] = _edit(st[4], 0x53, "<HHH", 2, 3, 2)       # place 2 + 2
    add("data_cnt_minus_one", st, (0, 1, 0, 0, 0, 1), model.ERR_SET)
    st = good()
    st[3] = _edit(st[3], 0x53, "<HHH", 2, 4, 1)       # the first code shred says d = 2: data shred 2 stands at j >= d
    add("data_shred_at_or_behind_d", st, (0, 1, 0, 0, 1, 1), model.ERR_SET)
    st = good()
    st[5] = _edit(st[5], 0x55, "<H", 4)
    add("code_cnt_plus_one", st, (1, 0, 0, 0, 1, 0), model.ERR_SET)
    add("all_but_one_erased_is_partial", good(), (1, 1, 1, 1, 0, 1), model.ERR_PARTIAL)
    # PARTIAL is a set-level rule: a parse error of any slot, also a later one, comes first ...
    st = good()
    st[5] = st[5][:1227]
    add("partial_against_a_later_parse_error", st, (1, 1, 0, 0, 1, 1), model.ERR_PARSE)
    st = good()
    st[5] = st[5][:1227]
    add("partial_against_a_later_received_parse_error", st, (1, 1, 1, 0, 1, 0), model.ERR_PARSE)
    # ... and so does the missing code shred before PARTIAL
    add("no_code_shred_before_partial", good(), (0, 1, 0, 1, 1, 1), model.ERR_SET)
    # the first failing slot decides, in both directions
    st = good()
    st[1] = st[1][:1202]
    st[4] = _edit(st[4], 0x55, "<H", 4)
    add("erased_parse_then_code_cnt", st, (0, 1, 0, 0, 0, 1), model.ERR_PARSE)
    st = good()
    st[3] = _edit(st[3], 0x55, "<H", 4)
    st[4] = st[4][:1227]
    add("code_cnt_then_erased_parse", st, (0, 1, 0, 0, 1, 0), model.ERR_SET)
    st = good()
    st[0] = _edit(_edit(st[0], 0x40, "<B", 0x93), 0x56, "<H", 0x58)
    st[4] = st[4][:1227]
    add("unsupported_then_erased_parse", st, (0, 1, 0, 0, 1, 0), model.UNSUPPORTED)
    # CORRUPT: a received target beyond the basis, in its first byte, its last byte (the 3-byte column) and a
    # header byte (the slot field of a data shred: a received data shred is always in the basis, so the targets
    # show it)
    P = rs.region(6)
    for name, j, o in (("corrupt_first_byte", 4, 0x59), ("corrupt_last_byte", 4, 0x59 + P - 1),
                       ("corrupt_first_byte_last_slot", 5, 0x59), ("corrupt_byte_of_last_dword", 5, 0x59 + P - 3)):
        st = good()
        st[j] = st[j][:o] + bytes([st[j][o] ^ 0x80]) + st[j][o + 1:]
        add(name, st, (0, 1, 0, 0, 0, 0), model.ERR_CORRUPT)
    st = good()
    st[2] = _edit(st[2], 0x41, "<Q", struct.unpack_from("<Q", st[2], 0x41)[0] ^ 1)
    add("corrupt_header_byte_of_a_basis_data_shred", st, (0, 0, 0, 0, 1, 1), model.ERR_CORRUPT)
    st = good()
    st[5] = st[5][:0x59 + P] + bytes([st[5][0x59 + P] ^ 1]) + st[5][0x59 + P + 1:]
    add("proof_byte_is_not_compared", st, (0, 1, 0, 0, 0, 0), 0)
    # CORRUPT comes before rule 11
    st = _inconsistent(rng, "slot")
    st[5] = st[5][:0x100] + bytes([st[5][0x100] ^ 1]) + st[5][0x101:]
    add("corrupt_before_rule_11", st, (0, 1, 0, 0, 0, 0), model.ERR_CORRUPT)
    # rule 11: the leader's own set is inconsistent, and the recovered data shred shows it
    for field in ("slot", "version", "parent_off", "idx"):
        add("recovered_" + field, _inconsistent(rng, field), (0, 1, 0, 0, 0, 1), model.ERR_SET)
        add("recovered_" + field + "_beside_a_recovered_data_shred_0", _inconsistent(rng, field), (1, 1, 0, 0, 0, 0),
            model.ERR_SET)
    # ... a received one shows it too, and so does a received code shred of another slot number
    add("received_slot_differs", _inconsistent(rng, "slot"), (1, 0, 0, 0, 1, 1), model.ERR_SET)
    st = good()
    st[4] = _edit(st[4], 0x4D, "<H", struct.unpack_from("<H", st[4], 0x4D)[0] ^ 1)
    add("received_code_version_differs", st, (0, 1, 0, 1, 0, 0), model.ERR_SET)   # a code header is outside the region
    st = good()
    st[5] = _edit(st[5], 0x4F, "<I", struct.unpack_from("<I", st[5], 0x4F)[0] ^ 1)
    add("compared_code_fec_set_idx_differs", st, (0, 1, 0, 0, 0, 0), model.ERR_SET)
    return tuple(out)


MUTATION_SEED = 241


@functools.lru_cache(maxsize=None)
def mutated(count=None):
    """((erased mask, the received set, the model's (code, set after)), ...): fec_util.mutated_sets() with their
    parity filled where the parity's rules pass them, then a seeded mask: mostly p or fewer erasures, sometimes
    one more, and every fifth set with one byte of a region flipped"""
    rng = random.Random(MUTATION_SEED)
    out = []
    for k, st in enumerate(fec_util.mutated_sets()[:count]):
        st = list(rs.fill(list(st))[1])
        cnt = len(st)
        d = sum(len(s) > 0x40 and s[0x40] & 0xF0 == 0x80 for s in st)
        n_erased = min(cnt, max(0, cnt - d + rng.choice((0, 0, 0, -1, -2, 1))))
        m = random_mask(rng, cnt, n_erased)
        if k % 5 == 2 and cnt:
            j = rng.randrange(cnt)
            if len(st[j]) >= 1203:
                o = rng.randrange(0x59, 1000)
                st[j] = st[j][:o] + bytes([st[j][o] ^ (1 << rng.randrange(8))]) + st[j][o + 1:]
        st = model.erase(st, m)
        out.append((m, tuple(st), model.fill(st, m)))
    return tuple(out)


def changed_bytes_ok(before, after, mask, d):
    """exactly rule 12's bytes may differ between the received set and the recovered one"""
    P = rs.region(len(before))
    for j, (a, b) in enumerate(zip(before, after)):
        if len(a) != len(b):
            return False
        if not mask[j]:
            if a != b:
                return False
            continue
        keep = [(0x40 + P, len(a))] if j < d else [(0x59 + P, len(a))]
        if any(a[lo:hi] != b[lo:hi] for lo, hi in keep):
            return False
    return True


def flat_npy(sets):
    return np.cumsum([0] + [len(s) for s in sets])


# ---- the device-resident run the GPU test modules share (fd_ed25519_hip_fec_recover_dev) ----

def expect(sets, masks):
    """the model's (code, slots) per set"""
    return [model.fill(list(s), m) for s, m in zip(sets, masks)]


def written_d(st, mask):
    """data_cnt of the set's first received code shred"""
    return next(int.from_bytes(s[0x53:0x55], "little") for s, e in zip(st, mask) if not e and s[0x40] & 0xF0 == 0x40)


def run_dev(eng, sets, masks, place, want=None, set_first=None):
    """fd_ed25519_hip_fec_recover_dev on a device-resident buffer of guard
    bytes in which place(i, end of the previous slot) says where slot i
    starts -- an erased slot is guard bytes too, nothing of it is read --; the
    whole buffer afterwards must be the same layout with exactly the bytes the
    model writes changed: guard bytes, received slots, the proofs and tails of
    erased slots unchanged"""
    flat = [s for st in sets for s in st]
    erased = [int(bool(e)) for m in masks for e in m]
    n, n_set = len(flat), len(sets)
    if set_first is None:
        set_first = np.cumsum([0] + [len(s) for s in sets])
    want = expect(sets, masks) if want is None else want
    rng = random.Random(257)
    off, end = [], 0
    for i, s in enumerate(flat):
        off.append(place(i, end))
        assert off[-1] >= end
        end = off[-1] + len(s)
    size = end + 64
    guard = rng.randbytes(size)
    before, after = bytearray(guard), bytearray(guard)
    i = 0
    for st, mask, (code, filled) in zip(sets, masks, want):
        d = written_d(st, mask) if code == 0 else 0
        P = rs.region(len(st)) if st else 0
        for j, (s, w, e) in enumerate(zip(st, filled, mask)):
            o = off[i]
            i += 1
            if not e:
                assert w == bytes(s)
                before[o:o + len(s)] = s
                after[o:o + len(s)] = s
            elif code == 0:
                # rule 12's bytes of an erased slot over the guard bytes; its proof and tail stay guard bytes
                cut = (0x40 if j < d else 0x59) + P
                after[o:o + 64] = w[:64]
                after[o + 0x40:o + cut] = w[0x40:cut]
    d_buf = eng.alloc(size).upload(np.frombuffer(bytes(before), np.uint8))
    d_off = eng.alloc(8 * n + 8).upload(np.array(off + [0], np.uint64))
    d_sz = eng.alloc(4 * n + 4).upload(np.array([len(s) for s in flat] + [0], np.uint32))
    d_er = eng.alloc(n + 1).upload(np.array(erased + [0], np.uint8))
    d_first = eng.alloc(4 * (n_set + 1)).upload(np.array(set_first, np.uint32))
    d_out = eng.alloc(n_set + 8).upload(np.full(n_set + 8, 0x55, np.int8))
    eng.fec_recover_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, d_er.ptr, n_set, d_first.ptr, d_out.ptr)
    eng.sync()
    buf = d_buf.download(np.uint8, size).tobytes()
    out = d_out.download(np.int8, n_set + 8)
    for b in (d_buf, d_off, d_sz, d_er, d_first, d_out):
        b.free()
    assert (out[n_set:] == 0x55).all()   # nothing written past the n_set results
    assert out[:n_set].tolist() == [w[0] for w in want]
    if buf != bytes(after):
        at = next(i for i in range(size) if buf[i] != after[i])
        which = max((i for i in range(n) if off[i] <= at), default=-1)
        raise AssertionError(f"byte {at} of the buffer differs: slot {which} starts at {off[which] if which >= 0 else None}")
    return off


def back_to_back(i, end):
    return end + 16 if i == 0 else end
