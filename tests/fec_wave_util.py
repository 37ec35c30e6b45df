"""Builds the cases that reach the FEC-set kernels' parallel machinery beyond
lanes 0-15 of wave 0 -- the workgroup reductions, the wave ballots, the row
passes and the column passes of fd_ed25519_fec.hip, fd_ed25519_reedsol.hip and
fd_ed25519_recover.hip -- and the operands of the GF(2^8) diag entry point,
each made once a process with the model's answer beside it.  The conditions
under which a case means what its name says are asserted here, on the CPU,
where the case is built: tests/test_fec_wave_cases.py runs every builder
without a device, the GPU modules (test_gpu_fec_waves.py,
test_gpu_recover_sweep.py, test_gpu_fec_mutations.py, test_gpu_gf256_diag.py)
send what the builders return.

Every expected value is a model's (fec_model, reedsol_model, recover_model,
poh_model), none the library's."""
import functools
import random
import struct

import numpy as np

import fec_model
import fec_util
import poh_model
import poh_util
import recover_model
import recover_util
import reedsol_model as rs

PARSE, UNSUPPORTED, SET = fec_model.ERR_PARSE, fec_model.UNSUPPORTED, fec_model.ERR_SET
CORRUPT = recover_model.ERR_CORRUPT

# the two failing slots lo < hi of a rule-order case: in one wave, in neighbouring lanes of two waves, two waves
# apart, the last lane of the set
PAIRS = ((0, 64), (63, 64), (5, 133), (64, 128), (127, 128), (63, 127))
SPLITS = ((134, 67), (65, 32))     # (cnt, d): three waves of slots, and one lane of a second wave
CODE_PAIRS = ((PARSE, UNSUPPORTED), (UNSUPPORTED, SET), (SET, PARSE))

_edit = fec_util._edit


# ---- the failures a received shred can have (fd_fec_core_judge's: fec_util.bad_sets()'s forms) ----

def cut(s):
    """one byte short: ERR_PARSE"""
    return s[:-1]


def unsupported(s):
    """the chained variant of the shred's own type and depth: UNSUPPORTED"""
    if s[0x40] & 0xF0 == 0x80:
        return _edit(_edit(s, 0x40, "<B", 0x90 | (s[0x40] & 0xF)), 0x56, "<H", 0x58)
    return _edit(s, 0x40, "<B", 0x60 | (s[0x40] & 0xF))


def set_rule(s):
    """the depth nibble of another set size: ERR_SET"""
    return _edit(s, 0x40, "<B", s[0x40] ^ 1)


STAGE_ONE = {PARSE: cut, UNSUPPORTED: unsupported, SET: set_rule}


def pairs_of(cnt):
    return tuple((lo, hi) for lo, hi in PAIRS if hi < cnt)


def _check_order(cases):
    """the conditions of a front's rule-order cases: (lo, hi, the set's code, lo's own code, hi's own code)"""
    assert all(code == lo_code and lo_code != hi_code for _, _, code, lo_code, hi_code in cases)
    assert {c[3] for c in cases} == {c[4] for c in cases} == {PARSE, UNSUPPORTED, SET}
    assert {(lo, hi) for lo, hi, _, _, _ in cases} == set(pairs_of(134)) | set(pairs_of(65))
    assert len(pairs_of(65)) == 2 and len(pairs_of(134)) == 6


@functools.lru_cache(maxsize=None)
def order_sets(front):
    """((lo, hi, set, code), ...) for front "seal" or "parity": a set of 134 or 65 shreds with two broken slots of
    different codes, every pair in both assignments"""
    rng = random.Random({"seal": 331, "parity": 337}[front])
    code_of = fec_model.set_code if front == "seal" else rs.parity_code
    out, seen, k = [], [], 0
    for cnt, d in SPLITS:
        base = fec_util.make_set(rng, cnt, data_cnt=d)
        assert code_of(base) == 0 and fec_model.depth_of(cnt) == (8 if cnt == 134 else 7)
        for lo, hi in pairs_of(cnt):
            x, y = CODE_PAIRS[k % 3]
            k += 1
            for a, b in ((x, y), (y, x)):
                st, only_lo, only_hi = list(base), list(base), list(base)
                st[lo] = only_lo[lo] = STAGE_ONE[a](base[lo])
                st[hi] = only_hi[hi] = STAGE_ONE[b](base[hi])
                assert (code_of(only_lo), code_of(only_hi)) == (a, b)
                seen.append((lo, hi, code_of(st), a, b))
                out.append((lo, hi, tuple(st), code_of(st)))
    _check_order(seen)
    return tuple(out)


def between_good(rng, bad, good):
    """good(), bad[0], good(), bad[1], ..., good()"""
    out = [good()]
    for b in bad:
        out += [b, good()]
    return out


# ---- recovery: the two stages of the judge ----

def _short(st, mask, j, d):
    """slot j erased and one byte too short: ERR_PARSE of fd_reedsol_core_recover_judge"""
    st[j] = st[j][:(1203 if j < d else 1228) - 1]
    mask[j] = 1


def _data_behind_d(st, mask, j, d):
    """a received data shred at place j >= d, which fd_fec_core_judge passes: ERR_SET"""
    assert j >= d
    fec, = struct.unpack_from("<I", st[0], 0x4F)
    st[j] = _edit(st[0], 0x49, "<I", (fec + j) & 0xFFFFFFFF)


def _code_cnt_off(st, mask, j, d):
    """a received code shred whose code_cnt is one off (one below: rule 2 bounds it at 67): ERR_SET"""
    assert j >= d
    p = len(st) - d
    st[j] = _edit(st[j], 0x55, "<H", p - 1 if p > 1 else p + 1)


STAGE_TWO = (("short", _short, PARSE), ("data_behind_d", _data_behind_d, SET), ("code_cnt_off", _code_cnt_off, SET))


def _one(code):
    def apply(st, mask, j, d):
        st[j] = STAGE_ONE[code](st[j])
    return apply


@functools.lru_cache(maxsize=None)
def recover_order_sets():
    """((lo, hi, kind of lo, kind of hi, erased mask, the received set, code), ...): the seal's pairs on received
    sets, and for every pair the two stage mixes -- a failure of fd_fec_core_judge at lo against one of
    fd_reedsol_core_recover_judge at hi, and the reverse"""
    rng = random.Random(347)
    out, seen, k, two_used = [], [], 0, set()
    for cnt, d in SPLITS:
        base = rs.fill(fec_util.make_set(rng, cnt, data_cnt=d))[1]
        base_mask = [0] * cnt
        for j in (1, d + 3):            # two erasures away from every pair and from the first code shred
            base_mask[j] = 1
        assert recover_model.fill(recover_model.erase(base, base_mask), base_mask)[0] == 0

        def add(lo, hi, brk_lo, brk_hi, name_lo, name_hi):
            got = []
            for which in ("both", "lo", "hi"):
                st, mask = list(base), list(base_mask)
                if which != "hi":
                    brk_lo(st, mask, lo, d)
                if which != "lo":
                    brk_hi(st, mask, hi, d)
                st = recover_model.erase(st, mask)
                code, after = recover_model.fill(st, mask)
                assert after == st
                got.append((code, st, mask))
            (code, st, mask), lo_code, hi_code = got[0], got[1][0], got[2][0]
            seen.append((lo, hi, code, lo_code, hi_code))
            out.append((lo, hi, name_lo, name_hi, tuple(mask), tuple(st), code))

        for lo, hi in pairs_of(cnt):
            x, y = CODE_PAIRS[k % 3]
            for a, b in ((x, y), (y, x)):
                add(lo, hi, _one(a), _one(b), "one", "one")
            # the stage mixes: the kinds a slot can have (a slot in front of d only the short erased one), taken in
            # turn, the first whose code differs from the other slot's
            for first_is_one in (True, False):
                two_at = hi if first_is_one else lo
                kinds = [t for t in STAGE_TWO if t[0] == "short" or two_at >= d]
                for q in range(9):
                    one_code = (PARSE, UNSUPPORTED, SET)[(k + q) % 3]
                    name, brk, two_code = kinds[(k + q // 3) % len(kinds)]
                    if one_code != two_code:
                        break
                two_used.add(name)
                if first_is_one:
                    add(lo, hi, _one(one_code), brk, "one", name)
                else:
                    add(lo, hi, brk, _one(one_code), name, "one")
            k += 1
    _check_order(seen)
    assert two_used == {t[0] for t in STAGE_TWO}
    assert {(c[2], c[3]) for c in out} >= {("one", "one"), ("one", "short"), ("short", "one")}
    # both directions of the stage mix occur with the later stage winning and with it losing
    assert any(c[2] != "one" for c in out) and any(c[3] != "one" for c in out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def recover_reductions():
    """((name, erased mask, the received set, the model's (code, set after)), ...): the first received code shred
    in wave 2, that shred failing a set rule, the first received slot in wave 1, and -- when the rules pass it --
    recovered code shreds whose idx wraps below zero"""
    rng = random.Random(349)
    full = rs.fill(fec_util.make_set(rng, 134, data_cnt=67))[1]
    out = []

    def add(name, st, mask, code):
        st = recover_model.erase(st, mask)
        want = recover_model.fill(st, mask)
        assert want[0] == code, (name, want[0])
        assert code == 0 or want[1] == st
        out.append((name, tuple(mask), tuple(st), want))
        return want

    m = [0] * 67 + [1] * 61 + [0] * 6
    assert [j for j in range(67, 134) if not m[j]] == list(range(128, 134))
    w = add("code_shreds_from_128", list(full), m, 0)
    P = rs.region(134)
    assert all(w[1][j][0x59:0x59 + P] == full[j][0x59:0x59 + P] for j in range(67, 128))
    # slot 128 fails a set rule: the first code shred the rules pass is 129, and the set has slot 128's code
    st = list(full)
    st[128] = set_rule(st[128])
    add("first_code_shred_fails_a_set_rule", st, m, SET)
    m = [1] * 67 + [0] * 67
    w = add("all_data_erased", list(full), m, 0)
    assert all(s[:64] == full[67][:64] for s in w[1][:67]) and full[67][:64] != full[0][:64]
    # the wrap: the first received code shred, at code position 5, has idx 2; the recovered code shreds 0..2 get
    # idx 2 - 5 + i mod 2^32.  fd_fec_core.h's rule 2 does not read a code shred's idx, so the rules pass the set
    st = list(full)
    st[72] = _edit(st[72], 0x49, "<I", 2)
    m = [0] * 67 + [1] * 5 + [0] * 62
    w = recover_model.fill(recover_model.erase(st, m), m)
    if w[0] == 0:
        w = add("code_idx_wraps_below_zero", st, m, 0)
        assert [struct.unpack_from("<I", w[1][67 + i], 0x49)[0] for i in range(5)] == [0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF, 0, 1]
    return tuple(out)


# ---- the corruption sweep through the compare phase ----

SWEEP_ROWS = (0, 7, 8, 31, 32, 39, 63, 64, 66)
SWEEP_BYTES = (0, 255, 256, 511, 512, 767, 768, 995, 996, 998)
COL2_BYTES = (1023, 1024, 1055, 1056, 1058)
BASIS_BYTES = (4, 260, 516, 772)


def _flip(st, slot, at, bit):
    st = list(st)
    st[slot] = st[slot][:at] + bytes([st[slot][at] ^ (1 << bit)]) + st[slot][at + 1:]
    return st


def geometry(cnt, mask, d):
    """(region bytes, 4-byte columns, compared rows, the compared rows' slots) of a received set"""
    rcvd = [j for j in range(cnt) if not mask[j]]
    P = rs.region(cnt)
    return P, (P + 3) // 4, len(rcvd) - d, rcvd[d:]


@functools.lru_cache(maxsize=None)
def sweep_grid():
    """((row, region byte or None for the proof byte, bit, erased mask, set, code), ...): 2 + 67 with nothing
    erased, one bit flipped in a compared row -- the 90 sets of SWEEP_ROWS x SWEEP_BYTES, then the first proof
    byte of rows 0, 32 and 66"""
    rng = random.Random(353)
    full = rs.fill(fec_util.make_set(rng, 69, data_cnt=2))[1]
    mask = (0,) * 69
    P, ncol, ncmp, rows = geometry(69, mask, 2)
    assert (fec_model.depth_of(69), P, ncol, ncmp) == (7, 999, 250, 67) and rows == list(range(2, 69))
    assert [min(32, ncmp - r0) for r0 in range(0, ncmp, 32)] == [32, 32, 3]
    out = []
    for r in SWEEP_ROWS:
        for b in SWEEP_BYTES:
            out.append((r, b, len(out) % 8, mask, tuple(_flip(full, rows[r], 0x59 + b, len(out) % 8)), CORRUPT))
    for r in (0, 32, 66):
        out.append((r, None, len(out) % 8, mask, tuple(_flip(full, rows[r], 0x59 + P, len(out) % 8)), 0))
    for r, b, bit, mask, st, code in out:
        want = recover_model.fill(list(st), mask)
        assert want[0] == code and want[1] == list(st)     # nothing erased: nothing written either way
    assert {(r, b) for r, b, *_ in out[:90]} == {(r, b) for r in SWEEP_ROWS for b in SWEEP_BYTES} and len(out) == 93
    assert {c[2] for c in out[:90]} == set(range(8))
    # the three passes of 32 rows, the first and last row of a pass and of a group of eight; every wave of columns
    # (64 columns of 4 bytes), the first and last byte of each, and the three-byte last column
    assert {r // 32 for r in SWEEP_ROWS} == {0, 1, 2} and {b // 256 for b in SWEEP_BYTES} == {0, 1, 2, 3}
    assert 998 // 4 == ncol - 1 and 995 // 4 == ncol - 2
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sweep_rest():
    """((name, erased mask, the received set, code), ...): the shared group of eight, the second column pass and
    the basis flips, with the unflipped sets that are recovered"""
    rng = random.Random(359)
    out = []

    def add(name, st, mask, code):
        st = recover_model.erase(st, mask)
        want = recover_model.fill(st, mask)
        assert want[0] == code, (name, want[0])
        assert code == 0 or want[1] == st
        out.append((name, tuple(mask), tuple(st), code))

    # 2 + 67, the last 30 parity slots erased: 37 compared rows, the erased rows 37..39 in the last compared group
    full = rs.fill(fec_util.make_set(rng, 69, data_cnt=2))[1]
    mask = (0,) * 39 + (1,) * 30
    P, ncol, ncmp, rows = geometry(69, mask, 2)
    assert (P, ncol, ncmp) == (999, 250, 37) and rows == list(range(2, 39)) and ncmp % 8 == 5 and ncmp // 8 * 8 == 32
    add("group_unflipped", full, mask, 0)
    add("group_row_32_byte_300", _flip(full, rows[32], 0x59 + 300, 3), mask, CORRUPT)
    add("group_row_36_byte_998", _flip(full, rows[36], 0x59 + 998, 6), mask, CORRUPT)
    # 8 + 8, the last parity slot erased: 265 columns, 256..264 on a second column pass
    full = rs.fill(fec_util.make_set(rng, 16, data_cnt=8))[1]
    mask = (0,) * 15 + (1,)
    P, ncol, ncmp, rows = geometry(16, mask, 8)
    assert (fec_model.depth_of(16), P, ncol, ncmp) == (4, 1059, 265, 7) and rows == list(range(8, 15)) and ncol > 256
    assert all(b // 4 >= 255 for b in COL2_BYTES) and {b // 4 for b in COL2_BYTES} >= {255, 256, 263, 264}
    add("col2_unflipped", full, mask, 0)
    for k, b in enumerate(COL2_BYTES):
        add(f"col2_row_3_byte_{b}", _flip(full, rows[3], 0x59 + b, (k + 1) % 8), mask, CORRUPT)
        add(f"col2_basis_5_byte_{b}", _flip(full, 5, 0x40 + b, (k + 4) % 8), mask, CORRUPT)
    add("col2_row_3_proof_byte", _flip(full, rows[3], 0x59 + P, 7), mask, 0)
    # 67 + 67, nothing erased: one flip in a basis slot per wave of columns
    full = rs.fill(fec_util.make_set(rng, 134, data_cnt=67))[1]
    mask = (0,) * 134
    P, ncol, ncmp, rows = geometry(134, mask, 67)
    assert (P, ncol, ncmp) == (979, 245, 67) and [b // 4 // 64 for b in BASIS_BYTES] == [0, 1, 2, 3]
    for k, b in enumerate(BASIS_BYTES):
        add(f"basis_{13 * k + 2}_byte_{b}", _flip(full, 13 * k + 2, 0x40 + b, (2 * k + 1) % 8), mask, CORRUPT)
    return tuple(out)


# ---- the seeded mutations ----

MUTATION_COUNTS = {     # the model's codes over the first 600 mutated sets
    "seal": {0: 194, PARSE: 196, UNSUPPORTED: 40, SET: 170},
    "parity": {0: 172, PARSE: 196, UNSUPPORTED: 40, SET: 192},
    "recover": {0: 114, PARSE: 160, UNSUPPORTED: 22, SET: 260, recover_model.ERR_PARTIAL: 35, CORRUPT: 9},
}


def count(codes):
    return {c: codes.count(c) for c in set(codes)}


def mutated_sets():
    return fec_util.mutated_sets()[:600]


@functools.lru_cache(maxsize=None)
def mutated_codes(front):
    """the model's code of each of the first 600 mutated sets; every class of MUTATION_COUNTS occurs"""
    if front == "seal":
        codes = [fec_model.set_code(s) for s in mutated_sets()]
    elif front == "parity":
        codes = [rs.parity_code(s) for s in mutated_sets()]
    else:
        codes = [want[0] for _, _, want in recover_util.mutated(600)]
    assert len(codes) == 600 and count(codes) == MUTATION_COUNTS[front], count(codes)
    assert any(len(s) == 0 for s in mutated_sets()) and any(len(s) == 65 for s in mutated_sets())
    return tuple(codes)


@functools.lru_cache(maxsize=None)
def mutated_blocks(hash_cnt_max=4096):
    """(blocks, in states, the model's codes, first bad microblocks, last hashes) of poh_util.mutated(400) under
    hash_cnt_max: blocks that walk and blocks that do not, and a walked one with a hash mismatch"""
    blocks = poh_util.mutated(400)
    ins = [bytes(32)] * len(blocks)
    codes, bad, last, walked = [], [], [], 0
    for blk, st in zip(blocks, ins):
        w = poh_model.walk(blk)
        if w[0] or not w[1]:
            codes.append(poh_model.ERR_PARSE); bad.append(0xFFFFFFFF); last.append(bytes(32))
            continue
        walked += 1
        d = poh_util.describe(blk, st)
        code, first_bad = poh_model.reduce_block(d.want(hash_cnt_max)[0].tolist())
        codes.append(code); bad.append(first_bad)
        last.append(d.buf[int(d.hdr_off[-1]) + 8:int(d.hdr_off[-1]) + 40])
    assert 0 < walked < len(blocks) and poh_model.ERR_HASH in codes and poh_model.ERR_PARSE in codes
    return tuple(blocks), tuple(ins), tuple(codes), tuple(bad), tuple(last)


# ---- the GF(2^8) product and the coefficient build ----

def product_rows():
    """(c, x, c x) as uint32 arrays of 65,536: every (c, v) with v in each of the four byte lanes once, the other
    three lanes holding v + 85, v + 170 and v + 255 mod 256 in turn"""
    c = np.repeat(np.arange(256, dtype=np.uint32), 256)
    v = np.tile(np.arange(256, dtype=np.uint32), 256)
    lanes = [(v + 85 * k) & 0xFF for k in range(4)]
    x = lanes[0] | lanes[1] << 8 | lanes[2] << 16 | lanes[3] << 24
    table = np.array([[rs.mul(a, b) for b in range(256)] for a in range(256)], np.uint32)
    want = table[c, lanes[0]] | table[c, lanes[1]] << 8 | table[c, lanes[2]] << 16 | table[c, lanes[3]] << 24
    for k in range(4):
        assert {(int(a), int(b)) for a, b in zip(c, lanes[k])} == {(a, b) for a in range(256) for b in range(256)}
    assert all(len({int(l[i]) for l in lanes}) == 4 for i in range(0, 65536, 257))
    return c, x.astype(np.uint32), want.astype(np.uint32)


COEF_D = (1, 2, 3, 4, 5, 63, 64, 65, 66, 67)
COEF_CNT = 134


@functools.lru_cache(maxsize=None)
def coef_cases():
    """((basis, targets, the coefficients L[e][r] as field elements, uint8 [targets][d]), ...): for every d of COEF_D
    the first d slots of 134, the last d, every other slot and two seeded choices"""
    rng = random.Random(367)
    exp = np.array(rs.EXP[:255], np.uint8)
    out, seen = [], set()
    for d in COEF_D:
        for basis in (range(d), range(COEF_CNT - d, COEF_CNT), range(0, 2 * d, 2), sorted(rng.sample(range(COEF_CNT), d)),
                      sorted(rng.sample(range(COEF_CNT), d))):
            basis = tuple(basis)
            targets = tuple(e for e in range(COEF_CNT) if e not in basis)
            want = exp[recover_model.lagrange(basis, targets)]
            assert want.shape == (COEF_CNT - d, d) and len(basis) == d and max(basis) < COEF_CNT
            seen |= set(want.flatten().tolist())
            out.append((basis, targets, want))
    assert seen == set(range(1, 256)) and len(out) == 50
    return tuple(out)
