"""Test-side model of the reference's Ed25519 precompile
(fd_precompile_ed25519_verify, src/flamenco/runtime/program/fd_precompiles.c:
72-109, 115-200) over one raw transaction: the instruction table is the
reference parser's own fd_txn_t (txn_util.ref_parse_raw), every entry is
verified by the reference's compiled fd_ed25519_verify (fdref_verify).  The
reference function itself needs the runtime's instruction context, so its
rules are applied here, written from the rules and not from the library."""
import ctypes
import struct

from txn_util import ref_parse_raw

B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"
_n = 0
for _c in "Ed25519SigVerify111111111111111111111111111":
    _n = _n * 58 + B58.index(_c)
ED25519_ID = _n.to_bytes(32, "big")
ERR_SIGNATURE, ERR_DATA_OFFSET, ERR_INSTR_DATA_SIZE, PARSE_FAILED, BAD_RESERVATION = -3, -4, -5, -16, -17


def walk(ref, payload):
    """None for a payload the reference parser rejects, else (entries,
    hdr_instr): entries (instr, sig_off, pub_off, msg_off, msg_sz, pre) of
    every precompile instruction whose header passes, hdr_instr the first
    one whose header fails (0xFF: none)."""
    raw = ref_parse_raw(ref, payload)
    if raw is None:
        return None
    acct_off, instr_cnt = struct.unpack_from("<H", raw, 10)[0], struct.unpack_from("<H", raw, 18)[0]
    ins = [struct.unpack_from("<BxHHHH", raw, 20 + 10 * j) for j in range(instr_cnt)]   # prog, acct_cnt, data_sz, acct_off, data_off
    ents, hdr_instr = [], 0xFF
    for j, (prog, _, dsz, _, doff) in enumerate(ins):
        if payload[acct_off + 32 * prog:acct_off + 32 * prog + 32] != ED25519_ID:
            continue
        data = payload[doff:doff + dsz]
        if dsz < 16:
            ok, cnt = dsz == 2 and data[0] == 0, 0
        else:
            cnt = data[0]
            ok = cnt != 0 and dsz >= 2 + 14 * cnt
        if not ok:
            hdr_instr = j if hdr_instr == 0xFF else hdr_instr
            continue
        for i in range(cnt):
            so, si, po, pi, mo, msz, mi = struct.unpack_from("<7H", data, 2 + 14 * i)
            at = []
            for idx, off, size in ((si, so, 64), (pi, po, 32), (mi, mo, msz)):
                idx = j if idx == 0xFFFF else idx
                at.append(ins[idx][4] + off if idx < instr_cnt and off + size <= ins[idx][2] else None)
            ents.append((j, at[0], at[1], at[2], msz, 0) if None not in at else (j, 0, 0, 0, 0, ERR_DATA_OFFSET))
    return ents, hdr_instr


def judge(ref, payload):
    """(transaction code, failing instruction or 0xFF, per-entry codes)"""
    w = walk(ref, payload)
    if w is None:
        return PARSE_FAILED, 0xFF, []
    ref.fdref_verify.argtypes = [ctypes.c_char_p, ctypes.c_ulong, ctypes.c_char_p, ctypes.c_char_p]
    ents, hdr_instr = w
    codes = [pre or (ERR_SIGNATURE if ref.fdref_verify(payload[m:m + msz], msz, payload[s:s + 64], payload[k:k + 32]) else 0)
             for _, s, k, m, msz, pre in ents]
    # instruction order; a failing header is judged after the entries of the instructions before it
    events = [(e[0], 1, c) for e, c in zip(ents, codes) if c]
    if hdr_instr != 0xFF:
        events.append((hdr_instr, 0, ERR_INSTR_DATA_SIZE))
    first = min(events, key=lambda ev: ev[0], default=None)   # stable: entry order within an instruction
    return (first[2], first[0], codes) if first else (0, 0xFF, codes)
