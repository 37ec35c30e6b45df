"""Test-side model of the recovery of a received FEC set (what
fd_reedsol_recover_fini gives fd_fec_resolver_add_shred and what the resolver
does with it, src/disco/shred/fd_fec_resolver.c:474-572), written from the
formula and the rules 9-12 of fd_reedsol_core.h's header comment and not from
the library.  The field is reedsol_model's.

  basis R = the first d received slots in set order; for every other slot e
  v_e[b]  = sum_{r in R} L[e][r] v_r[b]
  L[e][r] = prod_{m in R, m != r} (e ^ m) / (r ^ m)      (= N_e / ((e ^ r) D_r))"""
import struct

import numpy as np

import fec_model
import reedsol_model as rs

OK, ERR_PARSE, UNSUPPORTED, ERR_SET = fec_model.OK, fec_model.ERR_PARSE, fec_model.UNSUPPORTED, fec_model.ERR_SET
ERR_PARTIAL, ERR_CORRUPT = -23, -24
# fd_reedsol.h:41-43
REF_CODES = {0: OK, -1: ERR_CORRUPT, -2: ERR_PARTIAL}


_LOG = np.array(rs.LOG, np.int64)
_EXP = np.array(rs.EXP[:255], np.uint8)


def lagrange(basis, targets):
    """L[e][r] for e in targets, r in basis, as logarithms: log N_e - log(e ^ r) - log D_r mod 255"""
    b, e = np.array(basis, np.int64), np.array(targets, np.int64)
    log_d = _LOG[b[:, None] ^ b[None, :]].sum(1)                 # LOG[0] is 0: the factor m == r drops out
    log_n = _LOG[e[:, None] ^ b[None, :]].sum(1)
    return (log_n[:, None] - _LOG[e[:, None] ^ b[None, :]] - log_d[None, :]) % 255


def evaluate(basis, regions, targets):
    """the regions of the target slots from the basis slots' equal-length regions"""
    log_l = lagrange(basis, targets)
    acc = np.zeros((len(targets), len(regions[0])), np.uint8)
    for i, x in enumerate(regions):
        x = np.frombuffer(bytes(x), np.uint8)
        prod = _EXP[(log_l[:, i][:, None] + _LOG[x][None, :]) % 255]
        prod[:, x == 0] = 0
        acc ^= prod
    return [a.tobytes() for a in acc]


def recover(slots, erased, d):
    """fd_reedsol_recover_fini on equal-length byte strings, d of them data:
    (code, the slots after it) -- an erased slot regenerated when the code is
    0, everything as it came otherwise"""
    rcvd = [j for j in range(len(slots)) if not erased[j]]
    if len(rcvd) < d:
        return ERR_PARTIAL, [bytes(s) for s in slots]
    basis = rcvd[:d]
    targets = [e for e in range(len(slots)) if e not in basis]
    out = [bytes(s) for s in slots]
    for e, v in zip(targets, evaluate(basis, [slots[r] for r in basis], targets)):
        if erased[e]:
            out[e] = v
        elif v != bytes(slots[e]):
            return ERR_CORRUPT, [bytes(s) for s in slots]
    return OK, out


def region_at(j, d):
    return 0x40 if j < d else 0x59


def _agree(h, h0, is_data):
    """slot, version, fec_set_idx and, of a data shred, parent_off: offsets from 0x40"""
    fields = [(0x01, 8), (0x0D, 2), (0x0F, 4)] + ([(0x13, 2)] if is_data else [])
    return all(h[a:a + n] == h0[a:a + n] for a, n in fields)


def fill(shreds, erased):
    """(code, the slots as the recovery leaves them): rules 9-12"""
    same = [bytes(s) for s in shreds]
    cnt = len(shreds)
    if cnt == 0 or cnt > fec_model.CNT_MAX:
        return ERR_SET, same
    # rule 9: d is the data_cnt of the first received code shred the seal's rules pass
    d, first_code = cnt, None
    for j, s in enumerate(shreds):
        if not erased[j] and fec_model.shred_code(s, cnt, j) == 0 and s[0x40] & 0xF0 == 0x40:
            d, first_code = struct.unpack_from("<H", s, 0x53)[0], j
            break
    for j, s in enumerate(shreds):
        if erased[j]:
            if len(s) < (1203 if j < d else 1228):
                return ERR_PARSE, same
            continue
        code = fec_model.shred_code(s, cnt, j)
        if code:
            return code, same
        if s[0x40] & 0xF0 == 0x80:
            if j >= d:
                return ERR_SET, same
        elif struct.unpack_from("<HH", s, 0x53) != (d, cnt - d):
            return ERR_SET, same
    # rule 10
    if first_code is None:
        return ERR_SET, same
    P = rs.region(cnt)
    regions = [bytes(s[region_at(j, d):region_at(j, d) + P]) for j, s in enumerate(shreds)]
    code, after = recover(regions, erased, d)
    if code:
        return code, same
    # rule 11
    depth = fec_model.depth_of(cnt)
    for j in range(d):
        if erased[j] and fec_model.shred_code(bytes(0x40) + after[j] + bytes(20 * depth), cnt, j):
            return ERR_SET, same
        if not _agree(after[j], after[0], True):
            return ERR_SET, same
    for j in range(d, cnt):
        if not erased[j] and not _agree(shreds[j][0x40:], after[0], False):
            return ERR_SET, same
    # rule 12
    sig = bytes(shreds[min(j for j in range(cnt) if not erased[j])][:64])
    ref = shreds[first_code]
    slot, idx, version, fec = struct.unpack_from("<QIHI", ref, 0x41)
    idx0 = (idx - struct.unpack_from("<H", ref, 0x57)[0]) & 0xFFFFFFFF
    out = []
    for j, s in enumerate(shreds):
        if not erased[j]:
            out.append(bytes(s))
        elif j < d:
            out.append(sig + after[j] + bytes(s[0x40 + P:]))
        else:
            i = j - d
            hdr = struct.pack("<BQIHIHHH", 0x40 | depth, slot, (idx0 + i) & 0xFFFFFFFF, version, fec, d, cnt - d, i)
            out.append(sig + hdr + after[j] + bytes(s[0x59 + P:]))
    return OK, out


def erase(shreds, erased):
    """the erased slots zero-filled, their sizes kept"""
    return [bytes(len(s)) if e else bytes(s) for s, e in zip(shreds, erased)]
