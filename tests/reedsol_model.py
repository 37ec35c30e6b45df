"""Test-side model of the Reed-Solomon parity of a FEC set (what
fd_reedsol_encode_fini gives fd_shredder_next_fec_set,
src/disco/shred/fd_shredder.c:167-223): log and exp tables of GF(2^8) over
0x11D and the Lagrange product formula, written from the rules of
fd_reedsol_core.h's header comment and not from the library.

  parity_j[b] = sum_i M_d[j][i] data_i[b]
  M_d[j][i]   = prod_{m != i, m < d} ((d+j) ^ m) / (i ^ m)"""
import functools
import struct

import numpy as np

import fec_model

EXP = [0] * 510
LOG = [0] * 256
_x = 1
for _k in range(255):
    EXP[_k] = EXP[_k + 255] = _x
    LOG[_x] = _k
    _x <<= 1
    if _x & 0x100:
        _x ^= 0x11D

# MUL[c] is the 256-entry table of products with c
_EXP, _LOG = np.array(EXP, np.uint8), np.array(LOG, np.int64)


@functools.lru_cache(maxsize=None)
def _mul_table(c):
    t = _EXP[_LOG + LOG[c]]
    t[0] = 0
    return t if c else np.zeros(256, np.uint8)


def mul(a, b):
    return EXP[LOG[a] + LOG[b]] if a and b else 0


def inv(a):
    return EXP[255 - LOG[a]]


@functools.lru_cache(maxsize=None)
def row(d, j):
    """M_d[j]"""
    out = []
    for i in range(d):
        c = 1
        for m in range(d):
            if m != i:
                c = mul(c, mul((d + j) ^ m, inv(i ^ m)))
        out.append(c)
    return tuple(out)


def encode(data, p):
    """the p parity rows of the equal-length byte strings data"""
    d = len(data)
    arr = [np.frombuffer(bytes(x), np.uint8) for x in data]
    out = []
    for j in range(p):
        acc = np.zeros(len(arr[0]), np.uint8)
        for c, x in zip(row(d, j), arr):
            acc ^= _mul_table(c)[x]
        out.append(acc.tobytes())
    return out


def region(cnt):
    """P: the protected bytes of a shred in a set of cnt shreds"""
    return 1139 - 20 * fec_model.depth_of(cnt)


def parity_code(shreds):
    """fec_model.set_code, then shred by shred in set order the first of: a
    data shred behind a code shred, a 68th data shred, a data shred as the
    set's last, a code shred at place 0, a code shred whose data_cnt or
    code_cnt is not the set's split -- ERR_SET; a shred fec_model's rule 2
    fails decides before any shred behind it"""
    cnt = len(shreds)
    if cnt == 0 or cnt > fec_model.CNT_MAX:
        return fec_model.ERR_SET
    d = None
    for j, s in enumerate(shreds):
        code = fec_model.shred_code(s, cnt, j)
        if code:
            return code
        if s[0x40] & 0xF0 == 0x80:
            if d is not None or j >= 67 or j == cnt - 1:
                return fec_model.ERR_SET
        else:
            if d is None:
                d = j
            data_cnt, code_cnt = struct.unpack_from("<HH", s, 0x53)
            if d == 0 or data_cnt != d or code_cnt != cnt - d:
                return fec_model.ERR_SET
    return fec_model.OK


def fill(shreds):
    """(code, the shreds as the parity leaves them): bytes [0x59, 0x59+P) of
    every code shred of a set with code 0, nothing otherwise"""
    code = parity_code(shreds)
    if code:
        return code, [bytes(s) for s in shreds]
    cnt = len(shreds)
    d = sum(s[0x40] & 0xF0 == 0x80 for s in shreds)
    P = region(cnt)
    par = encode([s[0x40:0x40 + P] for s in shreds[:d]], cnt - d)
    return 0, [bytes(s) for s in shreds[:d]] + [bytes(s[:0x59]) + q + bytes(s[0x59 + P:]) for s, q in zip(shreds[d:], par)]


def blank_parity(shreds):
    """the parity regions of a set's code shreds zeroed"""
    P = region(len(shreds))
    return [bytes(s) if s[0x40] & 0xF0 == 0x80 else bytes(s[:0x59]) + bytes(P) + bytes(s[0x59 + P:]) for s in shreds]
