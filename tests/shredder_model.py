"""Test-side model of the front of the leader's shred path (what
fd_shredder_init_batch and fd_shredder_next_fec_set,
src/disco/shred/fd_shredder.c:145-221, do to an entry batch, with the
fd_shredder_count_* arithmetic): the counts, the plan of every set, the data
shreds and the parity headers, on top of reedsol_model (the parity) and
fec_model (the seal).  Written from the rules of fd_shredder_core.h's header
comment and not from the library."""
import hashlib
import random
import struct

import fec_model
import reedsol_model as rs

OK, ERR_BATCH, BAD_RESERVATION = 0, -19, -17
SET_BYTES = 31840

# parity shreds of a set of d <= 32 data shreds: protocol constants
PARITY = (0, 17, 18, 19, 19, 20, 21, 21, 22, 23, 23, 24, 24, 25, 25, 26, 26,
          26, 27, 27, 28, 28, 29, 29, 29, 30, 30, 31, 31, 31, 32, 32, 32)


def split(r):
    """(d, p) of a batch's last set of r bytes"""
    assert 1 <= r <= 2 * SET_BYTES - 1
    if r <= 9135:
        d = max(1, -(-r // 1015))
        return d, PARITY[d]
    if r <= 31840:
        d = -(-r // 995)
        return d, PARITY[d]
    d = -(-r // 975) if r <= 62400 else -(-r // 955)
    return d, d


def count(sz):
    """(sets, data shreds, parity shreds) of a batch of sz bytes"""
    if sz == 0:
        return 0, 0, 0
    sets = max(sz, 2 * SET_BYTES - 1) // SET_BYTES
    d, p = split(sz - (sets - 1) * SET_BYTES)
    return sets, 32 * (sets - 1) + d, 32 * (sets - 1) + p


def plan(sz):
    """[(offset, bytes, d, p, depth, payload)] of the sets of a batch"""
    sets = count(sz)[0]
    out = []
    for q in range(sets):
        off = q * SET_BYTES
        size = SET_BYTES if q + 1 < sets else sz - off
        d, p = (32, 32) if q + 1 < sets else split(size)
        depth = fec_model.depth_of(d + p)
        payload = 1115 - 20 * depth
        assert (d - 1) * payload < size <= d * payload
        out.append((off, size, d, p, depth, payload))
    return out


def desc(slot=0, data_idx=0, parity_idx=0, version=0, parent_off=0, reference_tick=0, block_complete=0):
    return dict(slot=slot, data_idx=data_idx, parity_idx=parity_idx, version=version, parent_off=parent_off,
                reference_tick=reference_tick, block_complete=block_complete)


def front(batch, dsc):
    """the sets of a batch as the front leaves them, each the list of its
    shreds in tree order: data shreds whole with zero signature and proof,
    parity shreds with their header, a zero parity region and a zero proof"""
    batch = bytes(batch)
    D, C, sets = dsc["data_idx"], dsc["parity_idx"], []
    plans = plan(len(batch))
    for q, (off, size, d, p, depth, payload) in enumerate(plans):
        last = q + 1 == len(plans)
        shreds = []
        for i in range(d):
            body = batch[off + i * payload:off + min(size, (i + 1) * payload)]
            flags = dsc["reference_tick"] & 0x3F
            if i == d - 1 and last:
                flags |= 0x40 | ((dsc["block_complete"] & 1) << 7)
            hdr = struct.pack("<BQIHIHBH", 0x80 | depth, dsc["slot"], (D + i) & 0xFFFFFFFF, dsc["version"] & 0xFFFF, D & 0xFFFFFFFF,
                              dsc["parent_off"] & 0xFFFF, flags, 0x58 + len(body))
            s = bytes(64) + hdr + body
            shreds.append(s + bytes(1203 - len(s)))
        for j in range(p):
            hdr = struct.pack("<BQIHIHHH", 0x40 | depth, dsc["slot"], (C + j) & 0xFFFFFFFF, dsc["version"] & 0xFFFF, D & 0xFFFFFFFF,
                              d, p, j)
            s = bytes(64) + hdr
            shreds.append(s + bytes(1228 - len(s)))
        assert all(len(s) == 1203 for s in shreds[:d]) and len(shreds[0][0x40:0x58]) == 0x18
        sets.append(shreds)
        D, C = D + d, C + p
    return sets


def shred(oracle, batch, dsc, priv):
    """front, parity and seal: the finished sets; priv None leaves the
    signature fields zero"""
    out = []
    for s in front(batch, dsc):
        code, filled = rs.fill(s)
        assert code == 0
        code, sealed, _, _ = fec_model.seal(oracle, filled, priv)
        assert code == 0
        out.append(sealed)
    return out


def seeded_batch(seed, sz):
    """the fixture's batches: sz bytes of random.Random( seed ).randbytes"""
    return random.Random(seed).randbytes(sz)


def digests(sets):
    return [hashlib.sha256(s).digest() for st in sets for s in st]


def judge(sz, off, buf_sz, s0, s1, n_set, h0, h1, n):
    """rule 5"""
    if sz == 0 or off > buf_sz or sz > buf_sz - off:
        return ERR_BATCH
    if s0 > s1 or s1 > n_set or h0 > h1 or h1 > n:
        return BAD_RESERVATION
    sets, nd, npar = count(sz)
    return OK if (s1 - s0, h1 - h0) == (sets, nd + npar) else BAD_RESERVATION
