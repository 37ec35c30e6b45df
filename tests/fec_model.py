"""Test-side model of what fd_shredder_next_fec_set does to a filled FEC set
(src/disco/shred/fd_shredder.c:225-260 on fd_bmtree_commit_*,
src/ballet/bmtree/fd_bmtree.c:216-348): the set rules, the leaves, the tree
with its self-merged odd nodes and the doubly linked proofs with hashlib,
the signature of the root by the CPU oracle's fd_ed25519_sign.  Written from
the rules of fd_fec_core.h's header comment and not from the library."""
import ctypes
import hashlib
import struct

from shred_model import LEAF, NODE, parses

OK, ERR_PARSE, UNSUPPORTED, ERR_SET = 0, -16, -18, -19
CNT_MAX = 134


def depth_of(cnt):
    """fd_bmtree_depth( cnt ) - 1: 0 for one leaf, else msb( cnt-1 ) + 1"""
    return 0 if cnt <= 1 else (cnt - 1).bit_length()


def proof_at(s, depth):
    return (1203 if s[0x40] & 0xF0 == 0x80 else 1228) - 20 * depth


def shred_code(s, cnt, j):
    """rule 2 for shred j of a set of cnt"""
    if not parses(s):
        return ERR_PARSE
    variant = s[0x40]
    typ = variant & 0xF0
    if typ not in (0x80, 0x40):
        return UNSUPPORTED
    if variant & 0xF != depth_of(cnt):
        return ERR_SET
    if typ == 0x80:
        idx = (struct.unpack_from("<I", s, 0x49)[0] - struct.unpack_from("<I", s, 0x4F)[0]) & 0xFFFFFFFF
    else:
        data_cnt, code_cnt, code_idx = struct.unpack_from("<HHH", s, 0x53)
        if not (0 < data_cnt <= 67 and 0 < code_cnt <= 67):
            return ERR_SET
        idx = data_cnt + code_idx
    return OK if idx == j else ERR_SET


def set_code(shreds):
    """rules 1-2"""
    cnt = len(shreds)
    if cnt == 0 or cnt > CNT_MAX:
        return ERR_SET
    for j, s in enumerate(shreds):
        code = shred_code(s, cnt, j)
        if code:
            return code
    return OK


def tree(shreds):
    """(code, root, [proof bytes of leaf j]): rules 1-5"""
    code = set_code(shreds)
    if code:
        return code, None, None
    cnt, depth = len(shreds), depth_of(len(shreds))
    layers = [[hashlib.sha256(LEAF + s[64:proof_at(s, depth)]).digest() for s in shreds]]
    while len(layers[-1]) > 1:
        cur = layers[-1]
        layers.append([hashlib.sha256(NODE + cur[2 * t][:20] + cur[min(2 * t + 1, len(cur) - 1)][:20]).digest()
                       for t in range((len(cur) + 1) // 2)])
    assert len(layers) == depth + 1
    proofs = [b"".join(layers[l][min((j >> l) ^ 1, len(layers[l]) - 1)][:20] for l in range(depth)) for j in range(cnt)]
    return OK, layers[-1][0], proofs


def sign(oracle, msg, priv):
    pub, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    oracle.oracle_ed25519_public_from_private(pub, priv)
    oracle.oracle_ed25519_sign(sig, msg, len(msg), pub.raw, priv)
    return sig.raw


def public_key(oracle, priv):
    pub = ctypes.create_string_buffer(32)
    oracle.oracle_ed25519_public_from_private(pub, priv)
    return pub.raw


def seal(oracle, shreds, priv):
    """(code, the shreds as the seal leaves them, root, signature): rules
    1-6; priv None leaves bytes [0, 64) alone and gives no signature"""
    code, root, proofs = tree(shreds)
    if code:
        return code, [bytes(s) for s in shreds], None, None
    depth = depth_of(len(shreds))
    sig = sign(oracle, root, priv) if priv is not None else None
    out = []
    for s, proof in zip(shreds, proofs):
        s, at = bytearray(s), proof_at(s, depth)
        s[at:at + 20 * depth] = proof
        if sig is not None:
            s[:64] = sig
        out.append(bytes(s))
    return OK, out, root, sig
