"""Test-side model of what fd_fec_resolver_add_shred decides for a Merkle
shred that opens a FEC set (src/disco/shred/fd_fec_resolver.c:311-409 on
fd_shred_parse, src/ballet/shred/fd_shred.c:3-72): the parse, the header
rejections, the leaf and the walk of the inclusion proof with hashlib, the
signature by the reference's compiled fd_ed25519_verify (fdref_verify) where
oracle/_ref is built and by the CPU oracle elsewhere.  The resolver itself
needs its maps and free lists, so its rules are applied here, written from
the rules and not from the library."""
import ctypes
import hashlib
import struct

OK, ERR_PARSE, UNSUPPORTED, ERR_HEADER, ERR_SIGNATURE = 0, -16, -18, -19, -20
LEAF, NODE = b"\x00SOLANA_MERKLE_SHREDS_LEAF", b"\x01SOLANA_MERKLE_SHREDS_NODE"
CHAINED = (0x90, 0x60, 0xB0, 0x70)


def parses(s):
    """fd_shred_parse returns the shred"""
    if len(s) < 0x58:
        return False
    variant = s[0x40]
    typ = variant & 0xF0
    if typ not in (0x80, 0x40) + CHAINED and variant not in (0xA5, 0x5A):
        return False
    proof = 0 if typ in (0xA0, 0x50) else 20 * (variant & 0xF)
    chained = 32 if typ in CHAINED else 0
    if typ & 0x80:
        size, = struct.unpack_from("<H", s, 0x56)
        if size < 0x58 or (typ != 0xA0 and len(s) < 1203):
            return False
        eff = len(s) if typ & 0x20 else 1203
        return eff >= 0x58 + proof + (size - 0x58) + chained and len(s) >= eff
    return len(s) >= 1228


def root(s):
    """(code, root): rules 1-5"""
    if not parses(s):
        return ERR_PARSE, None
    variant = s[0x40]
    typ, depth = variant & 0xF0, variant & 0xF
    if typ not in (0x80, 0x40):
        return UNSUPPORTED, None
    data = typ == 0x80
    if s[:64] == bytes(64):
        return ERR_HEADER, None
    idx, fec = struct.unpack_from("<I", s, 0x49)[0], struct.unpack_from("<I", s, 0x4F)[0]
    data_cnt, code_cnt, code_idx = struct.unpack_from("<HHH", s, 0x53)
    if not data and not (0 < data_cnt <= 67 and 0 < code_cnt <= 67):
        return ERR_HEADER, None
    in_type = (idx - fec) & 0xFFFFFFFF if data else code_idx
    if in_type >= 67:
        return ERR_HEADER, None
    shred_idx = in_type if data else in_type + data_cnt
    leaves = shred_idx + 1
    if (leaves if leaves <= 1 else (leaves - 1).bit_length() + 1) > depth + 1:   # fd_bmtree_depth: msb + 2
        return ERR_HEADER, None
    node = hashlib.sha256(LEAF + s[64:64 + 1115 - 20 * depth + 0x18 + (0 if data else 0x19)]).digest()
    at = (1203 if data else 1228) - 20 * depth
    for l in range(depth):
        sib = s[at + 20 * l:at + 20 * l + 20]
        pair = sib + node[:20] if (shred_idx >> l) & 1 else node[:20] + sib
        node = hashlib.sha256(NODE + pair).digest()
    return OK, node


def verifier(oracle):
    """fd_ed25519_verify(msg, sig, pub) -> code (0: success)"""
    from txn_util import ref_lib
    ref = ref_lib()
    if ref is not None:
        ref.fdref_verify.argtypes = [ctypes.c_char_p, ctypes.c_ulong, ctypes.c_char_p, ctypes.c_char_p]
        return lambda m, sig, pub: ref.fdref_verify(m, len(m), sig, pub)
    return lambda m, sig, pub: oracle.oracle_ed25519_verify(m, len(m), sig, pub, 0)


def judge(verify, s, pub):
    """(code, root or None): rules 1-6"""
    code, r = root(s)
    if code == OK and verify(r, s[:64], pub) != 0:
        code = ERR_SIGNATURE
    return code, r
