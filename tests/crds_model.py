"""Test-side model of what fd_gossip_recv_packet and fd_gossip_recv_crds_value
(src/flamenco/gossip/fd_gossip.c:1858-1878, :1420-1430, :1020-1105) decide
for the CRDS values of one pull response or push message up to and including
fd_ed25519_verify: a bincode walk with a cursor, field by field as
src/flamenco/types/fd_types.c's decoders go (so a size is never computed,
only run out of), the key the switch picks, the own-identity drop, the signed
bytes, the signature by the reference's compiled fd_ed25519_verify
(fdref_verify) where oracle/_ref is built and by the CPU oracle elsewhere,
and the value hash with hashlib.  Written from those rules and not from the
library."""
import hashlib

from packet_model import Cursor, Short
from shred_model import verifier  # noqa: F401  (fd_ed25519_verify(msg, sig, pub) -> code)

OK, ERR_PARSE, BAD_RESERVATION, UNSUPPORTED, ERR_SIGNATURE, OWN = 0, -16, -17, -18, -20, -21
MAX = 1232        # PACKET_DATA_SIZE
VAL_MAX = 10      # (1232 - 44) // 115
VARIANTS = ("contact_info_v1", "vote", "lowest_slot", "snapshot_hashes", "accounts_hashes", "epoch_slots", "version_v1",
            "version_v2", "node_instance", "duplicate_shred", "incremental_snapshot_hashes", "contact_info_v2")


class Encoding(Exception):
    """FD_BINCODE_ERR_ENCODING, or a transaction the parser rejects"""


def u8(c):
    return c.take(1)[0]


def boolean(c):
    """fd_bincode_bool_decode: option tags too"""
    b = u8(c)
    if b > 1:
        raise Encoding
    return b


def compact_u16(c):
    """fd_bincode_compact_u16_decode (fd_bincode.h:204-232)"""
    rest = c.p[c.at:c.at + 3]
    if len(rest) >= 1 and not rest[0] & 0x80:
        c.take(1)
        return rest[0]
    if len(rest) >= 2 and not rest[1] & 0x80:
        if not rest[1]:
            raise Encoding
        c.take(2)
        return (rest[0] & 0x7F) + (rest[1] << 7)
    if len(rest) >= 3 and not rest[2] & 0xFC:
        if not rest[2]:
            raise Encoding
        c.take(3)
        return (rest[0] & 0x7F) + ((rest[1] & 0x7F) << 7) + (rest[2] << 14)
    raise Short


def varint(c):
    """fd_bincode_varint_decode (fd_bincode.h:311-340)"""
    out, shift = 0, 0
    while shift < 64:
        b = u8(c)
        out |= ((b & 0x7F) << shift) & (2 ** 64 - 1)
        if not b & 0x80:
            if out >> shift != b or (b == 0 and (shift != 0 or out != 0)):
                raise Encoding
            return out
        shift += 7
    raise Encoding


def byte_vec(c):
    """a u64 length and as many bytes: compared with what remains, never added"""
    n = c.u64()
    if n > len(c.p) - c.at:
        raise Short
    return c.take(n)


def ip_addr(c):
    d = c.u32()
    if d > 1:
        raise Encoding
    return c.take(16 if d else 4)


def socket_addr(c):
    ip_addr(c)
    c.take(2)


def slot_hashes(c):
    for _ in range(c.u64()):     # runs out of bytes long before a huge length ends
        c.take(40)


def txn_prefix(c):
    """fd_txn_parse_core with a size out-parameter (src/ballet/txn/fd_txn_parse.c):
    every check but "no byte left over"; the compact-u16s see all that remains"""
    def check(ok):
        if not ok:
            raise Encoding
    try:
        check(len(c.p) - c.at <= 1232)
        sig_cnt = u8(c)
        check(1 <= sig_cnt <= 127)
        c.take(64 * sig_cnt)
        b0 = u8(c)
        v0 = bool(b0 & 0x80)
        if v0:
            check(b0 & 0x7F == 0)
            check(u8(c) == sig_cnt)
        else:
            check(b0 == sig_cnt)
        check(u8(c) < sig_cnt)
        ro_unsigned = u8(c)
        acct = compact_u16(c)
        check(sig_cnt <= acct <= 128 and sig_cnt + ro_unsigned <= acct)
        c.take(32 * acct)
        c.take(32)
        instr = compact_u16(c)
        check(instr <= 64)
        check(3 * instr <= len(c.p) - c.at)
        check(acct > (1 if instr else 0))
        max_acct = 0
        for _ in range(instr):
            check(3 <= len(c.p) - c.at)
            prog = u8(c)
            max_acct = max([max_acct] + list(c.take(compact_u16(c))))
            c.take(compact_u16(c))
            check(0 < prog < acct)
        adtl = 0
        if v0:
            luts = compact_u16(c)
            check(luts <= 127)
            check(34 * luts <= len(c.p) - c.at)
            for _ in range(luts):
                c.take(32)
                w = compact_u16(c)
                c.take(w)
                r = compact_u16(c)
                c.take(r)
                check(w <= 128 - acct and r <= 128 - acct and w + r >= 1)
                adtl += w + r
        check(acct + adtl <= 128 and max_acct < acct + adtl)
    except Short:
        raise Encoding from None    # the parser's own bounds checks: a rejected transaction


def data(c):
    """fd_crds_data at the cursor -> (discriminant, bytes into the data at
    which the variant's own key lies, or None for contact_info_v2)"""
    disc = c.u32()
    if disc == 0:
        c.take(32)
        for _ in range(10):
            socket_addr(c)
        c.take(8 + 2)
        return disc, 4
    if disc == 1:
        c.take(1 + 32)
        txn_prefix(c)
        c.take(8)
        return disc, 5
    if disc == 2:
        c.take(1 + 32 + 8 + 8)
        for _ in range(c.u64()):
            c.take(8)
        c.take(8 + 8)
        return disc, 5
    if disc in (3, 4):
        c.take(32)
        slot_hashes(c)
        c.take(8)
        return disc, 4
    if disc == 5:
        c.take(1 + 32)
        for _ in range(c.u64()):
            kind = c.u32()
            if kind > 1:
                raise Encoding
            c.take(8 + 8)
            if kind == 0:
                byte_vec(c)
            else:
                if boolean(c):
                    byte_vec(c)
                c.take(8)
        c.take(8)
        return disc, 5
    if disc in (6, 7):
        c.take(32 + 8 + 2 + 2 + 2)
        if boolean(c):
            c.take(4)
        if disc == 7:
            c.take(4)
        return disc, 4
    if disc == 8:
        c.take(32 + 8 + 8 + 8)
        return disc, 4
    if disc == 9:
        c.take(2 + 32 + 8 + 8 + 4 + 1 + 1 + 1)
        byte_vec(c)
        return disc, 6
    if disc == 10:
        c.take(32 + 40)
        slot_hashes(c)
        c.take(8)
        return disc, 4
    if disc == 11:
        c.take(32)
        varint(c)
        c.take(8 + 2)
        compact_u16(c), compact_u16(c), compact_u16(c)
        c.take(4 + 4)
        compact_u16(c)
        for _ in range(compact_u16(c)):
            ip_addr(c)
        for _ in range(compact_u16(c)):
            c.take(2)
            compact_u16(c)
        for _ in range(compact_u16(c)):
            c.take(4)
        return disc, None
    raise Encoding


def walk(p):
    """(packet code, [(data discriminant, start, key offset, end)]): the
    decode of the whole packet, offsets into it"""
    if p is None or not 4 <= len(p) <= MAX:
        return ERR_PARSE, []
    c = Cursor(p)
    disc = c.u32()
    if disc >= 6:
        return ERR_PARSE, []
    if disc not in (1, 2):
        return UNSUPPORTED, []
    vals = []
    try:
        c.take(32)
        for _ in range(c.u64()):
            start = c.at
            c.take(64)
            d, key = data(c)
            vals.append((d, start, 4 if key is None else start + 64 + key, c.at))
    except (Short, Encoding):
        return ERR_PARSE, []
    if not c.done():
        return ERR_PARSE, []
    return OK, vals


def signed(p, self_key):
    """(packet code, [(discriminant, pre, key, signature, message, value
    bytes)]): pre is OWN for a value under the own identity (decided first,
    fd_gossip.c:1072), else UNSUPPORTED for a contact_info_v2 -- the
    reference verifies and hashes its own re-encode, which writes plain u16
    where the decoder read compact-u16 and never equals the received bytes
    (tests/golden/crds.npz holds the reference's bytes) --, else 0"""
    code, vals = walk(p)
    return code, [(d, OWN if p[k:k + 32] == self_key else UNSUPPORTED if d == 11 else OK, p[k:k + 32], p[s:s + 64],
                   p[s + 64:e], p[s:e]) for d, s, k, e in vals]


def judge(verify, p, self_key):
    """(packet code, [(value code, fd_ed25519_verify's own code or 0 where
    the value is not verified, value hash or zeros where the reference would
    hash other bytes)])"""
    code, vals = signed(p, self_key)
    out = []
    for d, pre, key, sig, msg, raw in vals:
        v = 0 if pre else verify(msg, sig, key)
        out.append((pre or (ERR_SIGNATURE if v != 0 else OK), v, bytes(32) if d == 11 else hashlib.sha256(raw).digest()))
    return code, out
