"""Test-side model of what fd_gossip_recv_packet
(src/flamenco/gossip/fd_gossip.c:1858-1878, :646-656, :940-949, :1201-1236)
and fd_repair_recv_serv_packet (src/flamenco/repair/fd_repair.c:1012-1070)
decide for one signed control packet up to and including fd_ed25519_verify:
a bincode walk with a cursor, field by field as
src/flamenco/types/fd_types.c's decoders go (so a size is never computed,
only run out of), the addressee check, the signed bytes assembled as the
handlers assemble them, the signature by the reference's compiled
fd_ed25519_verify (fdref_verify) where oracle/_ref is built and by the CPU
oracle elsewhere.  Written from those rules and not from the library."""
import struct

from shred_model import verifier  # noqa: F401  (fd_ed25519_verify(msg, sig, pub) -> code)

OK, ERR_PARSE, UNSUPPORTED, ERR_SIGNATURE, NOT_FOR_SELF = 0, -16, -18, -20, -21
GOSSIP, REPAIR = 0, 1
MAX = 1232   # PACKET_DATA_SIZE


class Short(Exception):
    """a bincode read past the end of the packet"""


class Cursor:
    def __init__(self, p):
        self.p, self.at = p, 0

    def take(self, k):
        if self.at + k > len(self.p):
            raise Short
        self.at += k
        return self.p[self.at - k:self.at]

    def u32(self):
        return struct.unpack("<I", self.take(4))[0]

    def u64(self):
        return struct.unpack("<Q", self.take(8))[0]

    def done(self):
        return self.at == len(self.p)


def ping(c):
    """fd_gossip_ping: from, token, signature"""
    return {"from": c.take(32), "token": c.take(32), "signature": c.take(64)}


def request_header(c):
    """fd_repair_request_header"""
    return {"signature": c.take(64), "sender": c.take(32), "recipient": c.take(32), "timestamp": c.u64(), "nonce": c.u32()}


def signed(proto, p, self_key):
    """(code, (key, signature, message) or None): everything before the verify"""
    if not 4 <= len(p) <= MAX:
        return ERR_PARSE, None
    c = Cursor(p)
    disc = c.u32()
    try:
        if proto == GOSSIP:
            if disc <= 2:
                return UNSUPPORTED, None        # CRDS values: not looked at
            if disc in (4, 5):
                m = ping(c)
                if not c.done():
                    return ERR_PARSE, None
                return OK, (m["from"], m["signature"], m["token"])
            if disc != 3:
                return ERR_PARSE, None
            c.take(32)                          # the outer pubkey, ignored
            pubkey, prunes_len = c.take(32), c.u64()
            prunes = []
            for _ in range(prunes_len):         # runs out of bytes long before a huge prunes_len ends
                prunes.append(c.take(32))
            signature, destination, wallclock = c.take(64), c.take(32), c.take(8)
            if not c.done():
                return ERR_PARSE, None
            if destination != self_key:
                return NOT_FOR_SELF, None
            # fd_gossip_prune_sign_data: pubkey, prunes (u64 length), destination, wallclock
            msg = pubkey + struct.pack("<Q", prunes_len) + b"".join(prunes) + destination + wallclock
            return OK, (pubkey, signature, msg)
        assert proto == REPAIR
        if disc <= 6:
            return (UNSUPPORTED if c.done() else ERR_PARSE), None
        if disc == 7:
            ping(c)
            return (UNSUPPORTED if c.done() else ERR_PARSE), None
        if disc in (8, 9):
            h = request_header(c)
            c.u64(), c.u64()                    # slot, shred_index
        elif disc in (10, 11):
            h = request_header(c)
            c.u64()                             # slot
        else:
            return ERR_PARSE, None
        if not c.done():
            return ERR_PARSE, None
        if disc == 11:
            return UNSUPPORTED, None
        if h["recipient"] != self_key:
            return NOT_FOR_SELF, None
        # the discriminant copied over the signature's last four bytes, verified from there
        return OK, (h["sender"], h["signature"], p[:4] + p[68:])
    except Short:
        return ERR_PARSE, None


def judge(verify, proto, p, self_key):
    """(code, fd_ed25519_verify's own code or 0 where the packet is not judged)"""
    code, s = signed(proto, p, self_key)
    if code != OK:
        return code, 0
    key, sig, msg = s
    v = verify(msg, sig, key)
    return (ERR_SIGNATURE if v != 0 else OK), v
