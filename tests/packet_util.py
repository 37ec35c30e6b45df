"""Builds signed gossip and repair control packets for the packet tests:
every kind fd_gossip_recv_packet and fd_repair_recv_serv_packet decode, with
valid signatures made by the oracle, the rule-edge cases of
fd_packet_core.h, seeded mutations, and the reference-judged fixture
(tests/golden/packets.npz)."""
import functools
import random
import struct

import packet_model as model
from conftest import load_golden
from txn_util import Signer

GOSSIP, REPAIR = model.GOSSIP, model.REPAIR


class Node:
    """a validator identity that signs packets; every unsigned byte random"""

    def __init__(self, oracle, seed):
        self.sg = Signer(oracle, seed)
        self.priv, self.pub = self.sg.key()
        self.rng = random.Random(seed)

    def rand(self, k):
        return bytes(self.rng.getrandbits(8) for _ in range(k))

    def sign(self, msg):
        return self.sg.sign(msg, self.priv, self.pub)

    def ping(self, disc=4):
        """gossip ping (4) or pong (5), or the repair port's pong (7)"""
        token = self.rand(32)
        return struct.pack("<I", disc) + self.pub + token + self.sign(token)

    def prune(self, m, destination, outer=None, signer=None):
        """gossip prune of m origins for destination, signed as data.pubkey
        signs it -- or by another node (signer), then invalid"""
        prunes, wallclock = self.rand(32 * m), self.rand(8)
        msg = self.pub + struct.pack("<Q", m) + prunes + destination + wallclock
        sig = (signer or self).sign(msg)
        return struct.pack("<I", 3) + (self.pub if outer is None else outer) + self.pub + struct.pack("<Q", m) + prunes + \
            sig + destination + wallclock

    def request(self, disc, recipient, signer=None):
        """repair window_index (8), highest_window_index (9), orphan (10) or
        ancestor_hashes (11) request to recipient"""
        body = self.pub + recipient + self.rand(8 + 4) + self.rand(8 if disc in (10, 11) else 16)
        head = struct.pack("<I", disc)
        return head + (signer or self).sign(head + body) + body


def valid_packets(oracle, seed, self_key, prune_ms=range(33)):
    """[(name, proto, packet)]: one valid packet of every kind either port
    decodes, a prune of every m"""
    nd = Node(oracle, seed)
    out = [("ping", GOSSIP, nd.ping(4)), ("pong", GOSSIP, nd.ping(5))]
    out += [(f"prune_m{m}", GOSSIP, nd.prune(m, self_key)) for m in prune_ms]
    out += [(f"request_{d}", REPAIR, nd.request(d, self_key)) for d in (8, 9, 10)]
    out += [("ancestor_hashes", REPAIR, nd.request(11, self_key)), ("repair_pong", REPAIR, nd.ping(7))]
    out += [(f"legacy_{d}", REPAIR, struct.pack("<I", d)) for d in range(7)]
    return out


def mutate(rng, proto, p, other_key):
    """one seeded mutation of a valid packet -> (kind, packet)"""
    p = bytearray(p)
    prune = proto == GOSSIP and p[0] == 3
    kinds = ["truncate1", "extend1", "disc", "disc_random", "bitflip", "addressee", "truncate", "extend", "unsigned_field"]
    if prune:
        kinds += ["m_plus", "m_minus", "m_wrap59", "m_wrap64"]
    kind = rng.choice(kinds)
    if kind == "truncate1":
        del p[-1:]
    elif kind == "extend1":
        p.append(rng.getrandbits(8))
    elif kind == "disc":
        p[:4] = struct.pack("<I", rng.randrange(14))
    elif kind == "disc_random":
        p[:4] = struct.pack("<I", rng.getrandbits(32))
    elif kind == "bitflip" and len(p) > 4:
        p[rng.randrange(4, len(p))] ^= 1 << rng.randrange(8)
    elif kind == "addressee" and len(p) >= 132:
        at = len(p) - 40 if prune else 100
        p[at:at + 32] = other_key
    elif kind == "unsigned_field":
        # what no signature covers: a prune's outer pubkey, ping for pong; a
        # repair request's discriminant is signed (8 for 9), the rest stays
        if prune:
            p[4:36] = other_key
        elif proto == GOSSIP:
            p[0] ^= 1
        elif p[0] in (8, 9):
            p[0] ^= 1
    elif kind == "truncate":
        del p[rng.randrange(len(p)):]
    elif kind == "extend":
        p += bytes(rng.getrandbits(8) for _ in range(rng.randrange(2, 40)))
    elif kind.startswith("m_"):
        m, = struct.unpack_from("<Q", p, 68)
        m = {"m_plus": m + 1, "m_minus": (m - 1) % 2 ** 64, "m_wrap59": 2 ** 59 + 1, "m_wrap64": 2 ** 64 - 1}[kind]
        struct.pack_into("<Q", p, 68, m)
    return kind, bytes(p)


def mutated(oracle, count, seed, self_key, prune_ms=(0, 1, 2, 3, 5, 8)):
    """[(kind, proto, packet)]: count seeded mutations of valid packets"""
    rng = random.Random(seed)
    base = valid_packets(oracle, seed, self_key, prune_ms)
    other = Node(oracle, seed + 1).pub
    out = []
    for _ in range(count):
        name, proto, p = base[rng.randrange(len(base))]
        kind, q = mutate(rng, proto, p, other)
        out.append((f"{name}:{kind}", proto, q))
    return out


@functools.lru_cache(maxsize=None)
def fixture():
    """the reference-judged packets of tests/golden/packets.npz:
    (self_key, [dict(proto, pkt, decodes, disc, sign_data)])"""
    d = load_golden("packets")
    buf, sbuf, at, sat, out = d["pkts"].tobytes(), d["sign_data"].tobytes(), 0, 0, []
    for proto, sz, ok, disc, ssz in zip(d["proto"], d["sz"], d["decodes"], d["disc"], d["sign_data_sz"]):
        out.append({"proto": int(proto), "pkt": buf[at:at + int(sz)], "decodes": bool(ok), "disc": int(disc),
                    "sign_data": sbuf[sat:sat + int(ssz)] if ssz else None})
        at += int(sz)
        sat += int(ssz)
    return d["self_key"].tobytes(), out


@functools.lru_cache(maxsize=None)
def _rule_cases(oracle):
    me, nd, ot = Node(oracle, 71), Node(oracle, 73), Node(oracle, 79)
    c = []

    def add(name, proto, p, want, key=None):
        c.append((name, proto, p, me.pub if key is None else key, want))

    for disc, name, full in ((4, "ping", 132), (5, "pong", 132)):
        p = nd.ping(disc)
        add(f"{name}", GOSSIP, p, model.OK)
        add(f"{name}_sz_{full - 1}", GOSSIP, p[:-1], model.ERR_PARSE)
        add(f"{name}_sz_{full + 1}", GOSSIP, p + b"\0", model.ERR_PARSE)
    for m in (0, 1, 32):
        p = nd.prune(m, me.pub)
        add(f"prune_m{m}", GOSSIP, p, model.OK)
        add(f"prune_m{m}_short", GOSSIP, p[:-1], model.ERR_PARSE)
        add(f"prune_m{m}_long", GOSSIP, p + b"\0", model.ERR_PARSE)
    p = nd.prune(32, me.pub)
    add("prune_m33", GOSSIP, p[:68] + struct.pack("<Q", 33) + p[76:] + bytes(32), model.ERR_PARSE)   # 1236 bytes
    add("prune_m33_in_1204", GOSSIP, p[:68] + struct.pack("<Q", 33) + p[76:], model.ERR_PARSE)
    p = nd.prune(4, me.pub)
    for name, m in (("m_minus", 3), ("m_plus", 5), ("m_wrap59", 2 ** 59 + 1), ("m_wrap59_exact", 2 ** 59 + 4),
                    ("m_wrap64", 2 ** 64 - 1)):
        add(f"prune_{name}", GOSSIP, p[:68] + struct.pack("<Q", m) + p[76:], model.ERR_PARSE)
    add("prune_sz_179", GOSSIP, nd.prune(0, me.pub)[:179], model.ERR_PARSE)
    add("prune_other_destination", GOSSIP, nd.prune(2, ot.pub), model.NOT_FOR_SELF)
    add("prune_outer_pubkey_differs", GOSSIP, nd.prune(2, me.pub, outer=ot.pub), model.OK)
    add("prune_signed_by_outer_pubkey", GOSSIP, nd.prune(2, me.pub, outer=ot.pub, signer=ot), model.ERR_SIGNATURE)
    for bit, name in ((0, "first"), (255, "last")):
        key = bytearray(me.pub)
        key[bit // 8] ^= 1 << (bit % 8)
        add(f"prune_self_key_{name}_bit", GOSSIP, nd.prune(1, me.pub), model.NOT_FOR_SELF, bytes(key))
        add(f"request_self_key_{name}_bit", REPAIR, nd.request(8, me.pub), model.NOT_FOR_SELF, bytes(key))
    for disc in (0, 1, 2):
        add(f"gossip_disc_{disc}", GOSSIP, struct.pack("<I", disc) + nd.rand(60), model.UNSUPPORTED)
        add(f"gossip_disc_{disc}_alone", GOSSIP, struct.pack("<I", disc), model.UNSUPPORTED)
    for disc in (6, 7, 0x104, 0xFFFFFFFF):
        add(f"gossip_disc_{disc:#x}", GOSSIP, struct.pack("<I", disc) + nd.ping(4)[4:], model.ERR_PARSE)
    for disc, full in ((8, 160), (9, 160), (10, 152)):
        p = nd.request(disc, me.pub)
        assert len(p) == full
        add(f"request_{disc}", REPAIR, p, model.OK)
        add(f"request_{disc}_sz_{full - 1}", REPAIR, p[:-1], model.ERR_PARSE)
        add(f"request_{disc}_sz_{full + 1}", REPAIR, p + b"\0", model.ERR_PARSE)
        add(f"request_{disc}_other_recipient", REPAIR, nd.request(disc, ot.pub), model.NOT_FOR_SELF)
    add("request_signed_by_recipient", REPAIR, nd.request(8, me.pub, signer=me), model.ERR_SIGNATURE)
    p = nd.request(11, me.pub)
    add("ancestor_hashes", REPAIR, p, model.UNSUPPORTED)
    add("ancestor_hashes_sz_151", REPAIR, p[:-1], model.ERR_PARSE)
    add("ancestor_hashes_sz_153", REPAIR, p + b"\0", model.ERR_PARSE)
    add("ancestor_hashes_other_recipient", REPAIR, nd.request(11, ot.pub), model.UNSUPPORTED)
    p = nd.ping(7)
    add("repair_pong", REPAIR, p, model.UNSUPPORTED)
    add("repair_pong_sz_131", REPAIR, p[:-1], model.ERR_PARSE)
    add("repair_pong_sz_133", REPAIR, p + b"\0", model.ERR_PARSE)
    for disc in range(7):
        add(f"legacy_{disc}", REPAIR, struct.pack("<I", disc), model.UNSUPPORTED)
        add(f"legacy_{disc}_sz_5", REPAIR, struct.pack("<I", disc) + b"\0", model.ERR_PARSE)
    for disc in (12, 13, 0x108, 0xFFFFFFFF):
        add(f"repair_disc_{disc:#x}", REPAIR, struct.pack("<I", disc) + nd.request(8, me.pub)[4:], model.ERR_PARSE)
    for proto in (GOSSIP, REPAIR):
        for sz in (0, 1, 3):
            add(f"proto{proto}_sz_{sz}", proto, bytes([4 if proto == GOSSIP else 8, 0, 0][:sz]), model.ERR_PARSE)
        add(f"proto{proto}_sz_1233", proto, struct.pack("<I", 1) + bytes(1229), model.ERR_PARSE)
    add("gossip_sz_1232", GOSSIP, struct.pack("<I", 2) + bytes(1228), model.UNSUPPORTED)
    flip = bytearray(nd.ping(4))
    flip[40] ^= 1
    add("ping_token_bit", GOSSIP, bytes(flip), model.ERR_SIGNATURE)
    assert len({n for n, _, _, _, _ in c}) == len(c)
    return tuple(c)


def rule_cases(oracle):
    """((name, proto, packet, self_key, the code the rules and the verify give), ...)"""
    return _rule_cases(oracle)
