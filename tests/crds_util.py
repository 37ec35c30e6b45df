"""Builds gossip pull responses and push messages for the CRDS tests: every
fd_crds_data variant with valid signatures made by the oracle, the rule-edge
cases of fd_crds_core.h, seeded mutations, and the reference-judged fixture
(tests/golden/crds.npz)."""
import functools
import random
import struct

import crds_model as model
from conftest import load_golden
from packet_util import Node
from packet_util import valid_packets as control_packets
from txn_util import cu16, random_txn

PULL_RESP, PUSH = 1, 2
WRAPS = (2 ** 59 + 1, 2 ** 64 - 1)


def u32(v):
    return struct.pack("<I", v)


def u64(v):
    return struct.pack("<Q", v % 2 ** 64)


def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    return bytes(out + bytes([v]))


class Data(bytes):
    """the bytes of one fd_crds_data with the places a mutation aims at:
    fields = [(kind, offset, size)], kind one of len64 (a u64 vector length),
    tag (an option tag), enum (a u32 discriminant of an inner enum), cu16,
    varint, txn (the vote's transaction)"""

    def __new__(cls, b, fields=()):
        self = super().__new__(cls, b)
        self.fields = tuple(fields)
        return self


class Build:
    """grows a Data and notes the fields"""

    def __init__(self, disc):
        self.b, self.fields = bytearray(u32(disc)), []

    def add(self, b, kind=None):
        if kind:
            self.fields.append((kind, len(self.b), len(b)))
        self.b += b
        return self

    def done(self):
        return Data(bytes(self.b), self.fields)


class Peer(Node):
    """a gossip identity: the data of every CRDS variant under its key (or
    under `key`), compressible filler in every field nothing checks"""

    def fill(self, k):
        return bytes([self.rng.getrandbits(8)]) * k

    def ip(self, b, six):
        b.add(u32(1 if six else 0), "enum").add(self.fill(16 if six else 4))

    def contact_info_v1(self, six=(), key=None):
        b = Build(0).add(key or self.pub)
        for i in range(10):
            self.ip(b, i in six)
            b.add(self.fill(2))
        return b.add(self.fill(8 + 2)).done()

    def vote(self, v0=False, txn=None, key=None):
        t = random_txn(self.sg, self.rng, 1 + self.rng.randrange(2), v0=v0) if txn is None else txn
        return Build(1).add(self.fill(1)).add(key or self.pub).add(t, "txn").add(self.fill(8)).done()

    def lowest_slot(self, n=0, key=None):
        return Build(2).add(self.fill(1)).add(key or self.pub).add(self.fill(16)).add(u64(n), "len64").add(self.fill(8 * n)) \
            .add(self.fill(16)).done()

    def slot_hashes(self, disc=3, n=1, key=None):
        return Build(disc).add(key or self.pub).add(u64(n), "len64").add(self.fill(40 * n)).add(self.fill(8)).done()

    def epoch_slots(self, kinds=("flate2", "bits"), key=None):
        """kinds: flate2 (compressed bytes), bits (uncompressed with its bit
        vector), nobits (uncompressed, option absent), empty (a bit vector of
        no bytes)"""
        b = Build(5).add(self.fill(1)).add(key or self.pub).add(u64(len(kinds)), "len64")
        for k in kinds:
            b.add(u32(0 if k == "flate2" else 1), "enum").add(self.fill(16))
            n = 0 if k == "empty" else 1 + self.rng.randrange(20)
            if k == "flate2":
                b.add(u64(n), "len64").add(self.fill(n))
            else:
                b.add(bytes([k != "nobits"]), "tag")
                if k != "nobits":
                    b.add(u64(n), "len64").add(self.fill(n))
                b.add(self.fill(8))
        return b.add(self.fill(8)).done()

    def version(self, disc=6, commit=False, key=None):
        b = Build(disc).add(key or self.pub).add(self.fill(8 + 6)).add(bytes([commit]), "tag")
        if commit:
            b.add(self.fill(4))
        if disc == 7:
            b.add(self.fill(4))
        return b.done()

    def node_instance(self, key=None):
        return Build(8).add(key or self.pub).add(self.fill(24)).done()

    def duplicate_shred(self, n=5, key=None):
        return Build(9).add(self.fill(2)).add(key or self.pub).add(self.fill(8 + 8 + 4 + 3)).add(u64(n), "len64") \
            .add(self.fill(n)).done()

    def incremental_snapshot_hashes(self, n=1, key=None):
        return Build(10).add(key or self.pub).add(self.fill(40)).add(u64(n), "len64").add(self.fill(40 * n)) \
            .add(self.fill(8)).done()

    def contact_info_v2(self, wallclock=1700000000000, addrs=(False, True), sockets=3, ext=1, big=0x81, key=None):
        """big: a version and offset value (one that takes two or three compact-u16 bytes when >= 0x80)"""
        b = Build(11).add(key or self.pub).add(varint(wallclock), "varint").add(self.fill(8 + 2))
        b.add(cu16(1), "cu16").add(cu16(big), "cu16").add(cu16(0x4000 if big >= 0x80 else 3), "cu16").add(self.fill(8))
        b.add(cu16(2), "cu16").add(cu16(len(addrs)), "cu16")
        for six in addrs:
            self.ip(b, six)
        b.add(cu16(sockets), "cu16")
        for _ in range(sockets):
            b.add(self.fill(2)).add(cu16(big), "cu16")
        b.add(cu16(ext), "cu16").add(self.fill(4 * ext))
        return b.done()

    def every_variant(self):
        """[(name, data)]: each variant, in the shapes that take another path through its decoder"""
        return [("contact_info_v1", self.contact_info_v1()), ("contact_info_v1_ip6", self.contact_info_v1(six=(0, 3, 9))),
                ("vote", self.vote()), ("vote_v0", self.vote(v0=True)),
                ("lowest_slot", self.lowest_slot()), ("lowest_slot_3", self.lowest_slot(3)),
                ("snapshot_hashes", self.slot_hashes(3, 2)), ("accounts_hashes", self.slot_hashes(4, 0)),
                ("epoch_slots", self.epoch_slots()), ("epoch_slots_none", self.epoch_slots(())),
                ("epoch_slots_all", self.epoch_slots(("nobits", "flate2", "empty", "bits"))),
                ("version_v1", self.version(6)), ("version_v1_commit", self.version(6, True)),
                ("version_v2", self.version(7)), ("version_v2_commit", self.version(7, True)),
                ("node_instance", self.node_instance()),
                ("duplicate_shred", self.duplicate_shred()), ("duplicate_shred_0", self.duplicate_shred(0)),
                ("incremental_snapshot_hashes", self.incremental_snapshot_hashes(2)),
                ("contact_info_v2", self.contact_info_v2()),
                ("contact_info_v2_small", self.contact_info_v2(wallclock=0, addrs=(), sockets=0, ext=0, big=5))]

    def value(self, data, signer=None):
        return (signer or self).sign(bytes(data)) + bytes(data)


class Packet(bytes):
    """a pull response or push message with its values' starts and, per
    value, the fields of its data at their packet offsets"""

    def __new__(cls, disc, outer, values, datas, crds_len=None):
        self = super().__new__(cls, u32(disc) + outer + u64(len(values) if crds_len is None else crds_len) + b"".join(values))
        self.starts, self.fields, at = [], [], 44
        for v, d in zip(values, datas):
            self.starts.append(at)
            self.fields += [(kind, at + 64 + off, sz) for kind, off, sz in getattr(d, "fields", ())]
            at += len(v)
        return self


class Other(bytes):
    """a packet without CRDS values, for mutate"""
    starts, fields = (), ()


def packet(peer, datas, disc=PUSH, outer=None, signers=None, crds_len=None):
    """datas signed by peer (or signers[i]) in one message under peer's pubkey (or outer)"""
    signers = signers or [peer] * len(datas)
    return Packet(disc, peer.pub if outer is None else outer, [s.value(d) for s, d in zip(signers, datas)], datas, crds_len)


def valid_packets(oracle, seed, me=None):
    """[(name, Packet)]: each variant alone as push and as pull response, every
    crds_len 0..VAL_MAX, mixed packets, values of the own identity `me` (a
    Peer) among them"""
    pr, other = Peer(oracle, seed), Peer(oracle, seed + 1000)
    out = []
    for name, d in pr.every_variant():
        out.append((f"push_{name}", packet(pr, [d], PUSH)))
    for name, d in pr.every_variant():
        out.append((f"pull_{name}", packet(pr, [d], PULL_RESP)))
    for n in range(model.VAL_MAX + 1):
        out.append((f"push_{n}_version_v1", packet(pr, [pr.version(6) for _ in range(n)], PUSH)))
    for n in (2, 3, 5):
        pool = pr.every_variant()
        pick = [pool[pr.rng.randrange(len(pool))] for _ in range(n)]
        if sum(len(d) + 64 for _, d in pick) + 44 <= model.MAX:
            out.append((f"mixed_{n}_" + "_".join(nm for nm, _ in pick), packet(pr, [d for _, d in pick], PULL_RESP)))
    out.append(("three_votes", packet(pr, [pr.vote(), pr.vote(v0=True), pr.vote()], PUSH)))
    out.append(("two_peers", packet(pr, [pr.node_instance(), other.lowest_slot(2), other.version(7, True)], PUSH,
                                    signers=[pr, other, other])))
    # contact_info_v2: the reference verifies its re-encode under the message's pubkey, whoever `from` is
    out.append(("ci2_signed_by_outer", packet(pr, [other.contact_info_v2()], PUSH, signers=[pr])))
    out.append(("ci2_signed_by_from", packet(pr, [other.contact_info_v2()], PUSH, signers=[other])))
    if me is not None:
        out.append(("own_alone", packet(me, [me.version(6)], PUSH, outer=pr.pub)))
        out.append(("own_between", packet(pr, [pr.node_instance(), me.lowest_slot(1), pr.version(7)], PULL_RESP,
                                          signers=[pr, me, pr])))
        out.append(("own_unsigned", packet(pr, [me.duplicate_shred(3), me.vote()], PUSH)))       # dropped before any verify
        out.append(("own_outer_ci2", packet(me, [pr.contact_info_v2(addrs=(True,), sockets=1)], PUSH, signers=[pr])))
        out.append(("own_from_ci2", packet(pr, [me.contact_info_v2(big=7)], PUSH, signers=[pr])))  # the outer key counts
        for name, d in me.every_variant()[:-2]:
            out.append((f"own_{name}", packet(pr, [d, pr.version(6)], PUSH, signers=[me, pr])))
    return out


def non_minimal(kind, b, rng):
    """an encoding of the same compact-u16 or varint that is too long, or one that is over-long for any value"""
    if kind == "cu16":
        v = model.compact_u16(model.Cursor(b))
        forms = [bytes([(v & 0x7F) | 0x80, (v >> 7) | 0x80, 0])] if v < 0x4000 else []
        forms += [bytes([v | 0x80, 0])] if v < 0x80 else []
        forms += [bytes([b[0] | 0x80, 0x80 | (b[1] if len(b) > 1 else 0), 4 + rng.randrange(252)])]
        return rng.choice(forms)
    return rng.choice([b[:-1] + bytes([b[-1] | 0x80, 0]), bytes([0x80 | b[0]]) + bytes([0x80] * 9) + b"\x01",
                       bytes([0xFF] * 9) + bytes([2 + rng.randrange(126)])])


def mutate(rng, p):
    """one seeded mutation of a valid Packet -> (kind, bytes)"""
    q = bytearray(p)
    kinds = ["truncate1", "extend1", "truncate", "extend", "disc", "disc_random", "bitflip", "crds_len"]
    if p.starts:
        kinds += ["data_disc", "sig_bit", "sig_bit", "value_bit"]
    kinds += sorted({k for k, _, _ in p.fields})
    if any(k == "txn" for k, _, _ in p.fields):
        kinds.append("txn_cut")
    kind = rng.choice(kinds)
    field = rng.choice([f for f in p.fields if f[0] == kind.replace("txn_cut", "txn")] or [None])
    if kind == "truncate1":
        del q[-1:]
    elif kind == "extend1":
        q.append(rng.getrandbits(8))
    elif kind == "truncate":
        del q[rng.randrange(len(q)):]
    elif kind == "extend":
        q += bytes(rng.getrandbits(8) for _ in range(rng.randrange(2, 40)))
    elif kind == "disc":
        q[:4] = u32(rng.randrange(14))
    elif kind == "disc_random":
        q[:4] = u32(rng.getrandbits(32))
    elif kind == "bitflip":
        q[rng.randrange(4, len(q))] ^= 1 << rng.randrange(8)
    elif kind == "crds_len":
        n, = struct.unpack_from("<Q", q, 36)
        q[36:44] = u64(rng.choice((n + 1, n - 1) + WRAPS))
    elif kind == "data_disc":
        at = rng.choice(p.starts) + 64
        q[at:at + 4] = u32(rng.randrange(14))
    elif kind == "sig_bit":
        q[rng.choice(p.starts) + rng.randrange(64)] ^= 1 << rng.randrange(8)
    elif kind == "value_bit":      # in a value's last byte but one: signed, and of fixed width in most variants
        ends = p.starts[1:] + [len(p)]
        q[rng.choice(ends) - 2] ^= 1 << rng.randrange(8)
    elif kind == "len64":
        n, = struct.unpack_from("<Q", q, field[1])
        q[field[1]:field[1] + 8] = u64(rng.choice((n + 1, n - 1) + WRAPS))
    elif kind == "tag":
        q[field[1]] = rng.choice((2, 0xFF, q[field[1]] ^ 1))
    elif kind == "enum":
        q[field[1]:field[1] + 4] = u32(rng.choice((2, 0xFFFFFFFF, q[field[1]] ^ 1)))
    elif kind in ("cu16", "varint"):
        q[field[1]:field[1] + field[2]] = non_minimal(kind, bytes(q[field[1]:field[1] + field[2]]), rng)
    elif kind == "txn":            # a transaction the parser rejects: no signatures, or a fee payer that is read-only
        q[field[1] + rng.choice((0, 1 + 64 * q[field[1]] + 1))] = rng.choice((0, 0x7F, 0xFF))
    elif kind == "txn_cut":        # the bytes behind the transaction (the wallclock) cut short or away
        end = field[1] + field[2]
        del q[end:end + rng.randrange(1, 9)]
    return kind, bytes(q)


def mutated(oracle, count, seed, me):
    """[(name, bytes)]: count seeded mutations of valid packets; me: the own identity's Peer"""
    rng = random.Random(seed)
    base = valid_packets(oracle, seed, me)
    # and of the gossip port's control packets, which this front leaves alone: a ping, a pong, prunes
    base += [(name, Other(p)) for name, proto, p in control_packets(oracle, seed, me.pub, prune_ms=range(8)) if proto == 0]
    out = []
    for _ in range(count):
        name, p = base[rng.randrange(len(base))]
        kind, q = mutate(rng, p)
        out.append((f"{name}:{kind}", q))
    return out


@functools.lru_cache(maxsize=None)
def fixture():
    """the reference-judged packets of tests/golden/crds.npz: (self_key,
    [dict(pkt, decodes, crds_len, vals=[(data discriminant, re-encoded bytes, equal to the received run)])])"""
    d = load_golden("crds")
    buf, ebuf, at, eat, vat, out = d["pkts"].tobytes(), d["enc"].tobytes(), 0, 0, 0, []
    for sz, ok, n in zip(d["sz"], d["decodes"], d["crds_len"]):
        vals = []
        for k in range(vat, vat + (int(n) if ok else 0)):
            esz = int(d["enc_sz"][k])
            vals.append((int(d["val_disc"][k]), ebuf[eat:eat + esz], bool(d["enc_equal"][k])))
            eat += esz
        vat += len(vals)
        out.append({"pkt": buf[at:at + int(sz)], "decodes": bool(ok), "crds_len": int(n), "vals": vals})
        at += int(sz)
    assert at == len(buf) and vat == len(d["val_disc"])
    return d["self_key"].tobytes(), out


@functools.lru_cache(maxsize=None)
def _rule_cases(oracle):
    me, pr, ot = Peer(oracle, 211), Peer(oracle, 223), Peer(oracle, 227)
    c = []

    def add(name, p, pkt_code, val_codes=()):
        c.append((name, bytes(p), me.pub, pkt_code, tuple(val_codes)))

    def patched(p, at, b):
        return p[:at] + b + p[at + len(b):]

    for name, d in pr.every_variant():
        for disc, kind in ((PUSH, "push"), (PULL_RESP, "pull")):
            p = packet(pr, [d], disc)
            add(f"{kind}_{name}", p, model.OK, [model.UNSUPPORTED if d[0] == 11 else model.OK])
        add(f"{name}_short", p[:-1], model.ERR_PARSE)
        add(f"{name}_long", p + b"\0", model.ERR_PARSE)
        add(f"{name}_wrong_signer", packet(pr, [d], signers=[ot]), model.OK,
            [model.UNSUPPORTED if d[0] == 11 else model.ERR_SIGNATURE])
        for j, (kind, at, sz) in enumerate(p.fields):
            if kind == "len64":
                n, = struct.unpack_from("<Q", p, at)
                for v in (n + 1, 2 ** 59 + 1, 2 ** 64 - 1):
                    add(f"{name}_len64_{j}_{v:#x}", patched(p, at, u64(v)), model.ERR_PARSE)
            elif kind == "tag":
                for v in (2, 0xFF):
                    add(f"{name}_tag_{j}_{v:#x}", patched(p, at, bytes([v])), model.ERR_PARSE)
            elif kind == "enum":
                add(f"{name}_enum_{j}_2", patched(p, at, u32(2)), model.ERR_PARSE)
            elif kind == "cu16":
                v = model.compact_u16(model.Cursor(p[at:at + sz]))
                if v < 0x80:
                    add(f"{name}_cu16_{j}_two_bytes", p[:at] + bytes([v | 0x80, 0]) + p[at + sz:], model.ERR_PARSE)
                if v < 0x4000:
                    add(f"{name}_cu16_{j}_three_bytes", p[:at] + bytes([v & 0x7F | 0x80, v >> 7 | 0x80, 0]) + p[at + sz:],
                        model.ERR_PARSE)
                add(f"{name}_cu16_{j}_over_long", p[:at] + bytes([0x80, 0x80, 4]) + p[at + sz:], model.ERR_PARSE)
            elif kind == "varint":
                b = p[at:at + sz]
                add(f"{name}_varint_{j}_zero_byte_behind", p[:at] + b[:-1] + bytes([b[-1] | 0x80, 0]) + p[at + sz:], model.ERR_PARSE)
                add(f"{name}_varint_{j}_eleven_bytes", p[:at] + bytes([0x80] * 10 + [1]) + p[at + sz:], model.ERR_PARSE)
                add(f"{name}_varint_{j}_top_bits_lost", p[:at] + bytes([0xFF] * 9 + [2]) + p[at + sz:], model.ERR_PARSE)
    p = packet(pr, [pr.contact_info_v2(wallclock=2 ** 64 - 1, addrs=(), sockets=0, ext=0)])
    add("contact_info_v2_varint_ten_bytes", p, model.OK, [model.UNSUPPORTED])
    for disc in range(14):
        d = pr.node_instance()
        p = packet(pr, [Data(u32(disc) + d[4:])])
        # 56 bytes of fields: no other variant's decoder ends there
        add(f"data_disc_{disc}", p, model.OK if disc == 8 else model.ERR_PARSE, [model.OK] if disc == 8 else [])
    for n in (0, 1, model.VAL_MAX):
        p = packet(pr, [pr.version(6) for _ in range(n)])
        add(f"crds_len_{n}", p, model.OK, [model.OK] * n)
        for v in (n + 1, 2 ** 59 + 1, 2 ** 64 - 1) + ((n - 1,) if n else ()):
            add(f"crds_len_{n}_as_{v:#x}", patched(p, 36, u64(v)), model.ERR_PARSE)
    assert len(p) == 44 + 115 * model.VAL_MAX <= model.MAX < len(p) + 115
    add("eleven_smallest_values", u32(PUSH) + pr.pub + u64(11) + p[44:] + p[44:44 + 115], model.ERR_PARSE)    # 1309 bytes
    add("eleven_in_1232", (u32(PUSH) + pr.pub + u64(11) + p[44:] + p[44:44 + 115])[:1232], model.ERR_PARSE)
    # contact_info_v2: the reference verifies its own re-encode under the message's pubkey, so whoever signed the
    # received bytes the value is not judged -- unless that pubkey is the own identity, which drops it first
    add("ci2_signed_by_outer", packet(pr, [ot.contact_info_v2()], signers=[pr]), model.OK, [model.UNSUPPORTED])
    add("ci2_signed_by_from", packet(pr, [ot.contact_info_v2()], signers=[ot]), model.OK, [model.UNSUPPORTED])
    add("own_outer_ci2", packet(me, [ot.contact_info_v2()], signers=[ot]), model.OK, [model.OWN])
    add("own_from_ci2", packet(pr, [me.contact_info_v2()], signers=[pr]), model.OK, [model.UNSUPPORTED])
    add("ci2_between", packet(pr, [pr.version(6), pr.contact_info_v2(), pr.node_instance()]), model.OK,
        [model.OK, model.UNSUPPORTED, model.OK])
    add("own_outer_other_values", packet(pr, [pr.version(7), ot.vote()], outer=me.pub, signers=[pr, ot]), model.OK,
        [model.OK, model.OK])
    for name, d in me.every_variant()[:-2]:
        add(f"own_{name}", packet(pr, [pr.node_instance(), d, pr.version(6)]), model.OK, [model.OK, model.OWN, model.OK])
    for bit, name in ((0, "first"), (255, "last")):
        key = bytearray(me.pub)
        key[bit // 8] ^= 1 << (bit % 8)
        c.append((f"self_key_{name}_bit", bytes(packet(me, [me.version(6)])), bytes(key), model.OK, (model.OK,)))
    # the vote's transaction: bytes behind it belong to the value, a rejected one fails the packet
    v = pr.vote()
    (_, t_at, t_sz), = v.fields
    add("vote_txn_no_signatures", packet(pr, [Data(v[:t_at] + b"\0" + v[t_at + 1:])]), model.ERR_PARSE)
    add("vote_wallclock_cut", packet(pr, [Data(v[:-3])]), model.ERR_PARSE)
    add("vote_wallclock_gone", packet(pr, [Data(v[:t_at + t_sz])]), model.ERR_PARSE)
    add("vote_then_value", packet(pr, [v, pr.node_instance()]), model.OK, [model.OK, model.OK])
    for disc in (0, 3, 4, 5):
        add(f"gossip_disc_{disc}", u32(disc) + pr.rand(128), model.UNSUPPORTED)
        add(f"gossip_disc_{disc}_alone", u32(disc), model.UNSUPPORTED)
    for disc in (6, 7, 0x102, 0xFFFFFFFF):
        add(f"gossip_disc_{disc:#x}", u32(disc) + packet(pr, [pr.version(6)])[4:], model.ERR_PARSE)
    for sz in (0, 1, 3):
        add(f"sz_{sz}", bytes([2, 0, 0][:sz]), model.ERR_PARSE)
    for sz in (4, 36, 43):
        add(f"push_sz_{sz}", packet(pr, [])[:sz], model.ERR_PARSE)
    add("sz_1233", u32(0) + bytes(1229), model.ERR_PARSE)
    big = packet(pr, [pr.duplicate_shred(1232 - 44 - 64 - 4 - 57 - 8)])
    assert len(big) == 1232
    add("sz_1232", big, model.OK, [model.OK])
    flip = bytearray(packet(pr, [pr.lowest_slot(2)]))
    flip[-1] ^= 1
    add("wallclock_bit", flip, model.OK, [model.ERR_SIGNATURE])
    assert len({n for n, _, _, _, _ in c}) == len(c)
    return tuple(c)


def rule_cases(oracle):
    """((name, packet, self_key, the packet's code, the values' codes after the verify), ...)"""
    return _rule_cases(oracle)
