"""Test helper: transactions carrying Ed25519 precompile instructions, with
offsets tables built from a list of entries -- right ones and deliberately
wrong ones -- and the case sets the CPU and GPU precompile tests share."""
import random
import struct

from precompile_model import ED25519_ID
from txn_util import Signer, message, mutate, txn

THIS = 0xFFFF
OTHER_PROG = bytes(range(100, 132))


def entry(sig_off, sig_idx, pub_off, pub_idx, msg_off, msg_sz, msg_idx):
    return struct.pack("<7H", sig_off, sig_idx, pub_off, pub_idx, msg_off, msg_sz, msg_idx)


def instr_data(entries, cnt=None, pad=0, tail=b""):
    """cnt byte (default: len(entries)), the ignored byte, the 14-byte entries, anything behind them"""
    return bytes([len(entries) if cnt is None else cnt, pad]) + b"".join(entries) + bytes(tail)


class Builder:
    """One transaction: a fee payer, the Ed25519 program (account 1) and
    another program (account 2); instructions added in order."""

    def __init__(self, signer, v0=False, accts=None):
        self.signer, self.v0 = signer, v0
        self.payer = signer.key()
        self.accts = [self.payer[1], ED25519_ID, OTHER_PROG] if accts is None else [self.payer[1]] + accts
        self.instrs = []

    def signed(self, msg, flip=False):
        """(sig, pub, msg) the reference accepts; flip: a message bit flipped after signing"""
        priv, pub = self.signer.key()
        sig = self.signer.sign(bytes(msg), priv, pub)
        if flip:
            msg = bytes([msg[0] ^ 1]) + bytes(msg[1:])
        return sig, pub, bytes(msg)

    def add(self, data, prog=1, accts=(0,)):
        self.instrs.append((prog, list(accts), bytes(data)))
        return len(self.instrs) - 1

    def add_inline(self, triples, prog=1, pad=0, idx=THIS, tail=b""):
        """one instruction holding its own table and every (sig, pub, msg) behind it"""
        at, blob, ents = 2 + 14 * len(triples), b"", []
        for sig, pub, msg in triples:
            o = at + len(blob)
            ents.append(entry(o, idx, o + 64, idx, o + 96, len(msg), idx))
            blob += sig + pub + msg
        return self.add(instr_data(ents, pad=pad, tail=blob + tail), prog=prog)

    def build(self):
        luts = [(bytes(range(32)), [0, 1], [2])] if self.v0 else ()
        m = message(1, self.accts, ro_unsigned=len(self.accts) - 1, instrs=self.instrs, version=0 if self.v0 else None,
                    luts=luts)
        return txn([self.signer.sign(m, *self.payer)], m)


def rule_cases(oracle, seed=7):
    """[(name, payload)]: one transaction per edge of the rules"""
    sg = Signer(oracle, seed)
    out = []

    def case(name, fill, v0=False, accts=None):
        b = Builder(sg, v0=v0, accts=accts)
        fill(b)
        out.append((name, b.build()))

    # P1: short data
    for dsz, d0 in ((0, 0), (1, 0), (2, 0), (2, 1), (3, 0), (15, 1), (16, 1)):
        case(f"data_sz{dsz}_d{d0}", lambda b, dsz=dsz, d0=d0: b.add((bytes([d0]) + bytes(15))[:dsz]))
    # P2: cnt and the table's size
    case("cnt0_sz16", lambda b: b.add(bytes(16)))
    case("cnt0_sz40", lambda b: b.add(bytes(40)))

    def table_fits(b, short):
        t = [b.signed(b"fits-0"), b.signed(b"fits-1")]
        store = b.add(b"".join(s + p + m for s, p, m in t), prog=2)
        ents = [entry(102 * i, store, 102 * i + 64, store, 102 * i + 96, 6, store) for i in range(2)]
        b.add(instr_data(ents)[:30 - short])
    case("table_exact", lambda b: table_fits(b, 0))
    case("table_one_short", lambda b: table_fits(b, 1))
    case("pad_byte_nonzero", lambda b: b.add_inline([b.signed(b"pad")], pad=0xA5))
    # P3: instruction indices
    case("idx_this", lambda b: b.add_inline([b.signed(b"this")]))
    case("idx_own", lambda b: (b.add(b"x", prog=2), b.add_inline([b.signed(b"own")], idx=1)))

    def other(b, idx):
        s, p, m = b.signed(b"another instruction's data")
        b.add(s + p + m, prog=2)
        b.add(instr_data([entry(0, idx[0], 64, idx[1], 96, len(m), idx[2])], tail=bytes(120)))
    case("idx_other", lambda b: other(b, (0, 0, 0)))
    for which in range(3):
        for bad, name in ((2, "instr_cnt"), (0xFFFE, "fffe")):
            case(f"idx_{name}_{'spm'[which]}", lambda b, which=which, bad=bad:
                 other(b, tuple(bad if q == which else 0 for q in range(3))))
    # P3: offset + size against the data's size

    def bound(b, which, over):
        s, p, m = b.signed(b"bound")
        blobs, o = [s, p, m], [16, 80, 112]
        body = s + p + m + blobs[which]      # a second copy of the item at the very end of the data
        o[which] = 16 + len(body) - len(blobs[which]) + over
        b.add(instr_data([entry(o[0], THIS, o[1], THIS, o[2], len(m), THIS)]) + body)
    for which in range(3):
        case(f"bound_eq_{'spm'[which]}", lambda b, which=which: bound(b, which, 0))
        case(f"bound_over_{'spm'[which]}", lambda b, which=which: bound(b, which, 1))
    case("msg_sz0", lambda b: b.add_inline([b.signed(b"")]))
    case("msg_sz0_at_end", lambda b: (lambda s, p, m: b.add(instr_data([entry(16, THIS, 80, THIS, 112, 0, THIS)]) + s + p))(
        *b.signed(b"")))

    def overlap_sig(b):
        s, p, m = b.signed(b"overlaps")
        b.add(instr_data([entry(16, THIS, 80, THIS, 40, 48, THIS)]) + s + p + m)   # message = sig[24:] || pub[:8]
    case("msg_overlaps_sig", overlap_sig)

    def overlap_pub(b):
        priv, pub = b.signer.key()
        m = pub + b"|tail"
        s = b.signer.sign(m, priv, pub)
        b.add(instr_data([entry(16, THIS, 80, THIS, 80, len(m), THIS)]) + s + m)   # the message starts with the key
    case("msg_overlaps_pub", overlap_pub)

    def shared(b):
        s, p, m = b.signed(b"shared")
        e = entry(30, THIS, 94, THIS, 126, len(m), THIS)
        b.add(instr_data([e, e]) + s + p + m)
    case("two_entries_one_sig", shared)
    # which instructions count
    case("other_program_same_data", lambda b: b.add_inline([b.signed(b"ignored", flip=True)], prog=2))
    case("other_program_bad_header", lambda b: b.add(bytes(5), prog=2))
    case("id_listed_other_named", lambda b: (b.add(bytes(7), prog=2), b.add_inline([b.signed(b"ok")], prog=1)))
    case("no_ed25519_account", lambda b: b.add(bytes(7), prog=1), accts=[OTHER_PROG, bytes(32)])

    def many(b):
        for _ in range(62):
            b.add(b"", prog=2, accts=())
        s, p, m = b.signed(b"63")
        b.add(instr_data([entry(0, 63, 64, 63, 96, len(m), 63)]), accts=())
        b.add(s + p + m, prog=2, accts=())
    case("instr64_lookup63", many)
    case("legacy_two_entries", lambda b: b.add_inline([b.signed(b"one"), b.signed(b"two" * 30)]))
    case("v0_luts", lambda b: (b.add(b"\x01\x02", prog=2), b.add_inline([b.signed(b"v0"), b.signed(b"v0-2")])), v0=True)
    case("v0_bad_sig", lambda b: b.add_inline([b.signed(b"v0"), b.signed(b"v0-bad", flip=True)]), v0=True)
    ok = out[-2][1]
    out.append(("rejected_trailing", ok + b"\0"))
    out.append(("rejected_truncated", ok[:-1]))
    out.append(("rejected_empty", b""))
    # priority
    good, flip = (lambda b: b.signed(b"good")), (lambda b: b.signed(b"flipped", flip=True))

    def two(b, first_bad_sig):
        t = [flip(b) if first_bad_sig else good(b), good(b) if first_bad_sig else flip(b)]
        blob = b"".join(s + p + m for s, p, m in t)
        at, ents = 30, []
        for i, (s, p, m) in enumerate(t):
            bad_off = (i == 1) == first_bad_sig      # the other entry's signature lies past the data
            ents.append(entry(2000 if bad_off else at, THIS, at + 64, THIS, at + 96, len(m), THIS))
            at += 96 + len(m)
        b.add(instr_data(ents) + blob)
    case("prio_sig_then_offset", lambda b: two(b, True))
    case("prio_offset_then_sig", lambda b: two(b, False))
    case("prio_second_instr_fails", lambda b: (b.add_inline([good(b)]), b.add(b"\0", prog=2), b.add_inline([flip(b)])))
    case("prio_both_instr_fail", lambda b: (b.add_inline([good(b), flip(b)]), b.add(bytes(3))))
    case("prio_header_then_sig", lambda b: (b.add(bytes(3)), b.add_inline([flip(b)])))
    case("prio_sig_then_header", lambda b: (b.add_inline([flip(b)]), b.add(bytes(3))))
    return out


def valid_txns(oracle, seed=11, n=20):
    """n transactions whose precompile instructions all pass: inline and cross-instruction tables"""
    sg, rng, out = Signer(oracle, seed), random.Random(seed), []
    for i in range(n):
        b = Builder(sg, v0=i % 3 == 2)
        for _ in range(1 + i % 2):
            if rng.random() < 0.5:
                b.add(bytes(rng.getrandbits(8) for _ in range(rng.randrange(20))), prog=2)
            b.add_inline([b.signed(bytes(rng.getrandbits(8) for _ in range(rng.randrange(1, 60))))
                          for _ in range(1 + rng.randrange(3))])
        if i % 4 == 1:
            s, p, m = b.signed(b"cross")
            store = b.add(s + p + m, prog=2)
            b.add(instr_data([entry(0, store, 64, store, 96, len(m), store)], tail=bytes(4)))
        out.append(b.build())
    return out


def mutated(oracle, seed=13, per=100):
    """about 2,000 structural mutations (one or two steps) of valid precompile transactions"""
    rng, out = random.Random(seed), []
    for p in valid_txns(oracle, seed):
        for k in range(per):
            q = mutate(rng, p)
            out.append(mutate(rng, q) if k % 4 == 3 else q)
    return out


def max_entries_txn(oracle, seed=17):
    """One one-signer legacy transaction with two accounts carrying the most
    entries a 1232-byte payload holds, all aliasing one signature, key and
    message; returns (payload, entries)."""
    sg = Signer(oracle, seed)
    b = Builder(sg, accts=[ED25519_ID])
    s, p, m = b.signed(b"m")
    n = 0
    while True:
        at = 2 + 14 * (n + 1)
        data = instr_data([entry(at, THIS, at + 64, THIS, at + 96, len(m), THIS)] * (n + 1)) + s + p + m
        b.instrs = [(1, [], data)]
        if len(b.build()) > 1232:
            break
        n += 1
    at = 2 + 14 * n
    b.instrs = [(1, [], instr_data([entry(at, THIS, at + 64, THIS, at + 96, len(m), THIS)] * n) + s + p + m)]
    return b.build(), n
