"""Makes tests/golden/crds.npz: gossip pull responses and push messages with
the reference decoder's and encoder's own account of each.

    python tests/golden/gen_crds.py <reference>/src

The packets come from tests/crds_util.py (signed with the CPU oracle,
oracle/liboracle_ed25519.so): valid push messages and pull responses of every
fd_crds_data variant alone and mixed, every crds_len 0..VAL_MAX, values under
the caller's own identity, a contact_info_v2 signed by its own `from` and one
signed by the message's pubkey, the control packets of tests/packet_util.py
(which this front leaves alone), and seeded mutations -- truncation and
extension by one byte and by more, every message and data discriminant 0..13,
crds_len and every inner length +- 1, 2^59+1 and 2^64-1, option tags 2 and
0xff, non-minimal and over-long compact-u16 and varint in every such field,
inner enum discriminants, a vote whose transaction the parser rejects and one
with the bytes behind it cut, bit flips.
gen_crds_ref.c, this project's own harness, is compiled in a temporary
directory against the reference's sources as gen_packets.py compiles its
harness, and records for each packet whether fd_gossip_msg_decode succeeded
and consumed every byte, the discriminant and crds_len, and for every decoded
value its data discriminant, the bytes of fd_crds_data_encode and whether
they equal the received run.  Nothing here is run by a test."""
import collections
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

MUTATIONS, SEED = 2200, 131
SIZE_LIMIT = 1 << 20    # of a committed file


def judge_with_reference(ref, packets):
    """[(decodes, disc, crds_len, [(data discriminant, equal, re-encoded bytes)])] of [packet]"""
    from gen_packets import REF_C, ref_defs
    with tempfile.TemporaryDirectory() as tmp:
        exe, objs = os.path.join(tmp, "gen_crds_ref"), []
        for src in REF_C + [os.path.join(HERE, "gen_crds_ref.c")]:
            obj = os.path.join(tmp, os.path.basename(src)[:-2] + ".o")
            subprocess.run(["gcc"] + ref_defs(ref) + ["-march=haswell", "-O1", "-c", os.path.join(ref, src), "-o", obj], check=True)
            objs.append(obj)
        subprocess.run(["gcc", "-pthread", "-o", exe] + objs + ["-lm"], check=True)
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<I", len(packets)) + b"".join(struct.pack("<I", len(p)) + p for p in packets))
        subprocess.run([exe, fin, fout], check=True)
        raw, at, out = open(fout, "rb").read(), 0, []
        for _ in packets:
            ok, disc, n = struct.unpack_from("<BIQ", raw, at)
            at += 13
            vals = []
            for _ in range(n):
                vdisc, equal, esz = struct.unpack_from("<IBI", raw, at)
                vals.append((vdisc, equal, raw[at + 9:at + 9 + esz]))
                at += 9 + esz
            out.append((ok, disc, n, vals))
        assert at == len(raw)
        return out


def main(ref):
    import crds_model as model
    from conftest import _oracle
    from crds_util import Peer, mutated, valid_packets
    from packet_util import GOSSIP
    from packet_util import valid_packets as control_packets
    oracle = _oracle()
    me = Peer(oracle, SEED - 1)
    packets = [bytes(p) for _, p in valid_packets(oracle, SEED, me)]
    packets += [p for _, proto, p in control_packets(oracle, SEED, me.pub) if proto == GOSSIP]
    packets += [p for _, p in mutated(oracle, MUTATIONS, SEED, me)]
    verdicts = judge_with_reference(ref, packets)
    # what the generator itself holds to: every decoded value is compared, every code occurs 50 times, and the
    # re-encode differs from the received run for contact_info_v2 and for nothing else
    verify = model.verifier(oracle)
    pkt_codes, val_codes, differ = collections.Counter(), collections.Counter(), 0
    for p, (ok, disc, n, vals) in zip(packets, verdicts):
        code, judged = model.judge(verify, p, me.pub)
        pkt_codes[code] += 1
        val_codes.update(v[0] for v in judged)
        assert len(vals) == (n if ok and disc in (1, 2) else 0)
        differ += sum(not equal for _, equal, _ in vals)
        assert all(bool(equal) == (vdisc != 11) for vdisc, equal, _ in vals)
    print("packet codes", dict(pkt_codes), "value codes", dict(val_codes), "re-encodes that differ", differ)
    assert all(pkt_codes[c] >= 50 for c in (model.OK, model.ERR_PARSE, model.UNSUPPORTED)), pkt_codes
    assert all(val_codes[c] >= 50 for c in (model.OK, model.UNSUPPORTED, model.ERR_SIGNATURE, model.OWN)), val_codes
    vals = [v for _, _, _, vs in verdicts for v in vs]
    out = os.path.join(HERE, "crds.npz")
    np.savez_compressed(out, self_key=np.frombuffer(me.pub, np.uint8),
                        sz=np.array([len(p) for p in packets], np.uint32),
                        pkts=np.frombuffer(b"".join(packets), np.uint8),
                        decodes=np.array([v[0] for v in verdicts], np.uint8),
                        disc=np.array([v[1] for v in verdicts], np.uint32),
                        crds_len=np.array([v[2] for v in verdicts], np.uint64),
                        val_disc=np.array([v[0] for v in vals], np.uint32),
                        enc_equal=np.array([v[1] for v in vals], np.uint8),
                        enc_sz=np.array([len(v[2]) for v in vals], np.uint32),
                        enc=np.frombuffer(b"".join(v[2] for v in vals) or b"\0", np.uint8))
    size = os.path.getsize(out)
    print(out, size, "bytes,", len(packets), "packets,", sum(v[0] for v in verdicts), "decode,", len(vals), "values")
    assert size <= SIZE_LIMIT, size


if __name__ == "__main__":
    main(sys.argv[1])
