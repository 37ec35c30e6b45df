"""Makes tests/golden/packets.npz: signed gossip and repair control packets
with the reference decoder's own verdict on each.

    python tests/golden/gen_packets.py <reference>/src

The packets come from tests/packet_util.py (signed with the CPU oracle,
oracle/liboracle_ed25519.so): one valid packet of every kind both ports
decode, a prune message of every m 0..32, and seeded mutations -- truncation
and extension by one byte and by more, every discriminant 0..13 and random
ones, bit flips, another addressee, a change to a field no signature covers,
and for prunes m +- 1, 2^59+1 and 2^64-1.
gen_packets_ref.c, this project's own harness, is compiled in a temporary
directory against the reference's flamenco/types/fd_types.c,
util/scratch/fd_scratch.c, ballet/txn/fd_txn_parse.c and the util objects
and REF_DEFS of oracle/Makefile, and records for each packet whether
fd_gossip_msg_decode / fd_repair_protocol_decode succeeded and consumed every
byte, the decoded discriminant, and for a decoded prune message the bytes of
fd_gossip_prune_sign_data_encode.  Nothing here is run by a test."""
import os
import re
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))

REF_C = ["flamenco/types/fd_types.c", "util/scratch/fd_scratch.c", "ballet/txn/fd_txn_parse.c", "util/log/fd_log.c",
         "util/cstr/fd_cstr.c", "util/env/fd_env.c", "util/io/fd_io.c", "util/tile/fd_tile.c"]
MUTATIONS, SEED = 2400, 83


def ref_defs(ref):
    """REF_DEFS of oracle/Makefile, with this reference tree"""
    mk = open(os.path.join(REPO, "oracle", "Makefile")).read()
    defs = re.search(r"^REF_DEFS := ((?:.*\\\n)*.*)$", mk, re.M).group(1).replace("\\\n", " ").split()
    return [d.replace("$(REF)", ref) for d in defs]


def judge_with_reference(ref, packets):
    """[(decodes, disc, sign_data)] of [(proto, packet)]"""
    with tempfile.TemporaryDirectory() as tmp:
        exe, objs = os.path.join(tmp, "gen_packets_ref"), []
        for src in REF_C + [os.path.join(HERE, "gen_packets_ref.c")]:
            obj = os.path.join(tmp, os.path.basename(src)[:-2] + ".o")
            # -O1 after REF_DEFS' -O3: fd_types.c is 24,000 lines
            subprocess.run(["gcc"] + ref_defs(ref) + ["-march=haswell", "-O1", "-c", os.path.join(ref, src), "-o", obj], check=True)
            objs.append(obj)
        subprocess.run(["gcc", "-pthread", "-o", exe] + objs + ["-lm"], check=True)
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<I", len(packets)) + b"".join(struct.pack("<BI", pr, len(p)) + p for pr, p in packets))
        subprocess.run([exe, fin, fout], check=True)
        raw, at, out = open(fout, "rb").read(), 0, []
        for _ in packets:
            ok, disc, ssz = struct.unpack_from("<BII", raw, at)
            out.append((ok, disc, raw[at + 9:at + 9 + ssz]))
            at += 9 + ssz
        assert at == len(raw)
        return out


def main(ref):
    from conftest import _oracle
    from packet_util import Node, mutated, valid_packets
    oracle = _oracle()
    self_key = Node(oracle, SEED - 1).pub
    packets = [(pr, p) for _, pr, p in valid_packets(oracle, SEED, self_key)]
    packets += [(pr, p) for _, pr, p in mutated(oracle, MUTATIONS, SEED, self_key)]
    verdicts = judge_with_reference(ref, packets)
    out = os.path.join(HERE, "packets.npz")
    np.savez_compressed(out, self_key=np.frombuffer(self_key, np.uint8),
                        proto=np.array([pr for pr, _ in packets], np.uint8),
                        sz=np.array([len(p) for _, p in packets], np.uint32),
                        pkts=np.frombuffer(b"".join(p for _, p in packets), np.uint8),
                        decodes=np.array([v[0] for v in verdicts], np.uint8),
                        disc=np.array([v[1] for v in verdicts], np.uint32),
                        sign_data_sz=np.array([len(v[2]) for v in verdicts], np.uint32),
                        sign_data=np.frombuffer(b"".join(v[2] for v in verdicts) or b"\0", np.uint8))
    print(out, os.path.getsize(out), "bytes,", len(packets), "packets,", sum(v[0] for v in verdicts), "decode")


if __name__ == "__main__":
    main(sys.argv[1])
