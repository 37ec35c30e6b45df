"""Makes tests/golden/shreds.npz from the reference's own shred capture:

    python tests/golden/gen_shreds.py <reference>/src/disco/shred/fixtures

demo-shreds.pcap holds 480 UDP packets of one Merkle shred each (7 FEC
sets: 240 data shreds of 1203 bytes, 240 code shreds of 1228), all signed
with demo-shreds.key, whose second half is the leader's public key.  The
fixture keeps the shreds back to back with their sizes, and that key.  It
is data the reference's shred tests read; nothing here is run by a test."""
import os
import struct
import sys

import numpy as np

NET_HDR = 14 + 20 + 8   # Ethernet, IPv4 without options, UDP


def shreds_of(pcap):
    magic, = struct.unpack_from("<I", pcap, 0)
    assert magic in (0xA1B2C3D4, 0xA1B23C4D), hex(magic)
    pos, out = 24, []
    while pos < len(pcap):
        _, _, incl, orig = struct.unpack_from("<IIII", pcap, pos)
        assert incl == orig
        out.append(pcap[pos + 16 + NET_HDR:pos + 16 + incl])
        pos += 16 + incl
    return out


def main(fixtures):
    shreds = shreds_of(open(os.path.join(fixtures, "demo-shreds.pcap"), "rb").read())
    key = open(os.path.join(fixtures, "demo-shreds.key"), "rb").read()
    assert len(key) == 64 and len(shreds) == 480
    sz = np.array([len(s) for s in shreds], np.uint32)
    assert sorted(set(sz.tolist())) == [1203, 1228]
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shreds.npz")
    np.savez_compressed(out, shreds=np.frombuffer(b"".join(shreds), np.uint8), sz=sz,
                        pubkey=np.frombuffer(key[32:], np.uint8))
    print(out, os.path.getsize(out), "bytes,", len(shreds), "shreds")


if __name__ == "__main__":
    main(sys.argv[1])
