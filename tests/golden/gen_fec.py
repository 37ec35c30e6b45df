"""Makes tests/golden/fec.npz from the reference's shred fixtures:

    python tests/golden/gen_fec.py <reference>/src/disco/shred/fixtures

demo-shreds.key is the 64-byte keypair file that signed the shreds of
demo-shreds.pcap (tests/golden/shreds.npz): its first half is the leader's
private key, its second half the public key shreds.npz already holds.  The
fixture keeps the 32 private-key bytes, with which sealing the captured FEC
sets anew must reproduce the capture's signatures byte for byte.  It is data
the reference's shred tests read; nothing here is run by a test."""
import os
import sys

import numpy as np


def main(fixtures):
    key = open(os.path.join(fixtures, "demo-shreds.key"), "rb").read()
    assert len(key) == 64
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fec.npz")
    np.savez_compressed(out, privkey=np.frombuffer(key[:32], np.uint8))
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
