"""Hostile input to the CRDS rules: fd_crds_core.h compiled with a stand-alone
main (tests/crds_walk_main.c) under ASan and UBSan, run on the
reference-judged fixture, rule-edge and mutated packets and on every prefix of
one packet per variant, held in heap blocks of exactly their size.  A program
of its own: nothing is loaded into this interpreter."""
import struct
import subprocess

import pytest

import san_build
from crds_util import Peer, fixture, mutated, packet, rule_cases

FIELDS = ("disc", "pre", "sig_off", "key_off", "msg_off", "msg_sz")


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    return san_build.build("crds_walk_main.c", tmp_path_factory.mktemp("crds_walk") / "crds_walk")


def test_walk_of_hostile_packets_is_clean_and_agrees_with_the_library(walker, oracle, tmp_path):
    from firedancer_amd import ed25519 as ed
    self_key, fx = fixture()
    me, pr = Peer(oracle, 239), Peer(oracle, 257)
    packets = [(self_key, f["pkt"]) for f in fx]                                         # (identity, packet)
    packets += [(key, p) for _, p, key, _, _ in rule_cases(oracle)]
    packets += [(me.pub, p) for _, p in mutated(oracle, 2000, 241, me)]
    # and every prefix of one packet per variant, a value of another variant behind it
    for _, d in pr.every_variant():
        p = packet(pr, [d, pr.version(7, True)])
        packets += [(me.pub, p[:k]) for k in range(len(p))]
    path = tmp_path / "packets.bin"
    path.write_bytes(struct.pack("<I", len(packets)) + b"".join(key + struct.pack("<I", len(p)) + p for key, p in packets))
    r = subprocess.run([walker, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = iter(r.stdout.split("\n")[:-1])
    for key, p in packets:
        code, vals = ed.crds_plan(p, key)
        assert [int(x) for x in next(lines).split()] == [code, len(vals)], p[:80].hex()
        for v in vals:
            assert [int(x) for x in next(lines).split()] == [int(v[f]) for f in FIELDS], p[:80].hex()
    assert next(lines, None) is None
