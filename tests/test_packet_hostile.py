"""Hostile input to the gossip and repair packet rules: fd_packet_core.h
compiled with a stand-alone main (tests/packet_walk_main.c) under ASan and
UBSan, run on the reference-judged fixture, rule-edge, mutated and truncated
packets held in heap blocks of exactly their size.  A program of its own:
nothing is loaded into this interpreter."""
import struct
import subprocess

import pytest

import san_build
from packet_util import Node, fixture, mutated, rule_cases, valid_packets

FIELDS = ("disc", "key_off", "sig_off", "msg0_off", "msg0_sz", "msg1_off", "msg1_sz")


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    return san_build.build("packet_walk_main.c", tmp_path_factory.mktemp("packet_walk") / "packet_walk")


def test_walk_of_hostile_packets_is_clean_and_agrees_with_the_library(walker, oracle, tmp_path):
    from firedancer_amd import ed25519 as ed
    self_key, fx = fixture()
    me = Node(oracle, 89).pub
    packets = [(self_key, f["proto"], f["pkt"]) for f in fx]                            # (identity, protocol, packet)
    packets += [(key, proto, p) for _, proto, p, key, _ in rule_cases(oracle)]
    packets += [(me, proto, p) for _, proto, p in mutated(oracle, 2000, 97, me)]
    # and every prefix of one valid packet of each kind (a prune of 3 origins)
    for _, proto, p in valid_packets(oracle, 101, me, prune_ms=(3,)):
        packets += [(me, proto, p[:k]) for k in range(len(p))]
    path = tmp_path / "packets.bin"
    path.write_bytes(struct.pack("<I", len(packets)) +
                     b"".join(key + struct.pack("<BI", proto, len(p)) + p for key, proto, p in packets))
    r = subprocess.run([walker, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(packets)
    for (key, proto, p), line in zip(packets, lines):
        code, pl = ed.packet_plan(proto, p, key)
        assert [int(x) for x in line.split()] == [code] + [int(pl[f]) for f in FIELDS], (proto, p[:80].hex(), line)
