"""GPU: the host wrappers of the three fronts (fd_ed25519_hip_shreds_host,
_packets_host, _precompile_host) share one staging set in the engine (a pinned
and a device in block, out block, and a device workspace).  One engine, the
fronts in turn, so that each grows or reuses a buffer another front used
last; every result against the models of test_gpu_shreds.py,
test_gpu_packets.py and test_gpu_precompile.py.  A small engine: compact
tables, 512-signature chunks."""
import pytest

import packet_model
import precompile_model
import shred_model
import packet_util
import precompile_util
import shred_util
from packet_util import GOSSIP, REPAIR
from txn_util import ref_lib

pytestmark = pytest.mark.gpu


def pick(src, n):
    return [src[(7 * i + 3 * n) % len(src)] for i in range(n)]


def test_fronts_in_turn_on_one_engine(oracle):
    from firedancer_amd import ed25519 as ed

    # shreds: rule edges and captured shreds, each with its leader
    fx, fx_pub = shred_util.fixture()
    cases, case_pub = shred_util.rule_cases(oracle)
    shreds = [(s, case_pub) for _, s, _ in cases] + [(s, fx_pub) for s in fx]
    shred_verify = shred_model.verifier(oracle)

    def run_shreds(eng, n):
        batch = pick(shreds, n)
        want = [shred_model.judge(shred_verify, s, k) for s, k in batch]
        codes, roots = eng.shreds_host([s for s, _ in batch], [k for _, k in batch])
        assert codes.tolist() == [c for c, _ in want]
        assert [bytes(r) for r in roots] == [r if r else bytes(32) for _, r in want]
        return set(codes.tolist())

    # packets: rule edges, every valid kind and judged captures, under the fixture's identity
    self_key, pfx = packet_util.fixture()
    pkts = [(proto, p) for _, proto, p, _, _ in packet_util.rule_cases(oracle)] + \
        [(proto, p) for _, proto, p in packet_util.valid_packets(oracle, 103, self_key)]
    pkts = {proto: [p for pr, p in pkts if pr == proto] + [f["pkt"] for f in pfx if f["proto"] == proto][:150]
            for proto in (GOSSIP, REPAIR)}
    packet_verify = packet_model.verifier(oracle)

    def run_packets(eng, proto, n):
        batch = pick(pkts[proto], n)
        want = [packet_model.judge(packet_verify, proto, p, self_key)[0] for p in batch]
        assert eng.packets_host(proto, batch, self_key).tolist() == want
        return set(want)

    # precompile: three payloads with entries, a passing one and the two priority orders, with the
    # verdicts test_gpu_precompile.py pins for them -- the model's, where the reference is built
    named = dict(precompile_util.rule_cases(oracle))
    payloads = [named[k] for k in ("legacy_two_entries", "prio_sig_then_offset", "prio_offset_then_sig")]
    assert all(ed.precompile_count(p) >= 2 for p in payloads)
    judged = [(0, 0xFF), (-3, 0), (-4, 0)]
    ref = ref_lib()
    if ref is not None:
        assert [precompile_model.judge(ref, p)[:2] for p in payloads] == judged

    eng = ed.Engine(0, max_chunk=512, compact=True)
    try:
        assert 0 in run_shreds(eng, 65)
        assert 0 in run_packets(eng, GOSSIP, 64)
        codes, instr = eng.precompile_host(payloads)
        assert codes.tolist() == [j[0] for j in judged] and instr.tolist() == [j[1] for j in judged]
        assert len(run_packets(eng, REPAIR, 257)) >= 3
        assert len(run_shreds(eng, 257)) >= 3
    finally:
        eng.close()
