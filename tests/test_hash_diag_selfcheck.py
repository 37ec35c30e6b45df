"""CPU checks of what tests/test_gpu_hash_diag.py is built from (the hash
case builders of tests/diag_util.py): the cases reach the block counts,
count edges, whole-message blocks, stream-length residues and byte shifts
the GPU tests claim, every message has its filler on both sides, no two
cases overlap and every case passes the entry point's own bounds rule.
Block counts are FIPS 180-4's padding rule (0x80, zeros, the length:
ceil((bytes + 17) / 128) for SHA-512, ceil((bytes + 9) / 64) for SHA-256),
not the device code.  Also the host-side bound on message sizes
(fd_ed25519_hip_private_msg_sz_check).  No GPU."""
import ctypes
import hashlib

import numpy as np
import pytest

import diag_util as du
import fec_model
import shred_model

INVAL = -22


@pytest.fixture(scope="module")
def sweeps():
    return {op: du.sha512_sweep(op) for op in du.SHA512_OPS}


def test_block_formulas_are_fips_180_4():
    # SHA-512: 111 message bytes + 0x80 + 16 length bytes fill one block, 112 need two
    assert [du.sha512_blocks(t) for t in (0, 111, 112, 239, 240)] == [1, 1, 2, 2, 3]
    # SHA-256: 55 + 0x80 + 8 fill one block
    assert [du.sha256_blocks(t) for t in (0, 55, 56, 119, 120)] == [1, 1, 2, 2, 3]
    assert du.sha512_full_blocks(64, 0) == 0 and du.sha512_full_blocks(64, 191) == 0
    assert du.sha512_full_blocks(64, 192) == 1 and du.sha512_full_blocks(32, 96 + 256) == 2


def test_hashlib_is_the_reference_it_claims():
    """FIPS 180-4's "abc" vectors"""
    assert hashlib.sha256(b"abc").hexdigest() == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"
    assert hashlib.sha512(b"abc").hexdigest() == (
        "ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a"
        "2192992a274fc1a836ba3c23a3feebbd454d4423643ce80e2a9ac94fa54ca49f")


def test_prefix_constants():
    assert du.LEAF_PREFIX == shred_model.LEAF == fec_model.LEAF == b"\x00SOLANA_MERKLE_SHREDS_LEAF"
    assert du.NODE_PREFIX == shred_model.NODE == fec_model.NODE == b"\x01SOLANA_MERKLE_SHREDS_NODE"
    assert len(du.LEAF_PREFIX) == len(du.NODE_PREFIX) == 26


@pytest.mark.parametrize("op", list(du.SHA512_OPS))
def test_sha512_sweep_reaches_what_it_claims(sweeps, op):
    pre = du.SHA512_OPS[op]
    _, cases = sweeps[op]
    have = {(c["sz"], c["shift"]) for c in cases}
    assert {(sz, sh) for sz in range(601) for sh in range(4)} <= have
    assert {(sz, sh) for sz in (1232, 1233, 65535, 65536, 65537) for sh in range(4)} <= have
    counts = {(du.sha512_blocks(pre + c["sz"]), c["shift"]) for c in cases}
    assert {(b, sh) for b in range(1, 6) for sh in range(4)} <= counts
    # both sides of every count edge: the last size of b blocks and the first of b + 1
    edges = [128 * b - 17 - pre for b in range(1, 6)]
    assert edges == ([47, 175, 303, 431, 559] if pre == 64 else [79, 207, 335, 463, 591])
    for e in edges:
        assert du.sha512_blocks(pre + e) + 1 == du.sha512_blocks(pre + e + 1)
        assert {(e, sh) for sh in range(4)} | {(e + 1, sh) for sh in range(4)} <= have
    # blocks that are message from end to end: none, one, two or more in a row, at every shift
    full = {(min(du.sha512_full_blocks(pre, c["sz"]), 2), c["shift"]) for c in cases if c["sz"] <= 600}
    assert full == {(k, sh) for k in range(3) for sh in range(4)}
    kinds = {c["note"] for c in cases}
    assert kinds == {"zero", "ones", "random"}
    for c in cases:
        if c["note"] != "random":
            assert set(c["opnd"]) == {0 if c["note"] == "zero" else 0xffffffff} and len(c["opnd"]) == pre // 4
    # the shuffle is a permutation with divergent waves; the sorted order has near-uniform ones
    sh = du.shuffled(cases)
    assert sorted(map(id, sh)) == sorted(map(id, cases)) and sh != cases
    per = du.hash_per_block(op)
    spread = lambda cs: [max(c["sz"] for c in cs[i:i + per]) - min(c["sz"] for c in cs[i:i + per])  # noqa: E731
                         for i in range(0, 4 * 601 - per, per)]     # the blocks of sizes 0..600 alone
    assert max(spread(cases)) <= per // 4 and min(spread(sh)) > 128


def test_sha256_sweeps_reach_what_they_claim():
    _, cases = du.sha256_bytes_sweep()
    assert {(c["sz"], c["shift"]) for c in cases} == {(sz, sh) for sz in range(1, 301) for sh in range(4)}
    assert {(c["sz"] % 64, c["shift"]) for c in cases} == {(r, sh) for r in range(64) for sh in range(4)}
    _, cases = du.sha256_leaf_sweep()
    have = {(c["sz"], c["shift"]) for c in cases}
    assert {(sz, sh) for sz in range(38, 301) for sh in range(4)} <= have
    assert {(1115 - 20 * d + x, sh) for d in range(16) for x in (0x18, 0x19) for sh in range(4)} <= have
    for lo, hi in ((38, 300), (800, 1200)):     # the sweep, and the real sizes on their own (14 of the 64)
        res = {((26 + c["sz"]) % 64, c["shift"]) for c in cases if lo <= c["sz"] <= hi}
        assert (res == {(r, sh) for r in range(64) for sh in range(4)}) == (lo == 38)
    assert {du.sha256_blocks(26 + c["sz"]) for c in cases if c["sz"] <= 300} == {2, 3, 4, 5, 6}
    _, nodes, pairs = du.sha256_node_sweep()
    assert len(nodes) == len(pairs) == len(du.CHILD_CLASSES) ** 2 * 4 * 2
    assert {(c["shift"], c["flag"]) for c in nodes} == {(sh, r) for sh in range(4) for r in (0, 1)}
    for nd, pr in zip(nodes, pairs):
        assert nd["want"] == pr["want"] and len(nd["opnd"]) == 5 and len(pr["opnd"]) == 10
        assert (pr["opnd"][5:] if nd["flag"] else pr["opnd"][:5]) == nd["opnd"]


def all_layouts(sweeps):
    yield from ((op,) + tuple(sweeps[op]) for op in du.SHA512_OPS)
    for op in ("sha512_ram", "sha512_ram_2w"):
        buf, cases, _ = du.sha512_wave_compositions(op)
        yield op, buf, cases
    for n in (1, 31, 33, 65):
        for last in ("longest", "shortest"):
            yield ("sha512_ram_2w",) + tuple(du.sha512_dead_lane_cases(n, last))
    yield ("sha256_bytes",) + tuple(du.sha256_bytes_sweep())
    yield ("sha256_leaf",) + tuple(du.sha256_leaf_sweep())
    buf, nodes, pairs = du.sha256_node_sweep()
    yield "sha256_node", buf, nodes
    yield "sha256_node_pair", buf, pairs


def test_layouts_keep_their_filler_and_bounds(sweeps):
    for op, buf, cases in all_layouts(sweeps):
        assert all(c["op"] == op for c in cases)
        size = buf.size()
        assert size <= du.HASH_MAX_BUF and len(cases) <= du.HASH_MAX_N
        assert all(du.hash_bounds_ok(c, size) for c in cases), op
        if op == "sha256_node_pair":
            continue
        # what a case reads as its message: [off, off + sz), the leaf's data 64 bytes on
        skip = 64 if op == "sha256_leaf" else 0
        spans = sorted((c["off"] + skip, c["off"] + skip + c["sz"]) for c in cases)
        assert spans == sorted(buf.spans), op
        assert spans[0][0] >= du.HASH_PAD and spans[-1][1] + du.HASH_PAD <= size
        for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
            assert a0 <= a1 and a1 + du.HASH_PAD <= b0, op       # disjoint, 16 bytes of filler between
        assert all(c["off"] % 4 == c["shift"] for c in cases)
        if op == "sha256_leaf":     # the 26 bytes the function loads and replaces, and the filler before them
            lead = sorted(buf.spans)
            for (a0, a1), (b0, b1) in zip([(0, 0)] + lead, lead):
                assert a1 + du.HASH_PAD <= b0 - 26
        # both fillers give the same message bytes, and only those
        z, f = buf.bytes(0x00), buf.bytes(0xff)
        same = z == f
        assert int(same.sum()) == sum(b - a for a, b in spans)
        for a, b in spans[:50] + spans[-50:]:
            assert same[a:b].all() and not same[a - du.HASH_PAD:a].any() and not same[b:b + du.HASH_PAD].any()


def test_wave_compositions_are_whole_blocks():
    for op, per, lanes in (("sha512_ram", 64, (0, 31, 32, 63)), ("sha512_ram_2w", 32, (0, 15, 31))):
        _, cases, names = du.sha512_wave_compositions(op)
        assert len(cases) == per * len(names)
        blocks = {names[i]: [c["sz"] for c in cases[per * i:per * i + per]] for i in range(len(names))}
        for sz in (0, 47, 48, 304):
            assert blocks[f"all lanes {sz} bytes"] == [sz] * per
        up = blocks["ascending with the lane"]
        assert up == sorted(up) and up[0] == 0 and up[-1] == 600 and len(set(up)) == per
        assert blocks["descending with the lane"] == up[::-1]
        for at in lanes:
            assert blocks[f"one 600-byte lane at {at} among empty messages"] == [600 * (l == at) for l in range(per)]
            assert blocks[f"one empty message at lane {at} among 600-byte ones"] == [600 * (l != at) for l in range(per)]
        assert cases[-1]["sz"] == 0     # case n - 1 adds no block to any two-wave composition
    for n in (1, 31, 33, 65):
        for last, pick in (("longest", max), ("shortest", min)):
            _, cases = du.sha512_dead_lane_cases(n, last)
            tail = [c["sz"] for c in cases[(n - 1) // 32 * 32:]]
            assert len(cases) == n and tail[-1] == pick(tail) and (len(tail) == 1 or tail.count(tail[-1]) == 1)


def test_host_entry_points_bound_the_message_size():
    """the device hashes are wrong from 2^31 bytes on ((int)sz - p): the
    host-buffer entry points refuse such a size before they stage anything.
    The check is a host function of its own: no engine, no allocation, and
    no 2 GiB message."""
    from firedancer_amd import ed25519
    f = ed25519.library().fd_ed25519_hip_private_msg_sz_check
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_ulong], ctypes.c_int
    ok = np.array([0, 1232, 2**31 - 1], np.uint32)
    assert f(ok.ctypes.data, len(ok)) == 0
    for big in (2**31, 2**31 + 1, 2**32 - 1):
        for at in range(3):
            sz = ok.copy()
            sz[at] = big
            assert f(sz.ctypes.data, len(sz)) == INVAL
            assert f(sz.ctypes.data, at) == 0          # only the first n sizes are read
    assert f(None, 0) == 0 and f(None, 1) == INVAL
