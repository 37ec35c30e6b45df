"""The device SHA-512 and SHA-256 on chosen bytes, sizes, byte shifts and
lanes (libfd_ed25519_diag.so, diag/fd_ed25519_diag_hash.hip), against
hashlib: exact, every case checked.

A whole front only hashes the lengths, shifts and wave mixes its inputs
happen to have.  Here:

  * SHA-512, each of sha512_pre<8>, sha512_ram and the two-wave form: every
    size 0..600 at every byte shift (one to six blocks, both sides of every
    block-count edge for both prefix lengths, the FULL path of sha_build_w
    zero, one and two times in a row), plus 1232, 1233 and 65535..65537; in
    size order (near-uniform waves) and shuffled (divergent waves);
  * chosen wave compositions for the one-wave and the two-wave form: uniform
    sizes, sizes ascending and descending with the lane, one long lane among
    empty ones and the reverse, dead lanes in the last block;
  * SHA-256: every size 1..300 (sha256_bytes) and every leaf size 38..300
    plus the real ones (sha256_leaf) at every shift -- every residue of the
    stream length mod 64, where the padding splits across blocks -- and the
    Merkle node in both forms over operand classes at the 16-bit funnel
    shifts' edges.

Every digest test runs with 0x00 and with 0xff around each message (at
least 16 bytes on both sides): nothing outside [off, off + sz) reaches a
digest, not the masked tail dwords, not the skipped chunks, not the bytes in
front of a shifted start.  A failure names (op, sz, shift, lane, wave
composition).  tests/test_hash_diag_selfcheck.py checks on the CPU that the
builders cover what is claimed here."""
import random

import numpy as np
import pytest

import diag_util as du
from diag_util import HIP_ERROR_INVALID_VALUE, Diag

pytestmark = pytest.mark.gpu

FILLERS = (0x00, 0xff)


@pytest.fixture(scope="module")
def diag():
    return Diag()


_cache = {}


def cached(key, build):
    """a reference is computed once and shared, unchanged, among the tests"""
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def check(diag, op, buf, cases, filler, extra_rows=0):
    out = du.run_hash(diag, op, buf.bytes(filler), cases, extra_rows)
    bad = du.hash_mismatches(cases, out)
    assert not bad, f"filler {filler:#04x}: {len(bad)} of {len(cases)} digests differ from hashlib:\n" + "\n".join(bad[:12])
    n = len(cases)
    if op.startswith("sha256"):
        assert (out[:n, 8:] == du.OUT_FILL).all(), f"{op}: a lane stored past its 8 words"
    assert (out[n:] == du.OUT_FILL).all(), f"{op}: a row past n = {n} changed"
    return out


# ---- SHA-512: every size x every shift ---------------------------------------

@pytest.mark.parametrize("filler", FILLERS)
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("op", list(du.SHA512_OPS))
def test_sha512_every_size_and_shift(diag, op, order, filler):
    buf, cases = cached(("sweep", op), lambda: du.sha512_sweep(op))
    check(diag, op, buf, cases if order == "sorted" else du.shuffled(cases), filler)


# ---- SHA-512: chosen wave compositions ---------------------------------------

@pytest.mark.parametrize("filler", FILLERS)
@pytest.mark.parametrize("op", ["sha512_ram", "sha512_ram_2w"])
def test_sha512_wave_compositions(diag, op, filler):
    buf, cases, names = cached(("waves", op), lambda: du.sha512_wave_compositions(op))
    per = du.hash_per_block(op)
    assert len(cases) == per * len(names)
    out = du.run_hash(diag, op, buf.bytes(filler), cases)
    bad = du.hash_mismatches(cases, out)
    assert not bad, f"filler {filler:#04x}: " + "\n".join(bad[:12])


@pytest.mark.parametrize("last", ["longest", "shortest"])
@pytest.mark.parametrize("n", [1, 31, 33, 65])
def test_sha512_two_wave_dead_lanes(diag, n, last):
    """dead lanes of the last block repeat case n - 1 and store nothing:
    the rows after n keep the caller's pattern, on the host and (the entry
    point's padding rows) on the device"""
    buf, cases = cached(("dead", n, last), lambda: du.sha512_dead_lane_cases(n, last))
    for filler in FILLERS:
        check(diag, "sha512_ram_2w", buf, cases, filler, extra_rows=64)


def test_sha512_one_wave_rows_past_n(diag):
    buf, cases = cached(("sweep", "sha512_ram"), lambda: du.sha512_sweep("sha512_ram"))
    for op, n in (("sha512_ram", 65), ("sha512_ram", 1)):
        check(diag, op, buf, cases[-n:], 0xff, extra_rows=64)


# ---- SHA-256: bytes and leaf ----------------------------------------------------

@pytest.mark.parametrize("filler", FILLERS)
def test_sha256_bytes_every_size_and_shift(diag, filler):
    buf, cases = cached("bytes", du.sha256_bytes_sweep)
    check(diag, "sha256_bytes", buf, cases, filler)


@pytest.mark.parametrize("filler", FILLERS)
def test_sha256_leaf_every_size_and_shift(diag, filler):
    """the filler also fills the 26 bytes in front of the leaf data, which
    sha256_leaf loads and replaces with the prefix"""
    buf, cases = cached("leaf", du.sha256_leaf_sweep)
    check(diag, "sha256_leaf", buf, cases, filler)


# ---- SHA-256: node and node pair --------------------------------------------------

def test_sha256_node_and_node_pair(diag):
    buf, nodes, pairs = cached("node", du.sha256_node_sweep)
    rng = random.Random(76)
    outs = []
    for filler in FILLERS:                      # the 4 bytes after the sibling too
        for garbage in (False, True):           # words 5..7 of the running node are no part of it
            run = [dict(c, opnd=c["opnd"] + ([rng.getrandbits(32) for _ in range(3)] if garbage else [0, 0, 0]))
                   for c in nodes]
            outs.append(check(diag, "sha256_node", buf, run, filler)[:len(nodes), :8])
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])
    pair_out = check(diag, "sha256_node_pair", buf, pairs, 0x00)[:len(pairs), :8]
    differ = np.nonzero((pair_out != outs[0]).any(axis=1))[0]
    assert len(differ) == 0, [du.hash_describe(nodes, int(i)) for i in differ[:8]]


# ---- the entry point's argument checks ----------------------------------------------

def test_hash_entry_point_rejects_bad_arguments(diag):
    buf = np.zeros(256, np.uint8)
    fill = 0x12345678

    def rc(op, off, sz, n=1, buf_sz=None):
        inp = np.zeros((4, du.HASH_IN), np.uint32)
        inp[:, 0], inp[:, 1] = off, sz
        inp[0, 0], inp[0, 1] = 0, 38           # case 0 is in bounds for every op: the check reads every case
        out = np.full((4, du.HASH_OUT), fill, np.uint32)
        got = diag.raw_hash(op, buf, inp, out, n, buf_sz)
        assert (out == fill).all() or got == 0
        return got

    ops = {name: i for i, name in enumerate(du.HASH_OPS)}
    for op in (-1, len(du.HASH_OPS), 99):
        assert rc(op, 0, 38) == HIP_ERROR_INVALID_VALUE
    for op in ops.values():
        assert rc(op, 0, 38, n=(1 << 20) + 1) == HIP_ERROR_INVALID_VALUE
    # one byte outside the buffer, for each op shape; the same case one byte further in is served
    for name in ("sha512_pre8", "sha512_ram", "sha512_ram_2w", "sha256_bytes"):
        assert rc(ops[name], 200, 57, n=2) == HIP_ERROR_INVALID_VALUE
        assert rc(ops[name], 257, 0, n=2) == HIP_ERROR_INVALID_VALUE
        assert rc(ops[name], 200, 56, n=2) == 0
    assert rc(ops["sha256_leaf"], 100, 93, n=2) == HIP_ERROR_INVALID_VALUE     # 100 + 64 + 93 = 257
    assert rc(ops["sha256_leaf"], 100, 92, n=2) == 0
    assert rc(ops["sha256_leaf"], 100, 37, n=2) == HIP_ERROR_INVALID_VALUE     # below the function's 38
    assert rc(ops["sha256_bytes"], 100, 0, n=2) == HIP_ERROR_INVALID_VALUE     # below the function's 1
    assert rc(ops["sha256_node"], 237, 0, n=2) == HIP_ERROR_INVALID_VALUE      # 237 + 20 = 257
    assert rc(ops["sha256_node"], 236, 0, n=2) == 0
    assert rc(ops["sha256_node_pair"], 1 << 30, 1 << 30, n=2) == 0              # no bytes: off and sz are not read
    assert rc(ops["sha512_ram"], 0, 38, buf_sz=(1 << 28) + 1) == HIP_ERROR_INVALID_VALUE
    assert rc(ops["sha512_ram"], 0, 38, n=0) == 0                               # nothing to do
