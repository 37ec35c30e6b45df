"""Makes tests/golden/poh.npz: what the reference's own proof-of-history
functions give for seeded signatures, states and microblocks, and for the
captured batch that tests/golden/shreds.npz's data shreds carry.

    python tests/golden/gen_poh.py <reference>/src

gen_poh_ref.c, this project's own harness, is compiled in a temporary
directory against the reference's sources the way gen_reedsol.py compiles its
harness (gen_packets.ref_defs), with the reference's SHA extensions path
where this CPU has them.  It calls fd_poh_append, fd_poh_mixin,
fd_wbmtree32_*, fd_bmtree_commit_* and fd_txn_parse_core.

  sigs[130][64], roots[130][32]
                   seeded signatures and fd_wbmtree32's root of the first S,
                   S = 1..130 (fd_bmtree_commit's root, 32-byte nodes and the
                   1-byte prefix, asserted equal)
  append_in[32], append_k[9], append_out[9][32]
                   fd_poh_append of a seeded state, k in 0, 1, 2, 3, 63, 64,
                   65, 1000, 4096
  mix_in[4][32], mix_root[4][32], mix_out[4][32]
                   fd_poh_mixin
  mb_in[n][32], mb_hash_cnt[n], mb_txn_cnt[n], mb_sig_at[n+1], mb_sigs[.][64],
  mb_hdr_hash[n][32], mb_state[n][32], mb_verdict[n], mb_kind[n]
                   synthetic microblocks: what the steps of
                   fd_runtime.c:2017-2062 compute from in, the counts and the
                   signatures mb_sigs[mb_sig_at[i]:mb_sig_at[i+1]], and 0 /
                   -25 for whether that is mb_hdr_hash; kind indexes KINDS
  cap_state[64][32], cap_verdict[64]
                   the captured batch, microblock 0 from a zero in state
  ref_hash_rate, ref_root20_rate, ref_cpu
                   fd_poh_append hashes/s and 20-leaf roots/s on one core of
                   the machine the generator ran on, and its CPU model
  cases            how many cases the generator asserted tests/poh_model.py on

Nothing here is run by a test."""
import os
import random
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

SEED = 257
SIZE_LIMIT = 1 << 20    # of a committed file
KS = (0, 1, 2, 3, 63, 64, 65, 1000, 4096)
KINDS = ("good", "hdr_hash_bit", "sig_bit", "wrong_in", "hash_cnt_0_txns", "hash_cnt_1_txns", "hash_cnt_0_tick")
REF_C = ["ballet/poh/fd_poh.c", "ballet/bmtree/fd_wbmtree.c", "ballet/bmtree/fd_bmtree.c", "ballet/sha256/fd_sha256.c",
         "ballet/sha256/fd_sha256_batch_avx.c", "ballet/txn/fd_txn_parse.c", "util/log/fd_log.c", "util/cstr/fd_cstr.c",
         "util/env/fd_env.c", "util/io/fd_io.c", "util/tile/fd_tile.c"]


def cpu():
    model, flags = "unknown", ""
    for line in open("/proc/cpuinfo"):
        if line.startswith("model name") and model == "unknown":
            model = line.split(":", 1)[1].strip()
        if line.startswith("flags") and not flags:
            flags = line
    return model, "sha_ni" in flags.split()


def run_reference(ref, blob):
    """the harness's output for the input blob"""
    from gen_packets import ref_defs
    root = os.path.dirname(os.path.abspath(ref))
    ref = os.path.abspath(ref)
    shani = cpu()[1]
    extra = ["-DFD_HAS_SHANI=1", "-msha"] if shani else []
    srcs = REF_C + (["ballet/sha256/fd_sha256_core_shaext.S"] if shani else [])
    with tempfile.TemporaryDirectory() as tmp:
        exe, objs, jobs = os.path.join(tmp, "gen_poh_ref"), [], []
        for src in srcs + [os.path.join(HERE, "gen_poh_ref.c")]:
            obj = os.path.join(tmp, os.path.basename(src).rsplit(".", 1)[0] + ".o")
            jobs.append(subprocess.Popen(["gcc"] + ref_defs(ref) + ["-march=haswell"] + extra +
                                         ["-c", os.path.join(ref, src), "-o", obj], cwd=root))
            objs.append(obj)
        assert not any(j.wait() for j in jobs)
        subprocess.run(["gcc", "-pthread", "-o", exe] + objs + ["-lm"], check=True)
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(blob)
        subprocess.run([exe, fin, fout], check=True, cwd=root)
        return open(fout, "rb").read()


def rand(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


def flip(rng, b):
    b = bytearray(b)
    b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
    return bytes(b)


def make_microblocks(rng, sigs):
    """[(kind, in, hash_cnt, txn_cnt, [sig], header hash)]: the header hash
    is what the model computes for the unbroken microblock"""
    import poh_model as model
    out = []

    def add(kind, hash_cnt, n_sig, txn_cnt=None):
        state = rand(rng, 32)
        mine = [sigs[rng.randrange(len(sigs))] for _ in range(n_sig)]
        txn_cnt = (max(1, n_sig - rng.randrange(0, 3)) if n_sig else 0) if txn_cnt is None else txn_cnt
        k, mix = model.steps(hash_cnt, txn_cnt)
        hdr = model.append(state, k)
        if mix:
            hdr = model.mixin(hdr, mine)
        if kind == "hdr_hash_bit":
            hdr = flip(rng, hdr)
        elif kind == "sig_bit":
            j = rng.randrange(n_sig)
            mine[j] = flip(rng, mine[j])
        elif kind == "wrong_in":
            state = flip(rng, state)
        out.append((kind, state, hash_cnt, txn_cnt, mine, hdr))

    for n_sig in (1, 2, 3, 4, 5, 7, 8, 9, 20, 63, 64, 65, 127, 128, 129, 130, 300):
        add("good", rng.choice((1, 2, 3, 17)), n_sig)
    for k in KS:
        add("good", k, 0)
        add("good", k + 1, 3)
    for kind in ("hdr_hash_bit", "sig_bit", "wrong_in"):
        for hash_cnt, n_sig in ((1, 1), (5, 20), (64, 129)):
            add(kind, hash_cnt, n_sig)
    add("hdr_hash_bit", 9, 0)
    add("wrong_in", 9, 0)
    add("hash_cnt_0_txns", 0, 5)
    add("hash_cnt_1_txns", 1, 5)
    add("hash_cnt_0_tick", 0, 0)
    return out


def main(ref):
    import poh_model as model
    import poh_util as util
    rng = random.Random(SEED)
    sigs = [rand(rng, 64) for _ in range(130)]
    append_in = rand(rng, 32)
    mixes = [(rand(rng, 32), rand(rng, 32)) for _ in range(4)]
    mbs = make_microblocks(rng, sigs)
    cap = util.captured()
    cap_txns = []
    blk, at = util.captured_block(), 8
    for i in range(64):
        txn_cnt, = struct.unpack_from("<Q", blk, at + 0x28)
        at += 48
        for _ in range(txn_cnt):
            size = model.txn_size(blk[at:at + 1232])
            assert size
            cap_txns.append((at, size))
            at += size
    assert at == len(blk)

    ops = []
    for s in range(1, 131):
        ops.append(struct.pack("<BI", 1, s) + b"".join(sigs[:s]))
    for k in KS:
        ops.append(struct.pack("<B", 2) + append_in + struct.pack("<Q", k))
    for st, rt in mixes:
        ops.append(struct.pack("<B", 3) + st + rt)
    for _, state, hash_cnt, txn_cnt, mine, _ in mbs:
        ops.append(struct.pack("<B", 4) + state + struct.pack("<QQI", hash_cnt, txn_cnt, len(mine)) + b"".join(mine))
    for i in range(cap.n):
        hash_cnt, = struct.unpack_from("<Q", cap.buf, int(cap.hdr_off[i]))
        txn_cnt, = struct.unpack_from("<Q", cap.buf, int(cap.hdr_off[i]) + 0x28)
        mine = [cap.buf[int(o):int(o) + 64] for o in cap.sig_off[cap.sig_first[i]:cap.sig_first[i + 1]]]
        state = cap.buf[int(cap.in_off[i]):int(cap.in_off[i]) + 32]
        ops.append(struct.pack("<B", 4) + state + struct.pack("<QQI", hash_cnt, txn_cnt, len(mine)) + b"".join(mine))
    for at, size in cap_txns:
        # offered what remains of the block, as the walk offers it
        rest = blk[at:at + 1232]
        ops.append(struct.pack("<BI", 5, len(rest)) + rest)
    ops.append(struct.pack("<BQQ", 6, 20_000_000, 200_000))
    raw = run_reference(ref, struct.pack("<I", len(ops)) + b"".join(ops))

    pos, cases = 0, 0

    def take(n):
        nonlocal pos
        pos += n
        return raw[pos - n:pos]

    roots = []
    for s in range(1, 131):
        wb, bm = take(32), take(32)
        assert wb == bm == model.root(sigs[:s]), s
        roots.append(wb)
        cases += 1
    append_out = []
    for k in KS:
        append_out.append(take(32))
        assert append_out[-1] == model.append(append_in, k), k
        cases += 1
    mix_out = []
    for st, rt in mixes:
        mix_out.append(take(32))
        assert mix_out[-1] == model.sha(st + rt)
        cases += 1
    mb_state, mb_verdict, seen = [], [], {}
    for kind, state, hash_cnt, txn_cnt, mine, hdr in mbs:
        got = take(32)
        # the model on the same microblock laid out in a buffer
        buf = state + struct.pack("<Q", hash_cnt) + hdr + struct.pack("<Q", txn_cnt) + b"".join(mine)
        code, want = model.verify(buf, 32, 0, 0, len(mine), len(mine), [80 + 64 * j for j in range(len(mine))])
        assert want == got, kind
        verdict = 0 if got == hdr else model.ERR_HASH
        assert verdict == code, kind
        mb_state.append(got); mb_verdict.append(verdict)
        seen.setdefault(kind, set()).add(verdict)
        cases += 1
    assert seen == {"good": {0}, "hdr_hash_bit": {-25}, "sig_bit": {-25}, "wrong_in": {-25}, "hash_cnt_0_txns": {0},
                    "hash_cnt_1_txns": {0}, "hash_cnt_0_tick": {0}}, seen
    cap_codes, cap_states = cap.want()
    cap_state, cap_verdict = [], []
    for i in range(cap.n):
        got = take(32)
        hdr = cap.buf[int(cap.hdr_off[i]) + 8:int(cap.hdr_off[i]) + 40]
        verdict = 0 if got == hdr else model.ERR_HASH
        assert got == cap_states[i].tobytes() and verdict == cap_codes[i], i
        cap_state.append(got); cap_verdict.append(verdict)
        cases += 1
    assert cap_verdict[1:] == [0] * 63, cap_verdict
    for at, size in cap_txns:
        pay, = struct.unpack("<Q", take(8))
        assert pay == size, (at, pay, size)
        cases += 1
    r_hash, r_root = struct.unpack("<dd", take(16))
    assert pos == len(raw)

    sig_at = [0]
    for m in mbs:
        sig_at.append(sig_at[-1] + len(m[4]))
    arr = lambda rows, w: np.frombuffer(b"".join(rows), np.uint8).reshape(-1, w)   # noqa: E731
    out = os.path.join(HERE, "poh.npz")
    np.savez_compressed(
        out, sigs=arr(sigs, 64), roots=arr(roots, 32), append_in=np.frombuffer(append_in, np.uint8),
        append_k=np.array(KS, np.uint64), append_out=arr(append_out, 32), mix_in=arr([m[0] for m in mixes], 32),
        mix_root=arr([m[1] for m in mixes], 32), mix_out=arr(mix_out, 32), mb_in=arr([m[1] for m in mbs], 32),
        mb_hash_cnt=np.array([m[2] for m in mbs], np.uint64), mb_txn_cnt=np.array([m[3] for m in mbs], np.uint64),
        mb_sig_at=np.array(sig_at, np.uint32), mb_sigs=arr([s for m in mbs for s in m[4]], 64),
        mb_hdr_hash=arr([m[5] for m in mbs], 32), mb_state=arr(mb_state, 32), mb_verdict=np.array(mb_verdict, np.int8),
        mb_kind=np.array([KINDS.index(m[0]) for m in mbs], np.uint8), cap_state=arr(cap_state, 32),
        cap_verdict=np.array(cap_verdict, np.int8), ref_hash_rate=np.array(r_hash), ref_root20_rate=np.array(r_root),
        ref_cpu=np.array(cpu()[0] + (" (SHA extensions)" if cpu()[1] else "")), cases=np.array(cases, np.uint32))
    size = os.path.getsize(out)
    print(out, size, "bytes,", cases, "cases asserted, none failed; captured verdicts", cap_verdict[:2], "...;",
          "%.3g hashes/s, %.3g 20-leaf roots/s" % (r_hash, r_root), "on", cpu())
    assert size <= SIZE_LIMIT, size


if __name__ == "__main__":
    main(sys.argv[1])
