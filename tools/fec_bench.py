#!/usr/bin/env python3
"""Times the sealing of a leader's FEC sets (fd_ed25519_hip_fec_seal_dev) and,
in the same run, the shred front (fd_ed25519_hip_shreds_dev) on the sealed
result; device-resident inputs, HIP events on one engine in one process:

  --sets sets (default 4,096) of 32 + 32 shreds, 262,144 shreds, the count the
  shred front was measured on: the six 64-shred sets of the reference's
  capture (tests/golden/shreds.npz) with signatures and proofs blanked,
  repeated back to back, each set under a private key of its own;

  tree      fec_seal_dev without keys: the rules, the leaf hashes, the layers
            and the proofs (one launch)
  sign      the device signer over the roots the tree left in the workspace
            (fd_ed25519_hip_sign_dev, the launch fec_seal_dev makes)
  seal      fec_seal_dev with keys: tree, sign and scatter; the scatter's time
            is what the three launches take beyond the two above
  shreds    shreds_dev on the sealed shreds under the sets' public keys, and
            verify_dev over the slots it laid out: their difference is the
            shred front's stage and finish kernels, which hash the same leaf
            and `depth` nodes a shred where the tree hashes about one

All are warmed up, then timed in turn --reps times; the medians go to --out
(profiles/fec_bench.json).  The library (and with it the tree kernel's
workgroup size, FD_FEC_TREE_BLOCK at build time) is the one
$FD_ED25519_HIP_LIB names; --label names it in the result.

  python tools/fec_bench.py [--sets N] [--out PATH] [--label TEXT]
"""
import argparse
import ctypes
import json
import os
import statistics
import struct
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from precompile_bench import Events  # noqa: E402


def captured_sets(fx):
    """the capture's 64-shred sets, shreds in tree order, signature and proof zeroed"""
    fat = np.concatenate([[0], np.cumsum(fx["sz"].astype(np.int64))])
    sets = {}
    for i in range(len(fx["sz"])):
        s = bytearray(fx["shreds"][fat[i]:fat[i + 1]].tobytes())
        fec, = struct.unpack_from("<I", s, 0x4F)
        is_code = s[0x40] & 0xF0 == 0x40
        pos = struct.unpack_from("<H", s, 0x57)[0] if is_code else struct.unpack_from("<I", s, 0x49)[0] - fec
        depth = s[0x40] & 0xF
        s[:64] = bytes(64)
        s[len(s) - 20 * depth:] = bytes(20 * depth)
        sets.setdefault(fec, []).append((is_code, pos, bytes(s)))
    return [[s for _, _, s in sorted(v)] for _, v in sorted(sets.items()) if len(v) == 64]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max-chunk", type=int, default=0)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fec_bench.json"))
    a = ap.parse_args()
    from firedancer_amd import ed25519 as ed

    if ed.device_count() < 1:
        sys.exit("fec_bench: no GPU (this tool measures; it has no CPU mode)")
    ed._lib.fd_ed25519_hip_private_fec_tree_block.restype = ctypes.c_uint
    block = ed._lib.fd_ed25519_hip_private_fec_tree_block()
    base = captured_sets(np.load(os.path.join(REPO, "tests", "golden", "shreds.npz")))
    assert len(base) == 6
    n_set, per = a.sets, 64
    n = n_set * per
    blobs = [np.frombuffer(b"".join(s), np.uint8) for s in base]
    buf = np.concatenate([blobs[k % 6] for k in range(n_set)])
    sz = np.concatenate([np.array([len(x) for x in base[k % 6]], np.uint32) for k in range(n_set)])
    off = np.concatenate([[0], np.cumsum(sz.astype(np.uint64))[:-1]]).astype(np.uint64)
    total = int(sz.sum())
    first = (np.arange(n_set + 1) * per).astype(np.uint32)
    privs = np.random.default_rng(20253).integers(0, 256, 32 * n_set, dtype=np.uint8)

    eng = ed.Engine(0, max_chunk=a.max_chunk)
    d_buf = eng.alloc(total + 16).upload(np.concatenate([buf, np.zeros(16, np.uint8)]))
    d_off = eng.alloc(8 * n).upload(off)
    d_sz = eng.alloc(4 * n).upload(sz)
    d_first = eng.alloc(4 * (n_set + 1)).upload(first)
    d_priv = eng.alloc(32 * n_set).upload(privs)
    d_work = eng.alloc(ed.fec_work_bytes(n, n_set))
    d_set, d_sig2, d_pub2 = eng.alloc(n_set), eng.alloc(64 * n_set), eng.alloc(32 * n_set)
    w = d_work.ptr   # FD_ED25519_HIP_FEC_WORK_BYTES's layout: sigs, pubs, roots, msg_off, msg_sz, set_of

    def tree():
        eng.fec_seal_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, n_set, d_first.ptr, None, d_work.ptr, d_set.ptr)

    def sign():
        eng.sign_dev(n_set, w + 96 * n_set, w + 128 * n_set, w + 136 * n_set, d_priv.ptr, d_sig2.ptr, d_pub2.ptr)

    def seal():
        eng.fec_seal_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, n_set, d_first.ptr, d_priv.ptr, d_work.ptr, d_set.ptr)

    seal()
    eng.sync()
    assert not d_set.download(np.int8, n_set).any(), "every set must seal"
    pubs = d_work.download(np.uint8, 32 * n_set, offset_bytes=64 * n_set).reshape(n_set, 32)
    d_keys = eng.alloc(32 * n).upload(np.repeat(pubs, per, axis=0).reshape(-1))
    d_swork = eng.alloc(ed.shred_work_bytes(n))
    d_out, d_codes = eng.alloc(n), eng.alloc(n)

    def shreds():
        eng.shreds_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, d_keys.ptr, d_swork.ptr, d_out.ptr)

    def verify():   # the arrays the shred stage laid out (FD_ED25519_HIP_SHRED_WORK_BYTES's layout)
        v = d_swork.ptr
        eng.verify_dev(n, v + 64 * n, v + 96 * n, v + 104 * n, v, d_keys.ptr, d_codes.ptr)

    fns = {"tree": tree, "sign": sign, "seal": seal, "shreds": shreds, "verify": verify}
    ev, stream = Events(), eng.stream
    for _ in range(a.warmup):
        for f in fns.values():
            f()
    eng.sync()
    assert not d_out.download(np.int8, n).any() and not d_codes.download(np.int8, n).any(), "the sealed shreds must verify"
    t = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, f in fns.items():
            t[k].append(ev.time_ms(stream, f))
    med = {k: statistics.median(v) for k, v in t.items()}
    stage = med["shreds"] - med["verify"]
    res = {"label": a.label, "tree_block": block, "sets": n_set, "shreds_per_set": per, "shreds": n, "shred_bytes": total,
           "tree_depth": 6, "arch": eng.info()["arch"], "max_chunk": eng.info()["max_chunk"], "warmup": a.warmup,
           "reps": a.reps,
           "tree_ms": round(med["tree"], 4), "sign_ms": round(med["sign"], 4), "seal_ms": round(med["seal"], 4),
           "scatter_ms_by_difference": round(med["seal"] - med["tree"] - med["sign"], 4),
           "shreds_dev_ms": round(med["shreds"], 4), "verify_dev_ms": round(med["verify"], 4),
           "shred_stage_plus_finish_ms": round(stage, 4),
           "tree_over_shred_stage": round(med["tree"] / stage, 4) if stage > 0 else None,
           "sealed_shreds_per_s": round(n / med["seal"] * 1e3), "tree_read_GB_per_s": round(total / med["tree"] / 1e6, 1),
           "all_ms": {k: [round(x, 4) for x in v] for k, v in t.items()}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "all_ms"}))
    eng.close()


if __name__ == "__main__":
    main()
