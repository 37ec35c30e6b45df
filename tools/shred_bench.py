#!/usr/bin/env python3
"""Times the shred path (fd_ed25519_hip_shreds_dev) against plain
verification of the same signatures (fd_ed25519_hip_verify_dev),
device-resident inputs, HIP events on one engine in one process:

  --shreds shreds (default 262,144): the reference's 480 captured shreds
  (tests/golden/shreds.npz: 1203-byte data and 1228-byte code shreds of
  tree depth 6 and 7) repeated back to back, each under a leader key of its
  own, its signature made by the device signer over the root the host
  derives (fd_ed25519_hip_shred_root);

  shreds_dev  parse + leaf hash + proof walk + gather, the verify phases,
              finish
  verify_dev  the verify phases alone over the signatures, keys and 32-byte
              roots one shreds_dev call laid out in its workspace

Both are warmed up, then timed alternately --reps times; the medians and
their ratio (verify / shreds: 1 would mean staging and finish are free) go
to --out (profiles/shred_bench.json), with the difference of the two
medians as the stage and finish kernels' time and the shred bytes the
stage reads over it.

  python tools/shred_bench.py [--shreds N] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from precompile_bench import Events  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shreds", type=int, default=1 << 18)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max-chunk", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "shred_bench.json"))
    a = ap.parse_args()
    from firedancer_amd import ed25519 as ed

    if ed.device_count() < 1:
        sys.exit("shred_bench: no GPU (this tool measures; it has no CPU mode)")
    n = a.shreds
    fx = np.load(os.path.join(REPO, "tests", "golden", "shreds.npz"))
    fsz = fx["sz"].astype(np.int64)
    fat = np.concatenate([[0], np.cumsum(fsz)])
    fshred = [fx["shreds"][fat[i]:fat[i + 1]] for i in range(len(fsz))]
    froot = np.zeros((len(fsz), 32), np.uint8)
    for i, s in enumerate(fshred):
        code, root = ed.shred_root(s.tobytes())
        assert code == 0
        froot[i] = np.frombuffer(root, np.uint8)
    which = np.arange(n) % len(fsz)
    sz = fsz[which]
    off = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.uint64)
    total = int(sz.sum())
    reps = -(-n // len(fsz))
    buf = np.tile(fx["shreds"], reps)[:total].copy()

    eng = ed.Engine(0, max_chunk=a.max_chunk)
    # a key of its own per shred, its signature over the shred's root by the device signer
    privs = np.random.default_rng(20252).integers(0, 256, 32 * n, dtype=np.uint8)
    d_msg = eng.alloc(32 * n + 16).upload(froot[which].reshape(-1))
    d_moff = eng.alloc(8 * n).upload(np.arange(n, dtype=np.uint64) * 32)
    d_msz = eng.alloc(4 * n).upload(np.full(n, 32, np.uint32))
    d_priv = eng.alloc(32 * n).upload(privs)
    d_sig, d_keys = eng.alloc(64 * n), eng.alloc(32 * n)
    eng.sign_dev(n, d_msg.ptr, d_moff.ptr, d_msz.ptr, d_priv.ptr, d_sig.ptr, d_keys.ptr)
    eng.sync()
    sigs = d_sig.download(np.uint8, 64 * n).reshape(n, 64)
    for b in (d_msg, d_moff, d_msz, d_priv, d_sig):
        b.free()
    at = off.astype(np.int64)[:, None] + np.arange(64)[None, :]
    buf[at.reshape(-1)] = sigs.reshape(-1)
    assert len({bytes(s) for s in sigs[:4096]}) == 4096, "signatures must be distinct"

    d_buf = eng.alloc(total + 16).upload(buf)
    d_off = eng.alloc(8 * n).upload(off)
    d_sz = eng.alloc(4 * n).upload(sz.astype(np.uint32))
    d_work = eng.alloc(ed.shred_work_bytes(n))
    d_out, d_codes = eng.alloc(n), eng.alloc(n)

    def shreds():
        eng.shreds_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, d_keys.ptr, d_work.ptr, d_out.ptr)

    def verify():   # the arrays the stage kernel laid out (FD_ED25519_HIP_SHRED_WORK_BYTES's layout)
        w = d_work.ptr
        eng.verify_dev(n, w + 64 * n, w + 96 * n, w + 104 * n, w, d_keys.ptr, d_codes.ptr)

    ev, stream = Events(), eng.stream
    for _ in range(a.warmup):
        shreds()
        verify()
    eng.sync()
    assert not d_out.download(np.int8, n).any() and not d_codes.download(np.int8, n).any(), "workload must verify"
    t_shr, t_ver = [], []
    for _ in range(a.reps):
        t_shr.append(ev.time_ms(stream, shreds))
        t_ver.append(ev.time_ms(stream, verify))
    shr, ver = statistics.median(t_shr), statistics.median(t_ver)
    # the stage reads every byte of a shred: the signature, the leaf data behind it, the proof
    depth = np.array([int(s[0x40]) & 0xF for s in fshred])[which]
    leaf = 26 + 1115 - 20 * depth + 0x18 + np.where(sz == 1228, 0x19, 0)
    res = {"shreds": n, "shred_bytes": total, "tree_depths": sorted(set(depth.tolist())),
           "sha256_blocks_per_shred": round(float(((leaf + 9 + 63) // 64 + 2 * depth).mean()), 2),
           "max_chunk": eng.info()["max_chunk"], "arch": eng.info()["arch"], "warmup": a.warmup, "reps": a.reps,
           "shreds_dev_ms": round(shr, 4), "verify_dev_ms": round(ver, 4),
           "shreds_dev_ms_all": [round(x, 4) for x in t_shr], "verify_dev_ms_all": [round(x, 4) for x in t_ver],
           "ratio_verify_over_shreds": round(ver / shr, 4), "stage_plus_finish_ms": round(shr - ver, 4),
           "stage_read_GB_per_s": round(total / (shr - ver) / 1e6, 1) if shr > ver else None,
           "shreds_per_s": round(n / shr * 1e3), "verify_sigs_per_s": round(n / ver * 1e3)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
