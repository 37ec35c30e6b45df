#!/usr/bin/env python3
"""Times the Reed-Solomon parity of a leader's FEC sets
(fd_ed25519_hip_fec_parity_dev) beside the seal's tree launch on the same sets
in the same run; device-resident inputs, HIP events on one engine in one
process:

  --sets sets (default 4,096) of 32 + 32 shreds, the seal bench's workload: the
  six 64-shred sets of the reference's capture (tests/golden/shreds.npz) with
  parity regions, signatures and proofs blanked, repeated back to back, each
  set under a private key of its own;

  parity        fec_parity_dev (one launch)
  tree          fec_seal_dev without keys (one launch: rules, leaves, layers,
                proofs)
  parity_seal   fec_parity_dev, then fec_seal_dev with keys, on one stream

and, wall clock around the synchronous host calls on the same sets,

  seal_host          fec_seal_host on filled sets
  parity_seal_host   fec_parity_host, then fec_seal_host, on sets with empty
                     parity

All are warmed up, then timed in turn --reps times; medians and the spread
(min, max) go to --out (profiles/fec_parity_bench.json).  Beside the times:
the ratio parity / tree, the bytes of the sets' shreds read and written once
over the parity's time, and the two bounds the kernel can sit near --

  memory  the sets' protected regions once (32 read, 32 written) at the rate
          the tree launch reached in this run over the same shreds
  valu    the lane-operations of the compiled loop, 7 per coefficient and
          dword (3 v_perm_b32, 3 v_xor_b32, the table's address) over 256
          lanes a set, at 256 CUs x 64 lanes x 2.4 GHz

  python tools/fec_parity_bench.py [--sets N] [--out PATH] [--label TEXT]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from fec_bench import captured_sets  # noqa: E402
from precompile_bench import Events  # noqa: E402

REGION, DATA_AT, CODE_AT = 1019, 0x40, 0x59   # depth 6
VALU_LANE_OPS_PER_S = 256 * 64 * 2.4e9
LANE_OPS_PER_COEF_DWORD = 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max-chunk", type=int, default=0)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fec_parity_bench.json"))
    a = ap.parse_args()
    from firedancer_amd import ed25519 as ed
    from firedancer_amd.ed25519 import _ptr

    if ed.device_count() < 1:
        sys.exit("fec_parity_bench: no GPU (this tool measures; it has no CPU mode)")
    base = captured_sets(np.load(os.path.join(REPO, "tests", "golden", "shreds.npz")))   # signatures and proofs blanked
    assert len(base) == 6 and all(s[0x40] & 0xF0 == (0x80 if j < 32 else 0x40) for st in base for j, s in enumerate(st))
    empty = [[s if j < 32 else s[:CODE_AT] + bytes(REGION) + s[CODE_AT + REGION:] for j, s in enumerate(st)] for st in base]
    n_set, per = a.sets, 64
    n = n_set * per

    def tile(sets):
        blobs = [np.frombuffer(b"".join(s), np.uint8) for s in sets]
        return np.concatenate([blobs[k % 6] for k in range(n_set)] + [np.zeros(16, np.uint8)])

    filled_buf, empty_buf = tile(base), tile(empty)
    sz = np.concatenate([np.array([len(x) for x in base[k % 6]], np.uint32) for k in range(n_set)])
    off = np.concatenate([[0], np.cumsum(sz.astype(np.uint64))[:-1]]).astype(np.uint64)
    total = int(sz.sum())
    first = (np.arange(n_set + 1) * per).astype(np.uint32)
    privs = np.random.default_rng(20253).integers(0, 256, 32 * n_set, dtype=np.uint8)

    eng = ed.Engine(0, max_chunk=a.max_chunk)
    d_buf = eng.alloc(total + 16).upload(empty_buf)
    d_off = eng.alloc(8 * n).upload(off)
    d_sz = eng.alloc(4 * n).upload(sz)
    d_first = eng.alloc(4 * (n_set + 1)).upload(first)
    d_priv = eng.alloc(32 * n_set).upload(privs)
    d_work = eng.alloc(ed.fec_work_bytes(n, n_set))
    d_set, d_pset = eng.alloc(n_set), eng.alloc(n_set)

    def parity():
        eng.fec_parity_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, n_set, d_first.ptr, d_pset.ptr)

    def tree():
        eng.fec_seal_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, n_set, d_first.ptr, None, d_work.ptr, d_set.ptr)

    def parity_seal():
        parity()
        eng.fec_seal_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, n_set, d_first.ptr, d_priv.ptr, d_work.ptr, d_set.ptr)

    # the parity alone gives back the capture's code shreds
    parity()
    eng.sync()
    assert not d_pset.download(np.int8, n_set).any(), "every set must encode"
    assert (d_buf.download(np.uint8, total) == filled_buf[:total]).all(), "the parity must be the capture's"

    codes, pcodes = np.zeros(n_set, np.int8), np.zeros(n_set, np.int8)
    h_buf = np.empty_like(filled_buf)

    def seal_host():
        np.copyto(h_buf, filled_buf)
        t0 = time.perf_counter()
        assert ed._lib.fd_ed25519_hip_fec_seal_host(eng._h, n, _ptr(h_buf), _ptr(off), _ptr(sz), n_set, _ptr(first), _ptr(privs),
                                                    _ptr(codes), None, None) == 0
        return (time.perf_counter() - t0) * 1e3

    def parity_seal_host():
        np.copyto(h_buf, empty_buf)
        t0 = time.perf_counter()
        assert ed._lib.fd_ed25519_hip_fec_parity_host(eng._h, n, _ptr(h_buf), _ptr(off), _ptr(sz), n_set, _ptr(first),
                                                      _ptr(pcodes)) == 0
        assert ed._lib.fd_ed25519_hip_fec_seal_host(eng._h, n, _ptr(h_buf), _ptr(off), _ptr(sz), n_set, _ptr(first), _ptr(privs),
                                                    _ptr(codes), None, None) == 0
        return (time.perf_counter() - t0) * 1e3

    dev = {"parity": parity, "tree": tree, "parity_seal": parity_seal}
    host = {"seal_host": seal_host, "parity_seal_host": parity_seal_host}
    ev, stream = Events(), eng.stream
    for _ in range(a.warmup):
        for f in dev.values():
            f()
        eng.sync()
        for f in host.values():
            f()
    sealed_from_filled = None
    seal_host()
    sealed_from_filled = h_buf.copy()
    parity_seal_host()
    assert not codes.any() and not pcodes.any() and (h_buf == sealed_from_filled).all(), "both host paths must give the same shreds"
    t = {k: [] for k in list(dev) + list(host)}
    for _ in range(a.reps):
        for k, f in dev.items():
            t[k].append(ev.time_ms(stream, f))
        for k, f in host.items():
            t[k].append(f())
    med = {k: statistics.median(v) for k, v in t.items()}
    once = n_set * 64 * REGION                       # 32 regions read, 32 written
    valu_ms = n_set * 32 * 32 * 256 * LANE_OPS_PER_COEF_DWORD / VALU_LANE_OPS_PER_S * 1e3
    tree_rate = total / med["tree"] / 1e6            # GB/s the tree launch reached over the same shreds
    mem_ms = once / tree_rate / 1e6                  # the parity touches the regions only
    res = {"label": a.label, "sets": n_set, "shreds_per_set": per, "data_per_set": 32, "parity_per_set": 32, "shreds": n,
           "shred_bytes": total, "region_bytes_read_and_written_once": once, "arch": eng.info()["arch"],
           "max_chunk": eng.info()["max_chunk"], "warmup": a.warmup, "reps": a.reps,
           "parity_ms": round(med["parity"], 4), "tree_ms": round(med["tree"], 4),
           "parity_seal_ms": round(med["parity_seal"], 4),
           "parity_over_tree": round(med["parity"] / med["tree"], 4),
           "parity_region_GB_per_s": round(once / med["parity"] / 1e6, 1),
           "parity_shred_GB_per_s": round(total / med["parity"] / 1e6, 1), "tree_shred_GB_per_s": round(tree_rate, 1),
           "memory_bound_ms": round(mem_ms, 4), "valu_bound_ms": round(valu_ms, 4),
           "parity_over_memory_bound": round(med["parity"] / mem_ms, 3), "parity_over_valu_bound": round(med["parity"] / valu_ms, 3),
           "seal_host_ms": round(med["seal_host"], 2), "parity_seal_host_ms": round(med["parity_seal_host"], 2),
           "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()},
           "all_ms": {k: [round(x, 4) for x in v] for k, v in t.items()}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "all_ms"}))
    eng.close()


if __name__ == "__main__":
    main()
