#!/usr/bin/env python3
"""Times the shredder front (fd_ed25519_hip_shredder_front_dev) beside the
parity launch and the seal's tree launch on the same sets in the same run;
device-resident inputs, HIP events on one engine in one process:

  --sets batches (default 4,096) of 31,840 bytes, one set of 32 + 32 shreds
  each -- the seal bench's workload: the six 31,840-byte slices of the
  reference's captured entry batch (rebuilt from tests/golden/shreds.npz) that
  its six 64-shred sets carry, repeated, each batch under a private key of its
  own (a batch of its own is its own last set, so its last data shred carries
  the last-in-batch flag the capture's first six sets do not);

  front          shredder_front_dev (a memset and one launch)
  parity         fec_parity_dev on the front's sets (one launch)
  tree           fec_seal_dev without keys (one launch)
  parity_seal    fec_parity_dev, then fec_seal_dev with keys, on one stream
  shredder       shredder_dev: front, parity and seal with keys on one stream

and, wall clock around the synchronous host calls,

  shredder_host       fd_ed25519_hip_shredder_host: batch bytes up, shreds down
  cpu_front           fd_ed25519_hip_shredder batch by batch (the CPU build of
                      the sets the next line starts from)
  parity_seal_host    fec_parity_host, then fec_seal_host, on CPU-built sets

All are warmed up, then timed in turn --reps times; medians and the spread
(min, max) go to --out (profiles/shredder_bench.json) with the ratios and the
bytes each path moves each way.  The run checks that the three paths give the
same finished shreds.

  python tools/shredder_bench.py [--sets N] [--out PATH] [--label TEXT]
"""
import argparse
import json
import os
import statistics
import struct
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from precompile_bench import Events  # noqa: E402

SET_BYTES, PER, STRIDE = 31840, 64, 1228


def captured_block(golden):
    """the capture's entry batch: its data shreds' payloads in index order"""
    d = np.load(os.path.join(golden, "shreds.npz"))
    buf, at, data = d["shreds"].tobytes(), 0, []
    for sz in d["sz"]:
        s = buf[at:at + int(sz)]
        at += int(sz)
        if s[0x40] & 0xF0 == 0x80:
            data.append((struct.unpack_from("<I", s, 0x49)[0], s[0x58:struct.unpack_from("<H", s, 0x56)[0]]))
    return b"".join(p for _, p in sorted(data))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max-chunk", type=int, default=0)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "shredder_bench.json"))
    a = ap.parse_args()
    from firedancer_amd import ed25519 as ed
    from firedancer_amd.ed25519 import _ptr

    if ed.device_count() < 1:
        sys.exit("shredder_bench: no GPU (this tool measures; it has no CPU mode)")
    golden = os.path.join(REPO, "tests", "golden")
    block = captured_block(golden)
    nb = n_set = a.sets
    n = n_set * PER
    assert ed.shredder_count(SET_BYTES) == (1, 32, 32)
    slices = [np.frombuffer(block[SET_BYTES * k:SET_BYTES * (k + 1)], np.uint8) for k in range(6)]
    buf = np.concatenate([slices[b % 6] for b in range(nb)] + [np.zeros(16, np.uint8)])
    buf_sz = SET_BYTES * nb
    boff = (np.arange(nb, dtype=np.uint64) * SET_BYTES)
    bsz = np.full(nb, SET_BYTES, np.uint32)
    desc = np.zeros(nb, ed.SHREDDER_DESC)
    desc["data_idx"] = desc["parity_idx"] = 32 * (np.arange(nb) % 6)     # the capture's own indices: slot 0, version 0
    sfb = np.arange(nb + 1, dtype=np.uint32)
    hfb = (np.arange(nb + 1) * PER).astype(np.uint32)
    privs = np.random.default_rng(20261).integers(0, 256, 32 * nb, dtype=np.uint8)

    eng = ed.Engine(0, max_chunk=a.max_chunk)
    d_buf = eng.alloc(buf.nbytes).upload(buf)
    d_boff, d_bsz, d_desc = eng.alloc(8 * nb).upload(boff), eng.alloc(4 * nb).upload(bsz), eng.alloc(24 * nb).upload(desc)
    d_sfb, d_hfb = eng.alloc(4 * (nb + 1)).upload(sfb), eng.alloc(4 * (nb + 1)).upload(hfb)
    d_shreds = eng.alloc(STRIDE * n + 64)
    d_off, d_sz, d_first = eng.alloc(8 * n), eng.alloc(4 * n), eng.alloc(4 * (n_set + 1))
    d_bout, d_set, d_pset = eng.alloc(nb), eng.alloc(n_set), eng.alloc(n_set)
    d_priv = eng.alloc(32 * nb).upload(privs)
    d_work = eng.alloc(ed.shredder_work_bytes(n, n_set))
    front_args = (nb, d_buf.ptr, buf_sz, d_boff.ptr, d_bsz.ptr, d_desc.ptr, d_sfb.ptr, d_hfb.ptr, n_set, n, d_shreds.ptr, 0, STRIDE,
                  d_off.ptr, d_sz.ptr, d_first.ptr, d_bout.ptr)

    def front():
        eng.shredder_front_dev(*front_args)

    def parity():
        eng.fec_parity_dev(n, d_shreds.ptr, d_off.ptr, d_sz.ptr, n_set, d_first.ptr, d_pset.ptr)

    def tree():
        eng.fec_seal_dev(n, d_shreds.ptr, d_off.ptr, d_sz.ptr, n_set, d_first.ptr, None, d_work.ptr, d_set.ptr)

    def parity_seal():
        parity()
        eng.fec_seal_dev(n, d_shreds.ptr, d_off.ptr, d_sz.ptr, n_set, d_first.ptr, d_priv.ptr, d_work.ptr, d_set.ptr)

    def shredder():
        eng.shredder_dev(*front_args, d_priv.ptr, d_work.ptr, d_set.ptr)

    shredder()
    eng.sync()
    assert not d_bout.download(np.int8, nb).any() and not d_set.download(np.int8, n_set).any(), "every batch must shred"
    dev_shreds = d_shreds.download(np.uint8, STRIDE * n).reshape(n, STRIDE)

    h_out = np.zeros(STRIDE * n, np.uint8)
    h_ssz, h_first, h_bout = np.zeros(n, np.uint32), np.zeros(n_set + 1, np.uint32), np.zeros(nb, np.int8)
    codes, pcodes = np.zeros(n_set, np.int8), np.zeros(n_set, np.int8)
    h_off = np.arange(n, dtype=np.uint64) * STRIDE
    # the CPU-built sets keep arrays of their own, so that neither path's output can stand in for the other's;
    # fec_parity_host and fec_seal_host fill the caller's shreds in place (include/fd_ed25519_hip.h Parts 2g, 2f)
    h_cpu, h_cpu_ssz = np.zeros(STRIDE * n, np.uint8), np.zeros(n, np.uint32)

    def shredder_host():
        t0 = time.perf_counter()
        assert ed._lib.fd_ed25519_hip_shredder_host(eng._h, nb, _ptr(buf), _ptr(boff), _ptr(bsz), _ptr(desc), _ptr(privs), _ptr(h_out),
                                                    STRIDE, _ptr(h_ssz), _ptr(h_first), _ptr(h_bout), None, None) == 0
        return (time.perf_counter() - t0) * 1e3

    def cpu_front():
        t0 = time.perf_counter()
        first = np.zeros(2, np.uint32)
        for b in range(nb):
            assert ed._lib.fd_ed25519_hip_shredder(buf.ctypes.data + SET_BYTES * b, SET_BYTES, desc.ctypes.data + 24 * b, _ptr(h_cpu),
                                                   h_off.ctypes.data + 8 * PER * b, h_cpu_ssz.ctypes.data + 4 * PER * b, _ptr(first)) == 0
        return (time.perf_counter() - t0) * 1e3

    def parity_seal_host():
        t0 = time.perf_counter()
        assert ed._lib.fd_ed25519_hip_fec_parity_host(eng._h, n, _ptr(h_cpu), _ptr(h_off), _ptr(h_cpu_ssz), n_set, _ptr(hfb), _ptr(pcodes)) == 0
        assert ed._lib.fd_ed25519_hip_fec_seal_host(eng._h, n, _ptr(h_cpu), _ptr(h_off), _ptr(h_cpu_ssz), n_set, _ptr(hfb), _ptr(privs),
                                                    _ptr(codes), None, None) == 0
        return (time.perf_counter() - t0) * 1e3

    dev = {"front": front, "parity": parity, "tree": tree, "parity_seal": parity_seal, "shredder": shredder}
    host = {"shredder_host": shredder_host, "cpu_front": cpu_front, "parity_seal_host": parity_seal_host}
    ev, stream = Events(), eng.stream
    for _ in range(a.warmup):
        for f in dev.values():
            f()
        eng.sync()
        for f in host.values():
            f()
    assert not codes.any() and not pcodes.any() and not h_bout.any()
    # the device-resident path, the host wrapper and the parent's path on CPU-built sets give the same finished shreds
    assert (h_ssz == h_cpu_ssz).all() and (h_first == hfb).all()
    code = h_ssz == 1228
    for other in (h_cpu.reshape(n, STRIDE), dev_shreds):
        assert (h_out.reshape(n, STRIDE)[:, :1203] == other[:, :1203]).all() and (h_out.reshape(n, STRIDE)[code] == other[code]).all()
    t = {k: [] for k in list(dev) + list(host)}
    for _ in range(a.reps):
        for k, f in dev.items():
            t[k].append(ev.time_ms(stream, f))
        for k, f in host.items():
            t[k].append(f())
    med = {k: statistics.median(v) for k, v in t.items()}
    shred_bytes = n_set * 32 * (1203 + 1228)
    front_read, front_written = buf_sz, n_set * 32 * (1203 + 0x59 + 120)
    res = {"label": a.label, "batches": nb, "sets": n_set, "shreds_per_set": PER, "shreds": n, "batch_bytes": buf_sz,
           "shred_bytes": shred_bytes, "arch": eng.info()["arch"], "max_chunk": eng.info()["max_chunk"], "warmup": a.warmup,
           "reps": a.reps,
           "front_ms": round(med["front"], 4), "parity_ms": round(med["parity"], 4), "tree_ms": round(med["tree"], 4),
           "parity_seal_ms": round(med["parity_seal"], 4), "shredder_ms": round(med["shredder"], 4),
           "front_over_parity": round(med["front"] / med["parity"], 4), "front_over_tree": round(med["front"] / med["tree"], 4),
           "shredder_over_parity_seal": round(med["shredder"] / med["parity_seal"], 4),
           "front_bytes_read": front_read, "front_bytes_written": front_written,
           "front_GB_per_s": round((front_read + front_written) / med["front"] / 1e6, 1),
           "shredder_host_ms": round(med["shredder_host"], 2), "cpu_front_ms": round(med["cpu_front"], 2),
           "parity_seal_host_ms": round(med["parity_seal_host"], 2),
           "shredder_host_over_parity_seal_host": round(med["shredder_host"] / med["parity_seal_host"], 4),
           "shredder_host_over_cpu_front_and_parity_seal_host":
               round(med["shredder_host"] / (med["cpu_front"] + med["parity_seal_host"]), 4),
           "shredder_host_bytes_up": buf_sz + 32 * nb + 24 * nb, "shredder_host_bytes_down": STRIDE * n + 98 * n_set,
           "parity_seal_host_bytes_up": n_set * 32 * (1203 + 0x59) + shred_bytes,
           "parity_seal_host_bytes_down": n_set * 32 * 1228 + shred_bytes,
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
