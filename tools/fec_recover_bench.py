#!/usr/bin/env python3
"""Times the recovery of received FEC sets (fd_ed25519_hip_fec_recover_dev)
beside the parity launch on the same sets in the same run; device-resident
inputs, HIP events on one engine in one process:

  --sets sets (default 4,096) of 32 + 32 shreds: the six 64-shred sets of the
  reference's capture (tests/golden/shreds.npz) as the leader sent them,
  repeated back to back, each with a seeded 32 of its 64 slots erased (their
  bytes zeroed; at least one code shred stays);

  recover              fec_recover_dev (one launch)
  parity               fec_parity_dev (one launch) over the same sets whole
  recover_seal_verify  fec_recover_dev, fec_seal_dev without keys and
                       shreds_dev under the capture's leader, on one stream

and, wall clock around the synchronous host call on the same sets,

  recover_host         fec_recover_host

All are warmed up, then timed in turn --reps times; medians and the spread
(min, max) go to --out (profiles/fec_recover_bench.json).  Beside the times:
the ratio recover / parity and an estimate of what the recovery does more
than the parity, in lane-operations a set against the parity's
7 x 32 x 32 x 256 (3 v_perm_b32, 3 v_xor_b32 and the table's address per
coefficient and dword):

  matrix   log D_r and log N_e, 32 additions (a table read and an add) for
           each of 64 lanes, and 1,024 coefficients of about 12 operations
           each (two divisions by a constant, four table reads, the address)
  headers  the first 7 columns of the erased data shreds, 7 x 32 products of
           about 12 operations for each of 8 x (erased data shreds) lanes
  stores   24 lanes an erased slot, about 40 operations each
  judge    the basis pick, rule 11 and the second judge pass, about 300
           operations for each of 64 lanes

  python tools/fec_recover_bench.py [--sets N] [--out PATH] [--label TEXT]
"""
import argparse
import json
import os
import random
import statistics
import struct
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from precompile_bench import Events  # noqa: E402

REGION, DATA_AT, CODE_AT = 1019, 0x40, 0x59   # depth 6
PARITY_LANE_OPS = 7 * 32 * 32 * 256
SEED = 277


def captured_sets(fx):
    """the capture's 64-shred sets as the leader sent them, shreds in tree order"""
    fat = np.concatenate([[0], np.cumsum(fx["sz"].astype(np.int64))])
    sets = {}
    for i in range(len(fx["sz"])):
        s = fx["shreds"][fat[i]:fat[i + 1]].tobytes()
        fec, = struct.unpack_from("<I", s, 0x4F)
        is_code = s[0x40] & 0xF0 == 0x40
        pos = struct.unpack_from("<H", s, 0x57)[0] if is_code else struct.unpack_from("<I", s, 0x49)[0] - fec
        sets.setdefault(fec, []).append((is_code, pos, s))
    return [[s for _, _, s in sorted(v)] for _, v in sorted(sets.items()) if len(v) == 64]


def extra_lane_ops(erased_data):
    """the estimate of the docstring, for a set of 32 + 32 with 32 erased slots of which erased_data are data shreds"""
    matrix = 64 * 32 * 2 + 1024 * 12
    headers = 8 * erased_data * 32 * 12
    stores = 32 * 24 * 40
    judge = 64 * 300
    return {"matrix": matrix, "headers": headers, "stores": stores, "judge": judge, "sum": matrix + headers + stores + judge}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max-chunk", type=int, default=0)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fec_recover_bench.json"))
    a = ap.parse_args()
    from firedancer_amd import ed25519 as ed
    from firedancer_amd.ed25519 import _ptr

    if ed.device_count() < 1:
        sys.exit("fec_recover_bench: no GPU (this tool measures; it has no CPU mode)")
    fx = np.load(os.path.join(REPO, "tests", "golden", "shreds.npz"))
    base = captured_sets(fx)
    assert len(base) == 6 and all(s[0x40] & 0xF0 == (0x80 if j < 32 else 0x40) for st in base for j, s in enumerate(st))
    n_set, per = a.sets, 64
    n = n_set * per
    rng = random.Random(SEED)
    erased = np.zeros((n_set, per), np.uint8)
    for k in range(n_set):
        while True:
            pick = rng.sample(range(per), 32)
            if len([j for j in pick if j >= 32]) < 32:      # a code shred stays
                break
        erased[k, pick] = 1
    erased_data = float(erased[:, :32].sum()) / n_set

    whole = np.concatenate([np.frombuffer(b"".join(base[k % 6]), np.uint8) for k in range(n_set)] + [np.zeros(16, np.uint8)])
    sz = np.concatenate([np.array([len(x) for x in base[k % 6]], np.uint32) for k in range(n_set)])
    off = np.concatenate([[0], np.cumsum(sz.astype(np.uint64))[:-1]]).astype(np.uint64)
    total = int(sz.sum())
    first = (np.arange(n_set + 1) * per).astype(np.uint32)
    flat_erased = erased.reshape(-1)
    received = whole.copy()
    for i in np.nonzero(flat_erased)[0]:
        received[int(off[i]):int(off[i]) + int(sz[i])] = 0
    keys = np.tile(fx["pubkey"].astype(np.uint8), n)

    eng = ed.Engine(0, max_chunk=a.max_chunk)
    d_buf = eng.alloc(total + 16).upload(received)
    d_full = eng.alloc(total + 16).upload(whole)
    d_off = eng.alloc(8 * n).upload(off)
    d_sz = eng.alloc(4 * n).upload(sz)
    d_er = eng.alloc(n).upload(flat_erased)
    d_first = eng.alloc(4 * (n_set + 1)).upload(first)
    d_keys = eng.alloc(32 * n).upload(keys)
    d_work, d_swork = eng.alloc(ed.fec_work_bytes(n, n_set)), eng.alloc(ed.shred_work_bytes(n))
    d_rset, d_pset, d_sset, d_vout = eng.alloc(n_set), eng.alloc(n_set), eng.alloc(n_set), eng.alloc(n)

    def recover():
        eng.fec_recover_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, d_er.ptr, n_set, d_first.ptr, d_rset.ptr)

    def parity():
        eng.fec_parity_dev(n, d_full.ptr, d_off.ptr, d_sz.ptr, n_set, d_first.ptr, d_pset.ptr)

    def recover_seal_verify():
        recover()
        eng.fec_seal_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, n_set, d_first.ptr, None, d_work.ptr, d_sset.ptr)
        eng.shreds_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, d_keys.ptr, d_swork.ptr, d_vout.ptr)

    # the three steps give back the capture's shreds, and every one of them verifies
    recover_seal_verify()
    parity()
    eng.sync()
    assert not d_rset.download(np.int8, n_set).any(), "every set must be recovered"
    assert not d_sset.download(np.int8, n_set).any() and not d_pset.download(np.int8, n_set).any()
    assert (d_buf.download(np.uint8, total) == whole[:total]).all(), "the recovered sets must be the capture's"
    assert (d_full.download(np.uint8, total) == whole[:total]).all(), "the parity must be the capture's"
    assert not d_vout.download(np.int8, n).any(), "every shred must verify under the capture's leader"

    codes = np.zeros(n_set, np.int8)
    h_buf = np.empty_like(received)

    def recover_host():
        np.copyto(h_buf, received)
        t0 = time.perf_counter()
        assert ed._lib.fd_ed25519_hip_fec_recover_host(eng._h, n, _ptr(h_buf), _ptr(off), _ptr(sz), _ptr(flat_erased), n_set,
                                                       _ptr(first), _ptr(codes)) == 0
        return (time.perf_counter() - t0) * 1e3

    dev = {"recover": recover, "parity": parity, "recover_seal_verify": recover_seal_verify}
    host = {"recover_host": recover_host}
    ev, stream = Events(), eng.stream
    for _ in range(a.warmup):
        for f in dev.values():
            f()
        eng.sync()
        for f in host.values():
            f()
    # the host call leaves the capture's shreds but for the proofs of the recovered slots, which are the seal's
    assert not codes.any()
    for i in np.nonzero(flat_erased)[0][:512]:
        o, depth = int(off[i]), 6
        assert (h_buf[o:o + int(sz[i]) - 20 * depth] == whole[o:o + int(sz[i]) - 20 * depth]).all()
    t = {k: [] for k in list(dev) + list(host)}
    for _ in range(a.reps):
        for k, f in dev.items():
            t[k].append(ev.time_ms(stream, f))
        for k, f in host.items():
            t[k].append(f())
    med = {k: statistics.median(v) for k, v in t.items()}
    extra = extra_lane_ops(erased_data)
    once = n_set * 64 * REGION                       # 32 regions read, 32 written
    res = {"label": a.label, "sets": n_set, "shreds_per_set": per, "data_per_set": 32, "parity_per_set": 32,
           "erased_per_set": 32, "erased_data_per_set_mean": round(erased_data, 2), "shreds": n, "shred_bytes": total,
           "region_bytes_read_and_written_once": once, "arch": eng.info()["arch"], "max_chunk": eng.info()["max_chunk"],
           "warmup": a.warmup, "reps": a.reps,
           "recover_ms": round(med["recover"], 4), "parity_ms": round(med["parity"], 4),
           "recover_over_parity": round(med["recover"] / med["parity"], 4),
           "recover_seal_verify_ms": round(med["recover_seal_verify"], 4),
           "recover_host_ms": round(med["recover_host"], 2),
           "recover_region_GB_per_s": round(once / med["recover"] / 1e6, 1),
           "shreds_per_s_recover_seal_verify": round(n / med["recover_seal_verify"] * 1e3),
           "parity_lane_ops_per_set": PARITY_LANE_OPS, "extra_lane_ops_per_set": extra,
           "estimated_recover_over_parity": round(1.0 + extra["sum"] / PARITY_LANE_OPS, 4),
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
