#!/usr/bin/env python3
"""Times the control-packet path (fd_ed25519_hip_packets_dev) against plain
verification of the same signatures (fd_ed25519_hip_verify_dev),
device-resident inputs, HIP events on one engine in one process, for two
mixes of --packets packets (default 262,144) back to back in one buffer:

  repair  window_index, highest_window_index (160 bytes) and orphan (152)
          requests in turn, all to the own identity
  gossip  ping, pong (132 bytes) and prune messages of 8 origins (436) in
          turn, the prunes to the own identity

each packet under a sender key of its own, its signature made by the device
signer over the bytes the handlers verify.

  packets_dev  rules + gather + message copy, the verify phases, finish
  verify_dev   the verify phases alone over the signatures, keys and
               messages one packets_dev call laid out in its workspace

Both are warmed up, then timed alternately --reps times; the medians and
their ratio (verify / packets: 1 would mean staging and finish are free) go
to --out (profiles/packet_bench.json), with the difference of the two
medians as the stage and finish kernels' time and the bytes the stage reads
and writes over it.

  python tools/packet_bench.py [--packets N] [--out PATH]
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

PRUNE_M = 8


def kinds_of(mix):
    """[(discriminant, packet bytes, [(first, last) runs of the signed message], key at, signature at, addressee at)]"""
    if mix == "repair":
        return [(8, 160, [(0, 4), (68, 160)], 68, 4, 100), (9, 160, [(0, 4), (68, 160)], 68, 4, 100),
                (10, 152, [(0, 4), (68, 152)], 68, 4, 100)]
    m = 32 * PRUNE_M
    return [(4, 132, [(36, 68)], 4, 68, None), (5, 132, [(36, 68)], 4, 68, None),
            (3, 180 + m, [(36, 76 + m), (140 + m, 180 + m)], 36, 76 + m, 140 + m)]


def signed_on_device(eng, msgs, msg_sz, privs):
    """(signatures [n, 64], keys [n, 32]) of padded messages [n, w] by the device signer"""
    n, w = msgs.shape
    d_msg = eng.alloc(n * w + 16).upload(msgs.reshape(-1))
    d_moff = eng.alloc(8 * n).upload(np.arange(n, dtype=np.uint64) * w)
    d_msz = eng.alloc(4 * n).upload(msg_sz.astype(np.uint32))
    d_priv = eng.alloc(32 * n).upload(privs)
    d_sig, d_keys = eng.alloc(64 * n), eng.alloc(32 * n)
    eng.sign_dev(n, d_msg.ptr, d_moff.ptr, d_msz.ptr, d_priv.ptr, d_sig.ptr, d_keys.ptr)
    eng.sync()
    sigs, keys = d_sig.download(np.uint8, 64 * n).reshape(n, 64), d_keys.download(np.uint8, 32 * n).reshape(n, 32)
    for b in (d_msg, d_moff, d_msz, d_priv, d_sig, d_keys):
        b.free()
    return sigs, keys


def build(eng, mix, n, self_key, rng):
    """(packet buffer, offsets, sizes, message bytes) of n signed packets"""
    kinds = kinds_of(mix)
    which = np.arange(n) % len(kinds)
    width = max(k[1] for k in kinds)
    privs = rng.integers(0, 256, 32 * n, dtype=np.uint8)
    _, keys = signed_on_device(eng, np.zeros((n, 16), np.uint8), np.zeros(n, np.uint32), privs)   # the keys of these seeds
    pk = rng.integers(0, 256, (n, width), dtype=np.uint8)
    sz = np.zeros(n, np.int64)
    for j, (disc, size, _, key_at, _, to_at) in enumerate(kinds):
        rows = which == j
        sz[rows] = size
        pk[rows, 0:4] = np.frombuffer(np.uint32(disc).tobytes(), np.uint8)
        pk[rows, key_at:key_at + 32] = keys[rows]
        if disc == 3:
            pk[rows, 68:76] = np.frombuffer(np.uint64(PRUNE_M).tobytes(), np.uint8)
        if to_at is not None:
            pk[rows, to_at:to_at + 32] = np.frombuffer(self_key, np.uint8)
    msgs, msg_sz = np.zeros((n, width), np.uint8), np.zeros(n, np.int64)
    for j, (_, _, runs, _, _, _) in enumerate(kinds):
        rows, at = which == j, 0
        for a, b in runs:
            msgs[rows, at:at + b - a] = pk[rows, a:b]
            at += b - a
        msg_sz[rows] = at
    sigs, keys2 = signed_on_device(eng, msgs, msg_sz, privs)
    assert (keys2 == keys).all() and len({bytes(s) for s in sigs[:4096]}) == 4096, "signatures must be distinct"
    for j, (_, _, _, _, sig_at, _) in enumerate(kinds):
        rows = which == j
        pk[rows, sig_at:sig_at + 64] = sigs[rows]
    off = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.uint64)
    buf = pk[np.arange(width)[None, :] < sz[:, None]]    # row by row, each cut to its size
    assert buf.size == int(sz.sum())
    return buf, off, sz, int(msg_sz.sum())


def measure(eng, ed, ev, mix, n, warmup, reps):
    proto = ed.PROTO_REPAIR_SERV if mix == "repair" else ed.PROTO_GOSSIP
    rng = np.random.default_rng(20253)
    self_key = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    buf, off, sz, msg_bytes = build(eng, mix, n, self_key, rng)
    total = buf.size
    d_buf = eng.alloc(total + 16).upload(buf)
    d_off = eng.alloc(8 * n).upload(off)
    d_sz = eng.alloc(4 * n).upload(sz.astype(np.uint32))
    d_work = eng.alloc(ed.packet_work_bytes(n, total))
    d_out, d_codes = eng.alloc(n), eng.alloc(n)
    mirror = (total + 31) & ~15

    def packets():
        eng.packets_dev(proto, n, d_buf.ptr, d_off.ptr, d_sz.ptr, total, self_key, d_work.ptr, d_out.ptr)

    def verify():   # the arrays the stage kernel laid out (FD_ED25519_HIP_PACKET_WORK_BYTES's layout)
        w = d_work.ptr
        eng.verify_dev(n, w + 96 * n, w + 96 * n + mirror, w + 104 * n + mirror, w, w + 64 * n, d_codes.ptr)

    stream = eng.stream
    for _ in range(warmup):
        packets()
        verify()
    eng.sync()
    assert not d_out.download(np.int8, n).any() and not d_codes.download(np.int8, n).any(), "workload must verify"
    t_pkt, t_ver = [], []
    for _ in range(reps):
        t_pkt.append(ev.time_ms(stream, packets))
        t_ver.append(ev.time_ms(stream, verify))
    pkt, ver = statistics.median(t_pkt), statistics.median(t_ver)
    for b in (d_buf, d_off, d_sz, d_work, d_out, d_codes):
        b.free()
    # the stage reads a packet's header fields, its key, signature and message and writes the latter three
    moved = 2 * (96 * n + msg_bytes)
    return {"packets": n, "packet_bytes": int(total), "message_bytes": msg_bytes,
            "kinds": [{"disc": k[0], "bytes": k[1]} for k in kinds_of(mix)],
            "packets_dev_ms": round(pkt, 4), "verify_dev_ms": round(ver, 4),
            "packets_dev_ms_all": [round(x, 4) for x in t_pkt], "verify_dev_ms_all": [round(x, 4) for x in t_ver],
            "ratio_verify_over_packets": round(ver / pkt, 4), "stage_plus_finish_ms": round(pkt - ver, 4),
            "stage_moved_GB_per_s": round(moved / (pkt - ver) / 1e6, 1) if pkt > ver else None,
            "packets_per_s": round(n / pkt * 1e3), "verify_sigs_per_s": round(n / ver * 1e3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 18)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max-chunk", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "packet_bench.json"))
    a = ap.parse_args()
    from firedancer_amd import ed25519 as ed

    if ed.device_count() < 1:
        sys.exit("packet_bench: no GPU (this tool measures; it has no CPU mode)")
    eng = ed.Engine(0, max_chunk=a.max_chunk)
    ev = Events()
    res = {"max_chunk": eng.info()["max_chunk"], "arch": eng.info()["arch"], "warmup": a.warmup, "reps": a.reps,
           "prune_origins": PRUNE_M}
    for mix in ("repair", "gossip"):
        res[mix] = measure(eng, ed, ev, mix, a.packets, a.warmup, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
