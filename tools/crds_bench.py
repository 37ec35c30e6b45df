#!/usr/bin/env python3
"""Times the CRDS path (fd_ed25519_hip_crds_dev) against plain verification
of the same signatures (fd_ed25519_hip_verify_dev), device-resident inputs,
HIP events on one engine in one process, for two mixes of push messages that
hold --sigs values in all (default 262,144) back to back in one buffer:

  votes  three votes a packet (1,073 bytes): each a legacy transaction of one
         signature, two accounts and one instruction of 64 data bytes
  small  ten values a packet (1,226 bytes, filled to the size limit):
         version_v1, accounts_hashes of no hash, epoch_slots of no slots,
         version_v2 and node_instance, twice in turn

each value under a key of its own, its signature made by the device signer
over its data.  The last packet holds what is left of --sigs.

  crds_dev    walk + gather, the verify phases, finish (and, in a second
              timing, the hash pass of hash_out)
  verify_dev  the verify phases alone over the signatures, keys and messages
              one crds_dev call laid out in its workspace, the messages in
              place in the packet buffer

All are warmed up, then timed alternately --reps times; the medians and their
ratio (verify / crds: 1 would mean staging and finish are free) go to --out
(profiles/crds_bench.json), with the difference of the medians as the stage
and finish kernels' time and as the hash pass's.

  python tools/crds_bench.py [--sigs N] [--out PATH]
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

from packet_bench import signed_on_device  # noqa: E402
from precompile_bench import Events  # noqa: E402

HDR = 44   # message discriminant, pubkey, crds_len


def le(v, k):
    return np.frombuffer(int(v).to_bytes(k, "little"), np.uint8)


def vote_txn(rng):
    """a legacy transaction the parser accepts: one signature, the fee payer and the program, one instruction"""
    t = bytearray([1]) + rng.integers(0, 256, 64, dtype=np.uint8).tobytes() + bytes([1, 0, 1, 2]) + \
        rng.integers(0, 256, 64 + 32, dtype=np.uint8).tobytes() + bytes([1, 1, 1, 0, 64]) + rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
    return np.frombuffer(bytes(t), np.uint8)


def kinds_of(mix, rng):
    """the values of one full packet, in order: [(name, data bytes as a template, where the key lies in the data)]"""
    if mix == "votes":
        txn = vote_txn(rng)
        data = np.concatenate([le(1, 4), np.zeros(33, np.uint8), txn, np.zeros(8, np.uint8)])
        return [("vote", data, 5)] * 3
    five = [("version_v1", np.concatenate([le(6, 4), np.zeros(47, np.uint8)]), 4),
            ("accounts_hashes", np.concatenate([le(4, 4), np.zeros(48, np.uint8)]), 4),
            ("epoch_slots", np.concatenate([le(5, 4), np.zeros(49, np.uint8)]), 5),
            ("version_v2", np.concatenate([le(7, 4), np.zeros(51, np.uint8)]), 4),
            ("node_instance", np.concatenate([le(8, 4), np.zeros(56, np.uint8)]), 4)]
    return five * 2


def build(eng, mix, n_sig, rng):
    """(packet buffer, offsets, sizes, val_first) of push messages holding n_sig signed values"""
    kinds = kinds_of(mix, rng)
    per = len(kinds)
    privs = rng.integers(0, 256, 32 * n_sig, dtype=np.uint8)
    _, keys = signed_on_device(eng, np.zeros((n_sig, 16), np.uint8), np.zeros(n_sig, np.uint32), privs)   # the keys of these seeds
    width = max(len(d) for _, d, _ in kinds)
    pos = np.arange(n_sig) % per
    data, data_sz = np.zeros((n_sig, width), np.uint8), np.zeros(n_sig, np.int64)
    for j, (_, tmpl, key_at) in enumerate(kinds):
        rows = pos == j
        data[rows, :len(tmpl)] = tmpl
        data[rows, key_at:key_at + 32] = keys[rows]
        data[rows, len(tmpl) - 8:len(tmpl)] = rng.integers(0, 256, (int(rows.sum()), 8), dtype=np.uint8)   # a wallclock, a token
        if tmpl[0] in (6, 7):     # version_v1 / _v2: the option tag (absent) and, for v2, the feature set lie in the last 8
            data[rows, 4 + 46] = 0
        data_sz[rows] = len(tmpl)
    sigs, keys2 = signed_on_device(eng, data, data_sz, privs)
    assert (keys2 == keys).all() and len({bytes(s) for s in sigs[:4096]}) == 4096, "signatures must be distinct"
    vals = np.concatenate([sigs, data], axis=1)                   # [n_sig, 64 + width], each cut to 64 + its size below
    val_sz = 64 + data_sz
    flat = vals[np.arange(64 + width)[None, :] < val_sz[:, None]]
    cnt = np.full((n_sig + per - 1) // per, per, np.int64)
    cnt[-1] = n_sig - per * (len(cnt) - 1)
    first = np.concatenate([[0], np.cumsum(cnt)])
    val_end = np.cumsum(val_sz)
    body = np.concatenate([[0], val_end[first[1:] - 1]])          # value bytes in front of each packet
    out = []
    for i in range(len(cnt)):
        head = np.concatenate([le(2, 4), rng.integers(0, 256, 32, dtype=np.uint8), le(cnt[i], 8)])
        out.append(head)
        out.append(flat[body[i]:body[i + 1]])
    buf = np.concatenate(out)
    sz = HDR + np.diff(body)
    off = np.concatenate([[0], np.cumsum(sz)[:-1]]).astype(np.uint64)
    return buf, off, sz, first.astype(np.uint32), kinds


def measure(eng, ed, ev, mix, n_sig, warmup, reps):
    rng = np.random.default_rng(20261)
    self_key = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    buf, off, sz, first, kinds = build(eng, mix, n_sig, rng)
    n, total = len(sz), buf.size
    assert sz.max() <= ed.PACKET_MAX and first[-1] == n_sig
    d_buf = eng.alloc(total + 16).upload(buf)
    d_off = eng.alloc(8 * n).upload(off)
    d_sz = eng.alloc(4 * n).upload(sz.astype(np.uint32))
    d_first = eng.alloc(4 * n + 4).upload(first)
    d_work = eng.alloc(ed.crds_work_bytes(n, n_sig))
    d_pkt, d_val, d_codes, d_hash = eng.alloc(n), eng.alloc(n_sig), eng.alloc(n_sig), eng.alloc(32 * n_sig)

    def crds(hash_out=None):
        eng.crds_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, total, self_key, d_first.ptr, n_sig, d_work.ptr, d_pkt.ptr, d_val.ptr,
                     None, hash_out)

    def crds_hash():
        crds(d_hash.ptr)

    def verify():   # the arrays the stage kernel laid out (FD_ED25519_HIP_CRDS_WORK_BYTES's layout), the messages in place
        w = d_work.ptr
        eng.verify_dev(n_sig, d_buf.ptr, w + 96 * n_sig, w + 104 * n_sig, w, w + 64 * n_sig, d_codes.ptr)

    stream = eng.stream
    for _ in range(warmup):
        crds()
        crds_hash()
        verify()
    eng.sync()
    assert not d_pkt.download(np.int8, n).any() and not d_val.download(np.int8, n_sig).any(), "workload must verify"
    assert not d_codes.download(np.int8, n_sig).any() and d_hash.download(np.uint8, 32 * n_sig).reshape(-1, 32).any(axis=1).all()
    t_crds, t_hash, t_ver = [], [], []
    for _ in range(reps):
        t_crds.append(ev.time_ms(stream, crds))
        t_hash.append(ev.time_ms(stream, crds_hash))
        t_ver.append(ev.time_ms(stream, verify))
    c, h, v = statistics.median(t_crds), statistics.median(t_hash), statistics.median(t_ver)
    for b in (d_buf, d_off, d_sz, d_first, d_work, d_pkt, d_val, d_codes, d_hash):
        b.free()
    return {"signatures": n_sig, "packets": n, "packet_bytes": int(total), "values_per_packet": len(kinds),
            "kinds": [{"name": k[0], "bytes": 64 + len(k[1])} for k in kinds[:5 if mix == "small" else 1]],
            "crds_dev_ms": round(c, 4), "crds_dev_hash_ms": round(h, 4), "verify_dev_ms": round(v, 4),
            "crds_dev_ms_all": [round(x, 4) for x in t_crds], "crds_dev_hash_ms_all": [round(x, 4) for x in t_hash],
            "verify_dev_ms_all": [round(x, 4) for x in t_ver],
            "ratio_verify_over_crds": round(v / c, 4), "ratio_verify_over_crds_hash": round(v / h, 4),
            "stage_plus_finish_ms": round(c - v, 4), "hash_pass_ms": round(h - c, 4),
            "stage_read_GB_per_s": round(total / (c - v) / 1e6, 1) if c > v else None,
            "values_per_s": round(n_sig / c * 1e3), "verify_sigs_per_s": round(n_sig / v * 1e3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sigs", type=int, default=1 << 18)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max-chunk", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "crds_bench.json"))
    a = ap.parse_args()
    from firedancer_amd import ed25519 as ed

    if ed.device_count() < 1:
        sys.exit("crds_bench: no GPU (this tool measures; it has no CPU mode)")
    eng = ed.Engine(0, max_chunk=a.max_chunk)
    ev = Events()
    res = {"max_chunk": eng.info()["max_chunk"], "arch": eng.info()["arch"], "warmup": a.warmup, "reps": a.reps}
    for mix in ("votes", "small"):
        res[mix] = measure(eng, ed, ev, mix, a.sigs, a.warmup, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
