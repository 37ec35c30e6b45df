#!/usr/bin/env python3
"""Times the Ed25519 precompile path (fd_ed25519_hip_precompile_dev) against
plain verification of the same signatures (fd_ed25519_hip_verify_dev),
device-resident inputs, HIP events on one engine in one process:

  --txns transactions (default 65,536) of --entries entries (4) each, every
  entry a distinct key over a --msg-bytes (100) byte message, all inside one
  precompile instruction (signatures from the device generator);

  precompile_dev  parse + offsets walk + gather, the verify phases, finish
  verify_dev      the verify phases alone over the signatures, keys and
                  in-place messages one precompile_dev call gathered

Both are warmed up, then timed alternately --reps times; the medians and
their ratio (verify / precompile: 1 means staging and finish are free) go
to --out (profiles/precompile_bench.json), with the difference of the two
medians as the stage and finish kernels' time.

  python tools/precompile_bench.py [--txns N] [--out PATH]
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

B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"


def ed25519_program_id():
    n = 0
    for c in "Ed25519SigVerify111111111111111111111111111":
        n = n * 58 + B58.index(c)
    return n.to_bytes(32, "big")


def cu16(v):
    out = bytearray()
    while True:
        b, v = v & 0x7F, v >> 7
        out.append(b | 0x80 if v else b)
        if not v:
            return bytes(out)


def build_payloads(sigs, pubs, msgs, entries, msg_bytes):
    """[ntxn][L] uint8: one legacy transaction per `entries` signatures, one
    precompile instruction holding its table and every (sig, key, message)"""
    ntxn = len(sigs) // (64 * entries)
    item = 96 + msg_bytes
    data_sz = 2 + 14 * entries + item * entries
    table = bytes([entries, 0]) + b"".join(
        struct.pack("<7H", o, 0xFFFF, o + 64, 0xFFFF, o + 96, msg_bytes, 0xFFFF)
        for o in (2 + 14 * entries + item * i for i in range(entries)))
    head = (b"\x01" + bytes(64) +                       # one (unverified here) transaction signature
            bytes([1, 0, 1]) + cu16(2) + bytes(range(1, 33)) + ed25519_program_id() + b"\x07" * 32 +
            cu16(1) + bytes([1]) + cu16(0) + cu16(data_sz) + table)
    L = len(head) + item * entries
    assert L <= 1232, L
    pay = np.zeros((ntxn, L), np.uint8)
    pay[:, :len(head)] = np.frombuffer(head, np.uint8)
    for i in range(entries):
        at = len(head) + item * i
        pay[:, at:at + 64] = sigs.reshape(ntxn, entries, 64)[:, i]
        pay[:, at + 64:at + 96] = pubs.reshape(ntxn, entries, 32)[:, i]
        pay[:, at + 96:at + item] = msgs.reshape(ntxn, entries, msg_bytes)[:, i]
    return pay


class Events:
    """hipEvent timing through the HIP runtime the library already loaded"""

    def __init__(self):
        path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)
        self.hip = ctypes.CDLL(path)
        self.hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
        self.hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        for e in (self.a, self.b):
            assert self.hip.hipEventCreate(ctypes.byref(e)) == 0

    def time_ms(self, stream, fn):
        assert self.hip.hipEventRecord(self.a, stream) == 0
        fn()
        assert self.hip.hipEventRecord(self.b, stream) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = ctypes.c_float()
        assert self.hip.hipEventElapsedTime(ctypes.byref(ms), self.a, self.b) == 0
        return ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--txns", type=int, default=1 << 16)
    ap.add_argument("--entries", type=int, default=4)
    ap.add_argument("--msg-bytes", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max-chunk", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "precompile_bench.json"))
    a = ap.parse_args()
    from firedancer_amd import ed25519 as ed

    if ed.device_count() < 1:
        sys.exit("precompile_bench: no GPU (this tool measures; it has no CPU mode)")
    ntxn, n = a.txns, a.txns * a.entries
    eng = ed.Engine(0, max_chunk=a.max_chunk)
    dw = ed.DeviceWorkload(eng, n, a.msg_bytes, a.msg_bytes, 0, seed=20251)
    sigs, pubs = dw.sigs.download(np.uint8, 64 * n), dw.pubs.download(np.uint8, 32 * n)
    msgs = dw.msgs.download(np.uint8, a.msg_bytes * n)
    dw.free()
    pay = build_payloads(sigs, pubs, msgs, a.entries, a.msg_bytes)
    L = pay.shape[1]
    assert ed.precompile_count(pay[0].tobytes()) == a.entries
    d_pay = eng.alloc(pay.size + 16).upload(pay.reshape(-1))
    d_off = eng.alloc(8 * ntxn).upload(np.arange(ntxn, dtype=np.uint64) * L)
    d_sz = eng.alloc(4 * ntxn).upload(np.full(ntxn, L, np.uint32))
    d_first = eng.alloc(4 * (ntxn + 1)).upload(np.arange(ntxn + 1, dtype=np.uint32) * a.entries)
    d_work = eng.alloc(ed.precompile_work_bytes(ntxn, n))
    d_txn, d_instr, d_codes = eng.alloc(ntxn), eng.alloc(ntxn), eng.alloc(n)

    def precompile():
        eng.precompile_dev(ntxn, d_pay.ptr, d_off.ptr, d_sz.ptr, d_first.ptr, n, d_work.ptr, d_txn.ptr, d_instr.ptr)

    def verify():   # the arrays the stage kernel gathered (FD_ED25519_HIP_PRECOMPILE_WORK_BYTES's layout)
        w = d_work.ptr
        eng.verify_dev(n, d_pay.ptr, w + 96 * n, w + 104 * n, w, w + 64 * n, d_codes.ptr)

    ev, stream = Events(), eng.stream
    for _ in range(a.warmup):
        precompile()
        verify()
    eng.sync()
    assert not d_txn.download(np.int8, ntxn).any() and not d_codes.download(np.int8, n).any(), "workload must verify"
    t_pre, t_ver = [], []
    for _ in range(a.reps):
        t_pre.append(ev.time_ms(stream, precompile))
        t_ver.append(ev.time_ms(stream, verify))
    pre, ver = statistics.median(t_pre), statistics.median(t_ver)
    res = {"txns": ntxn, "entries_per_txn": a.entries, "signatures": n, "msg_bytes": a.msg_bytes, "payload_bytes": L,
           "max_chunk": eng.info()["max_chunk"], "arch": eng.info()["arch"], "warmup": a.warmup, "reps": a.reps,
           "precompile_dev_ms": round(pre, 4), "verify_dev_ms": round(ver, 4),
           "precompile_dev_ms_all": [round(x, 4) for x in t_pre], "verify_dev_ms_all": [round(x, 4) for x in t_ver],
           "ratio_verify_over_precompile": round(ver / pre, 4), "stage_plus_finish_ms": round(pre - ver, 4),
           "precompile_sigs_per_s": round(n / pre * 1e3), "verify_sigs_per_s": round(n / ver * 1e3)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
