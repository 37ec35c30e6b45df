#!/usr/bin/env python3
"""Times the proof-of-history check (fd_ed25519_hip_poh_dev and its three
launches, fd_ed25519_hip_poh_host) on one engine in one process; device-resident
inputs and HIP events for the device legs, the wall clock around the
synchronous call for the host legs:

  (a) --copies copies (default 4,096) of the batch the captured shreds carry
      (tests/golden/shreds.npz: 64 microblocks of hash_cnt 1 and 20
      signatures): the leaf, tree and chain launches each, the whole
      poh_dev, poh_host, and poh_dev on the first n microblocks for n = 64,
      256, ... (the size at which the call overtakes 16 reference cores);
      beside them, in the same run, the seal's tree launch (fec_seal_dev
      without keys) on --sets sets of 32 + 32 captured shreds, both per
      SHA-256 block
  (b) 64 x --copies tick-only microblocks of hash_cnt 62,500: the chain
      launch alone; hashes/s against the instruction-count estimate
  (c) --blocks mainnet-shaped blocks: 64 ticks, each behind --entries entries
      of seeded hash counts and 1 to 3 signatures, k summing to 64 x 62,500 a
      block; poh_dev in block order and ordered by descending k (what
      poh_host does before upload)
  (d) one such block alone, both ways: the latency floor

Leg (b)'s one launch takes a sizeable fraction of a second; run it, and any
leg, in a process under a time limit of its own and collect the legs in one
file:

  timeout -k 10 400 python tools/poh_bench.py --legs a
  timeout -k 10 120 python tools/poh_bench.py --legs b --append
  timeout -k 10 180 python tools/poh_bench.py --legs cd --append

Every leg's codes are checked (all 0: every header hash is computed here with
hashlib, one block's worth, and repeated).  All legs are warmed up, then timed
--reps times; medians and the spread go to --out (profiles/poh_bench.json).

The estimate: the chain kernel's loop is CHAIN_VALU vector instructions a
hash (counted in the compiled kernel: 558 for rounds 0-31, 2 x 393 for rounds
32-63), a wave64 vector instruction is taken to issue in 4 cycles on one of
1,024 SIMDs at 2.4 GHz, so a full chip would do 1024 x 64 x 2.4e9 / (4 x
CHAIN_VALU) hashes/s.  The CPU figures are the fixture's
(tests/golden/poh.npz: the reference's fd_poh_append and 20-leaf root on one
core of the machine that made the fixture -- another machine than the GPU's
host).

  python tools/poh_bench.py [--copies N] [--blocks N] [--legs abcd [--append]] [--out PATH] [--label TEXT]
"""
import argparse
import ctypes
import hashlib
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
sys.path.insert(0, os.path.join(REPO, "tests"))

from precompile_bench import Events  # noqa: E402
from fec_recover_bench import captured_sets  # noqa: E402

CHAIN_VALU = 558 + 2 * 393
SIMDS, CLOCK, CYCLES_PER_VALU = 1024, 2.4e9, 4
TICK = 62500
SEED = 331


class Params(ctypes.Structure):
    """fd_ed25519_poh_params_t (fd_ed25519_hip_internal.h), field for field:
    the launches are timed one by one through the library's internal launch
    functions.  main() holds its size to the library's, and Batch.params()
    repeats front_work_poh's carve order (fd_front_work.h: leaves, roots,
    pre); both sites name this file.  A struct or an order that changed shows
    in the size check or in leg (a)'s codes, which are read after the three
    launches ran over these pointers."""
    _fields_ = [("buf", ctypes.c_void_p), ("buf_sz", ctypes.c_uint64), ("hdr_off", ctypes.c_void_p),
                ("in_off", ctypes.c_void_p), ("sig_first", ctypes.c_void_p), ("sig_off", ctypes.c_void_p),
                ("n", ctypes.c_uint64), ("n_sig", ctypes.c_uint64), ("hash_cnt_max", ctypes.c_uint64),
                ("leaves", ctypes.c_void_p), ("roots", ctypes.c_void_p), ("pre", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("out_hash", ctypes.c_void_p)]


class Batch:
    """descriptors on the device, with the launches over them"""

    def __init__(self, ed, eng, buf, hdr, inn, first, sig):
        self.ed, self.eng = ed, eng
        self.n, self.n_sig, self.size = len(hdr), len(sig), len(buf)
        self.host = (buf, hdr, inn, first, sig)
        self.d_buf = eng.alloc(self.size + 16).upload(buf)
        self.d_hdr, self.d_in = eng.alloc(8 * self.n).upload(hdr), eng.alloc(8 * self.n).upload(inn)
        self.d_first = eng.alloc(4 * self.n + 4).upload(first)
        self.d_sig = eng.alloc(8 * max(1, self.n_sig)).upload(sig if self.n_sig else np.zeros(1, np.uint64))
        self.d_out, self.d_hash = eng.alloc(self.n), eng.alloc(32 * self.n)
        self.d_work = eng.alloc(ed.poh_work_bytes(self.n, self.n_sig))

    def params(self):
        w = self.d_work.ptr
        return Params(self.d_buf.ptr, self.size, self.d_hdr.ptr, self.d_in.ptr, self.d_first.ptr, self.d_sig.ptr, self.n,
                      self.n_sig, self.ed.POH_HASH_CNT_CEIL, w, w + 32 * self.n_sig, w + 32 * self.n_sig + 32 * self.n,
                      self.d_out.ptr, self.d_hash.ptr)

    def launch(self, which):
        fn = getattr(self.ed._lib, "fd_ed25519_hip_launch_poh_" + which)
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        p = self.params()
        return lambda: self.check(fn(ctypes.byref(p), self.eng.stream))

    @staticmethod
    def check(rc):
        assert rc == 0, rc

    def dev(self, n=None):
        n = self.n if n is None else n
        n_sig = int(self.host[3][n])
        return lambda: self.eng.poh_dev(n, self.d_buf.ptr, self.size, self.d_hdr.ptr, self.d_in.ptr, self.d_first.ptr, n_sig,
                                        self.d_sig.ptr, self.ed.POH_HASH_CNT_CEIL, self.d_out.ptr, self.d_hash.ptr,
                                        self.d_work.ptr)

    def host_call(self):
        def run():
            t0 = time.perf_counter()
            codes, _ = self.eng.poh_host(*self.host)
            ms = (time.perf_counter() - t0) * 1e3
            assert not codes.any()
            return ms
        return run

    def codes(self):
        self.eng.sync()
        return self.d_out.download(np.int8, self.n)

    def free(self):
        for b in (self.d_buf, self.d_hdr, self.d_in, self.d_first, self.d_sig, self.d_out, self.d_hash, self.d_work):
            b.free()


def sha(b):
    return hashlib.sha256(b).digest()


def tree_nodes(leaves):
    """node hashes of a signature tree as the kernel performs them: a layer
    of m nodes makes ceil(m / 2), an odd layer's last node hashed with itself"""
    nodes = 0
    while leaves > 1:
        leaves = (leaves + 1) // 2
        nodes += leaves
    return nodes


def chain(state, k):
    for _ in range(k):
        state = sha(state)
    return state


def captured_batches(copies):
    """copies of the captured batch back to back, each behind the zero hash
    its first microblock chains from"""
    import poh_util as util
    d = util.captured()
    one = np.frombuffer(d.buf, np.uint8)
    size = (len(one) + 15) & ~15
    padded = np.zeros(size, np.uint8)
    padded[:len(one)] = one
    buf = np.tile(padded, copies)
    base = (np.arange(copies, dtype=np.uint64) * np.uint64(size))
    hdr = (base[:, None] + d.hdr_off[None, :]).reshape(-1)
    inn = (base[:, None] + d.in_off[None, :]).reshape(-1)
    sig = (base[:, None] + d.sig_off[None, :]).reshape(-1)
    per = len(d.sig_off)
    first = (np.arange(copies, dtype=np.uint64)[:, None] * per + d.sig_first[None, :-1]).reshape(-1)
    first = np.append(first, copies * per).astype(np.uint32)
    return buf, hdr, inn, first, sig


def ticks(copies, distinct=8):
    """64 x copies tick-only microblocks of hash_cnt TICK, `distinct` of them
    computed (each from a seeded state of its own) and repeated"""
    rng = random.Random(SEED)
    buf = bytearray()
    for _ in range(distinct):
        state = bytes(rng.getrandbits(8) for _ in range(32))
        buf += state + struct.pack("<Q", TICK) + chain(state, TICK) + struct.pack("<Q", 0)
    n = 64 * copies
    which = np.arange(n, dtype=np.uint64) % np.uint64(distinct)
    inn = which * np.uint64(80)
    return (np.frombuffer(bytes(buf), np.uint8), inn + np.uint64(32), inn, np.zeros(n + 1, np.uint32), np.zeros(0, np.uint64))


def mainnet_block(entries):
    """one block, chained from a seeded hash: 64 ticks, each behind `entries`
    entries; an entry has a seeded hash_cnt and 1 to 3 transactions of one
    signature, the tick the rest of its 62,500 -> (bytes with the in hash in
    front, hdr_off, in_off, sig_first, sig_off, k)"""
    import poh_model as model
    import poh_util as util
    rng = random.Random(SEED + 1)
    state = state0 = bytes(rng.getrandbits(8) for _ in range(32))
    out, ks = [struct.pack("<Q", 64 * (entries + 1))], []
    for _ in range(64):
        left = TICK
        for _ in range(entries):
            hash_cnt = rng.randrange(1, TICK // (entries + 1))      # the tick keeps the rest, 1 / (entries + 1) at least
            left -= hash_cnt
            mb, state2 = util.make_microblock(rng, state, hash_cnt, rng.randrange(1, 4))
            out.append(mb); ks.append(hash_cnt - 1); state = state2
        mb, state2 = util.make_microblock(rng, state, left, 0)
        out.append(mb); ks.append(left); state = state2
    blk = b"".join(out)
    d = util.describe(blk, state0)
    buf = d.buf
    assert sum(ks) + 64 * entries == 64 * TICK and model.walk(blk)[0] == 0
    return np.frombuffer(buf, np.uint8), d.hdr_off, d.in_off, d.sig_first, d.sig_off, np.array(ks, np.uint64)


def repeat_block(block, copies, order):
    """copies of the block's descriptors over the same bytes; order "block"
    or "k" (descending k over the whole batch, as poh_host orders)"""
    buf, hdr, inn, first, sig, ks = block
    n1 = len(hdr)
    pick = np.tile(np.arange(n1), copies)
    if order == "k":
        pick = pick[np.argsort(-np.tile(ks, copies).astype(np.int64), kind="stable")]
    cnt = np.diff(first.astype(np.int64))[pick]
    new_first = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    new_sig = np.concatenate([sig[first[i]:first[i + 1]] for i in pick]) if len(sig) else sig
    return buf, hdr[pick], inn[pick], new_first, new_sig.astype(np.uint64)


def timed(ev, stream, legs, warmup, reps):
    for _ in range(warmup):
        for f in legs.values():
            f()
    t = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():
            t[k].append(ev.time_ms(stream, f))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=4096)
    ap.add_argument("--sets", type=int, default=4096)
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--entries", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="abcd")
    ap.add_argument("--append", action="store_true", help="keep the legs --out already holds (a leg run in a process of its own)")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "poh_bench.json"))
    a = ap.parse_args()
    from firedancer_amd import ed25519 as ed

    if ed.device_count() < 1:
        sys.exit("poh_bench: no GPU (this tool measures; it has no CPU mode)")
    g = np.load(os.path.join(REPO, "tests", "golden", "poh.npz"))
    ref_hash, ref_root20, ref_cpu = float(g["ref_hash_rate"]), float(g["ref_root20_rate"]), str(g["ref_cpu"])
    est = SIMDS * 64 * CLOCK / (CYCLES_PER_VALU * CHAIN_VALU)
    ed._lib.fd_ed25519_hip_private_poh_params_bytes.restype = ctypes.c_uint
    assert ctypes.sizeof(Params) == ed._lib.fd_ed25519_hip_private_poh_params_bytes(), "Params is not the library's struct"
    eng = ed.Engine(0)
    ev, stream = Events(), eng.stream
    res = {"label": a.label, "arch": eng.info()["arch"], "warmup": a.warmup, "reps": a.reps,
           "reference_cpu": ref_cpu, "reference_append_hashes_per_s_one_core": ref_hash,
           "reference_root20_per_s_one_core": ref_root20, "reference_measured_on": "the machine that made tests/golden/poh.npz",
           "chain_valu_per_hash": CHAIN_VALU, "assumed": {"simds": SIMDS, "clock_hz": CLOCK, "cycles_per_wave64_valu": CYCLES_PER_VALU},
           "estimated_chain_hashes_per_s": est}
    all_ms = {}

    def med(t):
        return {k: round(statistics.median(v), 4) for k, v in t.items()}

    def keep(name, t):
        all_ms[name] = {k: [round(x, 4) for x in v] for k, v in t.items()}

    if "a" in a.legs:
        b = Batch(ed, eng, *captured_batches(a.copies))
        b.dev()()
        assert not b.codes().any(), "every captured microblock must verify"
        legs = {"leaf": b.launch("leaf"), "tree": b.launch("tree"), "chain": b.launch("chain")}
        for f in legs.values():     # the three launches over Batch.params()'s pointers give what poh_dev gives
            f()
        assert not b.codes().any(), "the launches over the mirrored layout must verify every microblock"
        legs["poh_dev"] = b.dev()
        # the seal's tree launch on captured sets, in the same run
        fx = np.load(os.path.join(REPO, "tests", "golden", "shreds.npz"))
        base = [[bytearray(s) for s in st] for st in captured_sets(fx)]
        n_set, n = a.sets, a.sets * 64
        whole = np.concatenate([np.frombuffer(b"".join(bytes(s) for s in base[k % 6]), np.uint8) for k in range(n_set)] +
                               [np.zeros(16, np.uint8)])
        sz = np.concatenate([np.array([len(x) for x in base[k % 6]], np.uint32) for k in range(n_set)])
        off = np.concatenate([[0], np.cumsum(sz.astype(np.uint64))[:-1]]).astype(np.uint64)
        s_buf, s_off, s_sz = eng.alloc(len(whole)).upload(whole), eng.alloc(8 * n).upload(off), eng.alloc(4 * n).upload(sz)
        s_first = eng.alloc(4 * (n_set + 1)).upload((np.arange(n_set + 1) * 64).astype(np.uint32))
        s_work, s_set = eng.alloc(ed.fec_work_bytes(n, n_set)), eng.alloc(n_set)
        legs["seal_tree"] = lambda: eng.fec_seal_dev(n, s_buf.ptr, s_off.ptr, s_sz.ptr, n_set, s_first.ptr, None, s_work.ptr,
                                                     s_set.ptr)
        t = timed(ev, stream, legs, a.warmup, a.reps)
        eng.sync()
        assert not s_set.download(np.int8, n_set).any()
        m = med(t)
        # SHA-256 blocks: a 65-byte message is two; a tree of 20 leaves is 10 + 5 + 3 + 2 + 1 = 21 nodes; a shred leaf
        # of depth 6 is 17 (26 + 1019 or 1044 bytes and the padding), a set of 64 has 63 nodes
        assert tree_nodes(20) == 21 and tree_nodes(64) == 63 and b.n_sig == 20 * b.n
        leaf_blocks, tree_blocks = 2 * b.n_sig, 2 * tree_nodes(20) * b.n
        seal_blocks = n_set * (64 * 17 + 63 * 2)
        host_ms = [b.host_call()() for _ in range(max(2, a.reps // 2))][1:]
        sweep = {}
        sizes = [s for s in (64, 256, 1024, 4096, 16384, 65536, 262144) if s <= b.n]
        st = timed(ev, stream, {str(s): b.dev(s) for s in sizes}, a.warmup, a.reps)
        cpu16 = 16 * ref_root20      # microblocks/s: the 20-leaf root is all but one hash of such a microblock
        for s in sizes:
            ms = statistics.median(st[str(s)])
            sweep[str(s)] = {"poh_dev_ms": round(ms, 4), "sixteen_reference_cores_ms": round(s / cpu16 * 1e3, 4)}
        over = next((s for s in sizes if sweep[str(s)]["poh_dev_ms"] < sweep[str(s)]["sixteen_reference_cores_ms"]), None)
        res["a"] = {"copies": a.copies, "microblocks": b.n, "signatures": b.n_sig, "ms": m,
                    "poh_host_ms": round(statistics.median(host_ms), 2),
                    "leaf_sha256_blocks": leaf_blocks, "tree_sha256_blocks": tree_blocks, "seal_tree_sha256_blocks": seal_blocks,
                    "leaf_ns_per_sha256_block": round(m["leaf"] * 1e6 / leaf_blocks, 4),
                    "tree_ns_per_sha256_block": round(m["tree"] * 1e6 / tree_blocks, 4),
                    "seal_tree_sets": n_set, "seal_tree_ns_per_sha256_block": round(m["seal_tree"] * 1e6 / seal_blocks, 4),
                    "leaf_over_seal_tree_per_block": round(m["leaf"] / leaf_blocks / (m["seal_tree"] / seal_blocks), 4),
                    "tree_over_seal_tree_per_block": round(m["tree"] / tree_blocks / (m["seal_tree"] / seal_blocks), 4),
                    "microblocks_per_s_poh_dev": round(b.n / m["poh_dev"] * 1e3),
                    "microblocks_per_s_sixteen_reference_cores": round(cpu16),
                    "first_n_microblocks": sweep, "poh_dev_overtakes_sixteen_reference_cores_at": over}
        keep("a", t); keep("a_first_n", st)
        all_ms["a"]["poh_host"] = [round(x, 2) for x in host_ms]
        b.free()
        for x in (s_buf, s_off, s_sz, s_first, s_work, s_set):
            x.free()

    if "b" in a.legs:
        b = Batch(ed, eng, *ticks(a.copies))
        t = timed(ev, stream, {"chain": b.launch("chain")}, 1, max(3, a.reps // 2))
        assert not b.codes().any(), "every tick must verify"
        m = med(t)
        rate = b.n * TICK / m["chain"] * 1e3
        res["b"] = {"microblocks": b.n, "hash_cnt": TICK, "hashes": b.n * TICK, "chain_ms": m["chain"],
                    "hashes_per_s": round(rate), "over_estimate": round(rate / est, 4),
                    "over_one_reference_core": round(rate / ref_hash, 2), "over_sixteen_reference_cores": round(rate / ref_hash / 16, 2)}
        keep("b", t)
        b.free()

    if "c" in a.legs or "d" in a.legs:
        block = mainnet_block(a.entries)
        for leg, copies in (("c", a.blocks), ("d", 1)):
            if leg not in a.legs:
                continue
            bs = {order: Batch(ed, eng, *repeat_block(block, copies, order)) for order in ("block", "k")}
            t = timed(ev, stream, {order: b.dev() for order, b in bs.items()}, 1, max(3, a.reps // 2))
            for b in bs.values():
                assert not b.codes().any(), "every microblock of the block must verify"
            m = med(t)
            hashes = copies * 64 * TICK
            entry = {"blocks": copies, "microblocks": bs["k"].n, "signatures": bs["k"].n_sig, "chain_hashes": hashes,
                     "poh_dev_block_order_ms": m["block"], "poh_dev_ordered_by_k_ms": m["k"],
                     "ordered_over_block_order": round(m["k"] / m["block"], 4),
                     "hashes_per_s_ordered": round(hashes / m["k"] * 1e3),
                     "one_reference_core_ms": round(hashes / ref_hash * 1e3, 2),
                     "sixteen_reference_cores_ms": round(hashes / ref_hash / 16 * 1e3, 2)}
            if leg == "d":
                entry["poh_host_ms"] = round(statistics.median([bs["block"].host_call()() for _ in range(3)]), 2)
                entry["longest_chain_hashes"] = int(block[5].max())
                entry["us_per_dependent_hash"] = round(m["k"] * 1e3 / int(block[5].max()), 4)
            res[leg] = entry
            keep(leg, t)
            for b in bs.values():
                b.free()

    if a.append and os.path.exists(a.out):
        old = json.load(open(a.out))
        all_ms = {**old.pop("all_ms", {}), **all_ms}
        res = {**old, **res}
    res["all_ms"] = all_ms
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "all_ms"}))
    eng.close()


if __name__ == "__main__":
    main()
