"""What the shredder tests share: the cases of tests/golden/shredder.npz (the
reference shredder's own sets, tests/golden/gen_shredder.py) and the
device-resident run of fd_ed25519_hip_shredder_front_dev / _dev in
guard-filled buffers."""
import functools
import hashlib
import random

import numpy as np

import shredder_model as model
from conftest import load_golden

GUARD = 0x5A


@functools.lru_cache(maxsize=None)
def fixture_cases():
    """((batch bytes, descriptor, counts, [(d, p)], [digest of every shred]) per batch) per case"""
    g = load_golden("shredder")
    assert str(g["rule"]) == "batch b = random.Random( seed[b] ).randbytes( sz[b] )"
    out, at = [], 0
    for c in range(len(g["case_first"]) - 1):
        case = []
        for b in range(int(g["case_first"][c]), int(g["case_first"][c + 1])):
            dsc = model.desc(int(g["slot"][b]), int(g["data_idx"][b]), int(g["parity_idx"][b]), int(g["version"][b]),
                             int(g["parent_off"][b]), int(g["reference_tick"][b]), int(g["block_complete"][b]))
            dp = [tuple(int(x) for x in r) for r in g["dp"][int(g["set_first"][b]):int(g["set_first"][b + 1])]]
            n = sum(d + p for d, p in dp)
            case.append((model.seeded_batch(int(g["seed"][b]), int(g["sz"][b])), dsc, tuple(int(x) for x in g["counts"][b]), dp,
                         [g["digest"][at + i].tobytes() for i in range(n)]))
            at += n
        out.append(tuple(case))
    assert at == len(g["digest"])
    return tuple(out)


def whole_shreds():
    """the reference's whole shreds of the first cases, in order"""
    g = load_golden("shredder")
    raw, at, out = g["whole"].tobytes(), 0, []
    for case in fixture_cases()[:int(g["whole_cases"])]:
        for _, _, _, dp, _ in case:
            for d, p in dp:
                for sz in [1203] * d + [1228] * p:
                    out.append(raw[at:at + sz])
                    at += sz
    assert at == len(raw)
    return out


def ed_desc(ed, dsc):
    return ed.shredder_desc(**dsc)


def blank_front(sets):
    """finished sets as the front alone leaves them: signature, proof and parity region zero"""
    out = []
    for st in sets:
        depth = (len(st) - 1).bit_length()
        P = 1139 - 20 * depth
        row = []
        for s in st:
            if s[0x40] & 0xF0 == 0x80:
                row.append(bytes(64) + s[64:1203 - 20 * depth] + bytes(20 * depth))
            else:
                row.append(bytes(64) + s[64:0x59] + bytes(P) + bytes(20 * depth))
        out.append(row)
    return out


class Reservation:
    """batches with the sets and shreds shredder_count reserves for them, or what `reserve` says instead"""

    def __init__(self, sizes, reserve=None):
        self.set_first_b, self.shred_first_b = [0], [0]
        for b, sz in enumerate(sizes):
            sets, nd, npar = model.count(sz)
            if reserve and b in reserve:
                sets, shreds = reserve[b]
            else:
                shreds = nd + npar
            self.set_first_b.append(self.set_first_b[-1] + sets)
            self.shred_first_b.append(self.shred_first_b[-1] + shreds)
        self.n_set, self.n = self.set_first_b[-1], self.shred_first_b[-1]


def run_front(eng, ed, batches, descs, res, base_off=16, stride=1229, lead=0, gap=3, privs=None, seal=False, leave=(),
              set_first_b=None, shred_first_b=None, tail=5):
    """fd_ed25519_hip_shredder_front_dev (seal False) or _dev on batches laid
    `gap` guard bytes apart from byte `lead` of buf; a batch in `leave` claims
    to run past buf_sz.  Every output stands in a guard-filled buffer with
    `tail` spare entries.  Returns a dict of what came back."""
    nb, n_set, n = len(batches), res.n_set, res.n
    buf, off = bytearray([GUARD] * lead), []
    for b in batches:
        off.append(len(buf))
        buf += bytes(b) + bytes([GUARD] * gap)
    buf_sz = len(buf)
    sizes = [len(b) for b in batches]
    for b in leave:
        sizes[b] = buf_sz - off[b] + 1
    sfb = res.set_first_b if set_first_b is None else set_first_b
    hfb = res.shred_first_b if shred_first_b is None else shred_first_b
    shred_bytes = base_off + stride * n + 64
    desc = np.concatenate([ed_desc(ed, d) for d in descs]) if nb else np.zeros(1, ed.SHREDDER_DESC)
    bufs = {}

    def dev(name, arr):
        arr = np.ascontiguousarray(arr)
        bufs[name] = eng.alloc(max(arr.nbytes, 16)).upload(arr)
        return bufs[name].ptr

    p_buf = dev("buf", np.frombuffer(bytes(buf) + bytes(32), np.uint8))
    p_off, p_sz = dev("off", np.array(off + [0], np.uint64)), dev("sz", np.array(sizes + [0], np.uint32))
    p_desc = dev("desc", desc)
    p_sfb, p_hfb = dev("sfb", np.array(sfb, np.uint32)), dev("hfb", np.array(hfb, np.uint32))
    p_shreds = dev("shreds", np.full(shred_bytes, GUARD, np.uint8))
    p_soff = dev("shred_off", np.full(n + tail, 0x5A5A5A5A5A5A5A5A, np.uint64))
    p_ssz = dev("shred_sz", np.full(n + tail, 0x5A5A5A5A, np.uint32))
    p_first = dev("set_first", np.full(n_set + 1 + tail, 0x5A5A5A5A, np.uint32))
    p_bout = dev("batch_out", np.full(nb + tail, GUARD, np.int8))
    args = (nb, p_buf, buf_sz, p_off, p_sz, p_desc, p_sfb, p_hfb, n_set, n, p_shreds, base_off, stride, p_soff, p_ssz, p_first, p_bout)
    if seal:
        p_privs = dev("privs", np.frombuffer(b"".join(privs), np.uint8)) if privs is not None else None
        p_work = dev("work", np.zeros(ed.shredder_work_bytes(n, n_set), np.uint8))
        p_sout = dev("set_out", np.full(n_set + tail, GUARD, np.int8))
        p_roots = dev("roots", np.full(32 * (n_set + tail), GUARD, np.uint8))
        p_sigs = dev("sigs", np.full(64 * (n_set + tail), GUARD, np.uint8)) if privs is not None else None
        eng.shredder_dev(*args, p_privs, p_work, p_sout, p_roots, p_sigs)
    else:
        eng.shredder_front_dev(*args)
    eng.sync()
    out = dict(shreds=bufs["shreds"].download(np.uint8, shred_bytes).tobytes(),
               shred_off=bufs["shred_off"].download(np.uint64, n + tail), shred_sz=bufs["shred_sz"].download(np.uint32, n + tail),
               set_first=bufs["set_first"].download(np.uint32, n_set + 1 + tail),
               batch_out=bufs["batch_out"].download(np.int8, nb + tail), bufs=bufs, n=n, n_set=n_set, nb=nb, tail=tail,
               base_off=base_off, stride=stride, shred_bytes=shred_bytes)
    if seal:
        out["set_out"] = bufs["set_out"].download(np.int8, n_set + tail)
        out["roots"] = bufs["roots"].download(np.uint8, 32 * (n_set + tail))
        if privs is not None:
            out["sigs"] = bufs["sigs"].download(np.uint8, 64 * (n_set + tail))
    return out


def free(out):
    for b in out["bufs"].values():
        b.free()


def expect_layout(out, res, batch_sets, codes):
    """the guard-filled buffers as the model lays them out: batch_sets[b] the
    model's sets of batch b as the call under test leaves them (None for a
    batch with a code) -- every other byte a guard byte"""
    n, n_set, nb, tail, base, stride = out["n"], out["n_set"], out["nb"], out["tail"], out["base_off"], out["stride"]
    shreds = bytearray([GUARD] * out["shred_bytes"])
    soff = np.full(n + tail, 0x5A5A5A5A5A5A5A5A, np.uint64)
    ssz = np.full(n + tail, 0x5A5A5A5A, np.uint32)
    ssz[:n] = 0
    first = np.full(n_set + 1 + tail, 0x5A5A5A5A, np.uint32)
    first[n_set] = n
    bout = np.full(nb + tail, GUARD, np.int8)
    bout[:nb] = codes
    keep = []   # (start, bytes) of every parity region, which the front does not write
    for b in range(nb):
        s0, s1, h0, h1 = res.set_first_b[b], res.set_first_b[b + 1], res.shred_first_b[b], res.shred_first_b[b + 1]
        if codes[b]:
            for k in range(s0, s1):
                first[k] = min(h0 if k == s0 else h1, n)
            continue
        i = h0
        for k, st in zip(range(s0, s1), batch_sets[b]):
            first[k] = i
            for s in st:
                at = base + stride * i
                shreds[at:at + len(s)] = s
                soff[i], ssz[i] = at, len(s)
                i += 1
        assert i == h1
    return dict(shreds=bytes(shreds), shred_off=soff, shred_sz=ssz, set_first=first, batch_out=bout)


def assert_layout(out, want, parity_untouched=False):
    for k in ("shred_off", "shred_sz", "set_first", "batch_out"):
        assert out[k].tolist() == want[k].tolist(), k
    got, exp = out["shreds"], want["shreds"]
    if parity_untouched:
        # the front leaves [0x59, 0x59 + P) of a parity shred alone: guard bytes there
        exp = bytearray(exp)
        n, base, stride = out["n"], out["base_off"], out["stride"]
        first = want["set_first"]
        for k in range(out["n_set"]):
            a, z = int(first[k]), int(first[k + 1])
            if not (a < z <= n) or want["shred_sz"][a] == 0:
                continue
            P = 1139 - 20 * (z - a - 1).bit_length()
            for i in range(a, z):
                if want["shred_sz"][i] == 1228:
                    at = base + stride * i + 0x59
                    exp[at:at + P] = bytes([GUARD] * P)
        exp = bytes(exp)
    if got != exp:
        at = next(i for i in range(len(exp)) if got[i] != exp[i])
        i = (at - out["base_off"]) // out["stride"]
        raise AssertionError(f"byte {at} of the shred buffer differs: shred {i}, byte {at - out['base_off'] - out['stride'] * i}")


def digests(sets):
    return [hashlib.sha256(s).digest() for st in sets for s in st]


def keys(seed, count):
    rng = random.Random(seed)
    return [rng.randbytes(32) for _ in range(count)]


def parity_and_seal(eng, ed, out, set_keys=None):
    """fec_parity_dev and fec_seal_dev over the arrays a front_dev run left on
    the device, then one sync -> (parity codes, seal codes, the shred buffer)"""
    n, n_set, bufs = out["n"], out["n_set"], out["bufs"]
    pout = eng.alloc(n_set + 16).upload(np.full(n_set + 16, GUARD, np.int8))
    sout = eng.alloc(n_set + 16).upload(np.full(n_set + 16, GUARD, np.int8))
    work = eng.alloc(ed.fec_work_bytes(n, n_set))
    privs = eng.alloc(32 * max(1, n_set)).upload(np.frombuffer(b"".join(set_keys), np.uint8)) if set_keys is not None else None
    eng.fec_parity_dev(n, bufs["shreds"].ptr, bufs["shred_off"].ptr, bufs["shred_sz"].ptr, n_set, bufs["set_first"].ptr, pout.ptr)
    eng.fec_seal_dev(n, bufs["shreds"].ptr, bufs["shred_off"].ptr, bufs["shred_sz"].ptr, n_set, bufs["set_first"].ptr,
                     privs.ptr if privs is not None else None, work.ptr, sout.ptr)
    eng.sync()
    got = (pout.download(np.int8, n_set).tolist(), sout.download(np.int8, n_set).tolist(),
           bufs["shreds"].download(np.uint8, out["shred_bytes"]).tobytes())
    for b in (pout, sout, work, privs):
        if b is not None:
            b.free()
    return got
