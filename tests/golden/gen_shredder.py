"""Makes tests/golden/shredder.npz: the reference shredder's own FEC sets of
seeded entry batches, at every edge of its counting rules.

    python tests/golden/gen_shredder.py <reference>/src

gen_shredder_ref.c, this project's own harness, is compiled in a temporary
directory against the reference's sources the way gen_reedsol.py and
gen_poh.py compile theirs.  It drives fd_shredder_new / _skip_batch /
_init_batch / _next_fec_set and the fd_shredder_count_* functions with a
signer that writes 64 zero bytes, so front + parity + seal without keys must
give the reference's whole shreds.

A case is one slot: one batch, or two chained in the slot.  Batch b is
random.Random( seed[b] ).randbytes( sz[b] ) (`rule`); only seed and size are
stored.

  case_first[cases+1]   the batches of case c: [case_first[c], case_first[c+1])
  sz, seed              per batch
  slot, data_idx, parity_idx, version, parent_off (before the reference's
  cast to 16 bits), reference_tick, block_complete
                        per batch: the descriptor; data_idx and parity_idx
                        are what the slot's earlier batches leave
  counts[batches][3]    fd_shredder_count_fec_sets / _data_shreds /
                        _parity_shreds
  set_first[batches+1]  the sets of batch b in dp
  dp[sets][2]           every set's (d, p)
  digest[shreds][32]    SHA-256 of every shred, set by set in tree order
  whole                 the shreds of the first WHOLE cases, back to back

The generator asserts the test-side model (tests/shredder_model.py on
reedsol_model and fec_model) on every case before writing.  Nothing here is
run by a test."""
import hashlib
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

SEED = 311
SIZE_LIMIT = 1 << 20    # of a committed file
WHOLE = 3
RULE = "batch b = random.Random( seed[b] ).randbytes( sz[b] )"
SIZES = (1, 1015, 1016, 9135, 9136, 31840, 31841, 62400, 62401, 63679, 63680, 63681, 95520)
# (block_complete, reference_tick, parent_off)
VARIANTS = ((0, 0, 1), (1, 63, 2), (1, 64, 0x1FFFF))
# a batch fd_shredder_skip_batch turns into 0xFFFFFFF0 data and as many parity shreds: 134,217,726 sets of 32 + 32 and one of 48 + 48
WRAP_SKIP = 134217726 * 31840 + 46800
REF_C = ["disco/shred/fd_shredder.c", "ballet/bmtree/fd_bmtree.c", "ballet/sha256/fd_sha256.c", "ballet/sha256/fd_sha256_batch_avx.c",
         "util/log/fd_log.c", "util/cstr/fd_cstr.c", "util/env/fd_env.c", "util/io/fd_io.c", "util/tile/fd_tile.c"]


def cases():
    """[(slot, version, skip_sz, [(parent_off, tick, block_complete, sz)])]"""
    out = []
    for i, sz in enumerate(SIZES):
        bc, tick, parent = VARIANTS[i % 3]
        out.append((3 + i, 0x1234 + i, 0, [(parent, tick, bc, sz)]))
    out.append((5, 0, 0, [(0, 0, 0, 237320), (0, 0, 1, 1016)]))
    out.append((0xFFFFFFFFFFFF, 0xFFFF, WRAP_SKIP, [(1, 5, 1, 63681)]))
    return out


def run_reference(ref, blob):
    from gen_packets import ref_defs
    from gen_reedsol import reference_sources
    root = os.path.dirname(os.path.abspath(ref))
    ref = os.path.abspath(ref)
    with tempfile.TemporaryDirectory() as tmp:
        exe, objs, jobs = os.path.join(tmp, "gen_shredder_ref"), [], []
        for src in REF_C + reference_sources(ref) + [os.path.join(HERE, "gen_shredder_ref.c")]:
            obj = os.path.join(tmp, os.path.basename(src)[:-2] + ".o")
            jobs.append(subprocess.Popen(["gcc"] + ref_defs(ref) + ["-march=haswell", "-O1", "-c", os.path.join(ref, src), "-o", obj],
                                         cwd=root))
            objs.append(obj)
        assert not any(j.wait() for j in jobs)
        subprocess.run(["gcc", "-pthread", "-o", exe] + objs + ["-lm"], check=True)
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(blob)
        subprocess.run([exe, fin, fout], check=True, cwd=root)
        return open(fout, "rb").read()


def main(ref):
    import shredder_model as model
    cs = cases()
    blob, seeds, seed = struct.pack("<I", len(cs)), [], SEED
    for slot, version, skip, batches in cs:
        blob += struct.pack("<QHQI", slot, version, skip, len(batches))
        for parent, tick, bc, sz in batches:
            blob += struct.pack("<QQII", parent, tick, bc, sz) + model.seeded_batch(seed, sz)
            seeds.append(seed)
            seed += 1
    raw, at = run_reference(ref, blob), 0
    rec = {k: [] for k in ("sz", "slot", "data_idx", "parity_idx", "version", "parent_off", "tick", "bc", "counts", "dp", "digest")}
    case_first, set_first, whole, nb = [0], [0], b"", 0
    for c, (slot, version, skip, batches) in enumerate(cs):
        _, D, C = model.count(skip)
        for parent, tick, bc, sz in batches:
            counts = struct.unpack_from("<III", raw, at)
            at += 12
            assert counts == model.count(sz), (sz, counts)
            dsc = model.desc(slot, D & 0xFFFFFFFF, C & 0xFFFFFFFF, version, parent, tick, bc)
            want = model.shred(None, model.seeded_batch(seeds[nb], sz), dsc, None)
            assert len(want) == counts[0]
            for st in want:
                d, p = struct.unpack_from("<II", raw, at)
                at += 8
                got = [raw[at + 1203 * i:at + 1203 * (i + 1)] for i in range(d)]
                at += 1203 * d
                got += [raw[at + 1228 * j:at + 1228 * (j + 1)] for j in range(p)]
                at += 1228 * p
                assert got == st, (c, sz, d, p, [i for i, (a, b) in enumerate(zip(got, st)) if a != b][:4])
                rec["dp"].append((d, p))
                rec["digest"] += [hashlib.sha256(s).digest() for s in got]
                if c < WHOLE:
                    whole += b"".join(got)
            for k, v in zip(("sz", "slot", "data_idx", "parity_idx", "version", "parent_off", "tick", "bc", "counts"),
                            (sz, slot, D & 0xFFFFFFFF, C & 0xFFFFFFFF, version, parent, tick, bc, counts)):
                rec[k].append(v)
            set_first.append(len(rec["dp"]))
            D, C, nb = D + counts[1], C + counts[2], nb + 1
        case_first.append(nb)
    assert at == len(raw)
    out = os.path.join(HERE, "shredder.npz")
    np.savez_compressed(out, rule=np.array(RULE), case_first=np.array(case_first, np.uint32), sz=np.array(rec["sz"], np.uint32),
                        seed=np.array(seeds, np.uint32), slot=np.array(rec["slot"], np.uint64),
                        data_idx=np.array(rec["data_idx"], np.uint32), parity_idx=np.array(rec["parity_idx"], np.uint32),
                        version=np.array(rec["version"], np.uint16), parent_off=np.array(rec["parent_off"], np.uint32),
                        reference_tick=np.array(rec["tick"], np.uint8), block_complete=np.array(rec["bc"], np.uint8),
                        counts=np.array(rec["counts"], np.uint32), set_first=np.array(set_first, np.uint32),
                        dp=np.array(rec["dp"], np.uint8), digest=np.frombuffer(b"".join(rec["digest"]), np.uint8).reshape(-1, 32),
                        whole=np.frombuffer(whole, np.uint8), whole_cases=np.array(WHOLE, np.uint32))
    size = os.path.getsize(out)
    print(out, size, "bytes,", len(cs), "cases,", nb, "batches,", len(rec["dp"]), "sets,", len(rec["digest"]), "shreds asserted")
    assert size <= SIZE_LIMIT, size


if __name__ == "__main__":
    main(sys.argv[1])
