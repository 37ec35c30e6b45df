"""Makes tests/golden/reedsol.npz: the reference encoder's own parity of seeded
data, for every number of data shreds.

    python tests/golden/gen_reedsol.py <reference>/src

gen_reedsol_ref.c, this project's own harness, is compiled in a temporary
directory against the reference's sources as gen_crds.py compiles its harness
and run with the reference's root as its working directory (the encoder's
constants are included from a path relative to it).  It encodes with
fd_reedsol_encode_init / _add_data_shred / _add_parity_shred / _fini.

  data[67][32]        seeded bytes
  parity[67][67][32]  parity[d-1][j] is parity shred j of the reference's
                      encoding of data[:d] with 67 parity shreds at shred_sz
                      32, the smallest the reference takes
  shredder_parity[68] the parity shreds the reference's shredder makes for d
                      data shreds (entry 0 unused)
  cases               how many (d, p, shred_sz) cases the generator asserted

What the generator itself holds to, for every pair (d, p) the shredder makes
-- (d, fd_shredder_data_to_parity_cnt[d]) for d <= 32 (fd_shredder.h:30-34),
(d, d) for 33 <= d <= 67 -- and for (d, 1), at shred_sz 32, 999 and 1019 (the
protected bytes of a shred at depth 7 and 6): the reference's p parity shreds
are the first p of its 67 for the same data, and both are the test-side
model's (tests/reedsol_model.py).  Nothing here is run by a test."""
import os
import random
import re
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

SEED = 149
SIZES = (32, 999, 1019)
SIZE_LIMIT = 1 << 20    # of a committed file


def reference_sources(ref):
    """the reference's Reed-Solomon library: every C file of ballet/reedsol and its wrapped_impl but the tests"""
    out = []
    for sub in ("ballet/reedsol", "ballet/reedsol/wrapped_impl"):
        out += [os.path.join(sub, f) for f in sorted(os.listdir(os.path.join(ref, sub)))
                if f.endswith(".c") and not f.startswith(("test_", "fuzz_"))]
    return out


def shredder_parity_table(ref):
    """[the parity shreds the shredder makes for d data shreds], d = 0..67: fd_shredder_data_to_parity_cnt
    (fd_shredder.h:30-34) read from the reference's header for d <= 32, d beyond"""
    text = open(os.path.join(ref, "disco/shred/fd_shredder.h")).read()
    body = re.search(r"fd_shredder_data_to_parity_cnt\[ 33UL \] = \{([^}]*)\}", text).group(1)
    table = [int(v) for v in re.findall(r"(\d+)UL", body)]
    assert len(table) == 33 and table[0] == 0 and table[32] == 32
    return table + list(range(33, 68))


def encode_with_reference(ref, cases):
    """[[parity shred]] of [(p, [data shred])]"""
    from gen_packets import ref_defs
    root = os.path.dirname(os.path.abspath(ref))
    with tempfile.TemporaryDirectory() as tmp:
        exe, objs = os.path.join(tmp, "gen_reedsol_ref"), []
        ref, jobs = os.path.abspath(ref), []
        for src in reference_sources(ref) + [os.path.join(HERE, "gen_reedsol_ref.c")]:
            obj = os.path.join(tmp, os.path.basename(src)[:-2] + ".o")
            # -O1 after REF_DEFS' -O3: the unrolled transforms are long
            jobs.append(subprocess.Popen(["gcc"] + ref_defs(ref) + ["-march=haswell", "-O1", "-c", os.path.join(ref, src), "-o", obj],
                                         cwd=root))
            objs.append(obj)
        assert not any(j.wait() for j in jobs)
        subprocess.run(["gcc", "-pthread", "-o", exe] + objs + ["-lm"], check=True)
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<I", len(cases)))
            for p, data in cases:
                f.write(struct.pack("<III", len(data), p, len(data[0])) + b"".join(data))
        subprocess.run([exe, fin, fout], check=True, cwd=root)
        raw, at, out = open(fout, "rb").read(), 0, []
        for p, data in cases:
            sz = len(data[0])
            out.append([raw[at + sz * j:at + sz * (j + 1)] for j in range(p)])
            at += sz * p
        assert at == len(raw)
        return out


def main(ref):
    import reedsol_model as model
    rng = random.Random(SEED)
    data = {sz: [bytes(rng.getrandbits(8) for _ in range(sz)) for _ in range(67)] for sz in SIZES}
    shredder_p = shredder_parity_table(ref)
    pairs = [(d, shredder_p[d]) for d in range(1, 68)] + [(d, 1) for d in range(1, 68)]
    cases, what = [], []
    for sz in SIZES:
        for d in range(1, 68):
            cases.append((67, data[sz][:d]))
            what.append(("full", sz, d, 67))
        for d, p in pairs:
            cases.append((p, data[sz][:d]))
            what.append(("pair", sz, d, p))
    got = encode_with_reference(ref, cases)
    full, asserted, failed = {}, 0, []
    for (kind, sz, d, p), par in zip(what, got):
        if kind == "full":
            full[(sz, d)] = par
            assert par == model.encode(data[sz][:d], 67), (sz, d)
    for (kind, sz, d, p), par in zip(what, got):
        if kind == "pair":
            asserted += 1
            if par != full[(sz, d)][:p] or par != model.encode(data[sz][:d], p):
                failed.append((d, p, sz))
    assert not failed, failed
    assert asserted == len(pairs) * len(SIZES)
    out = os.path.join(HERE, "reedsol.npz")
    np.savez_compressed(out, data=np.frombuffer(b"".join(data[32]), np.uint8).reshape(67, 32),
                        parity=np.frombuffer(b"".join(b"".join(full[(32, d)]) for d in range(1, 68)), np.uint8).reshape(67, 67, 32),
                        shredder_parity=np.array(shredder_p, np.uint32), cases=np.array(asserted, np.uint32))
    size = os.path.getsize(out)
    print(out, size, "bytes,", asserted, "cases asserted, none failed")
    assert size <= SIZE_LIMIT, size


if __name__ == "__main__":
    main(sys.argv[1])
