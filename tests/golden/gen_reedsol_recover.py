"""Makes tests/golden/reedsol_recover.npz: what the reference's own decoder
returns and recovers for a list of erasure patterns over reedsol.npz's seeded
data and the reference's own parity of it.

    python tests/golden/gen_reedsol_recover.py <reference>/src

gen_reedsol_recover_ref.c, this project's own harness, is compiled in a
temporary directory against the reference's sources exactly as gen_reedsol.py
compiles its harness, and run with the reference's root as its working
directory.  It decodes with fd_reedsol_recover_init / _add_rcvd_shred /
_add_erased_shred / _fini at shred size 32.

A case is (d, p, erased mask, corrupted slot or none): the codeword is
reedsol.npz's data[:d] and parity[d-1][:p]; an erased slot goes in as 0xA5
bytes; a corrupted slot is a received one with bit 0 of byte corrupt_at
flipped.

  d[n], p[n]       the split of case k
  erased[n][134]   its mask (zero beyond d + p)
  corrupt[n]       its corrupted slot, -1 for none;  corrupt_at[n] the byte
  kind[n]          index into KINDS, what the case is there for
  ret[n]           what fd_reedsol_recover_fini returned (0, -1 corrupt, -2
                   partial)
  rec_at[n+1], recovered[.][32]
                   for a case with ret 0 the slots the reference wrote, in
                   set order: recovered[rec_at[k]:rec_at[k+1]]
  cases            n, how many cases the generator asserted

The cases: every d in 1..67 with the shredder's p, and 1+1, 1+67, 67+1,
67+67, each with a seeded mask of exactly p erasures, with all data erased
(where p >= d), with all parity erased, with nothing erased, with d - 1
received (partial), with d + 1 and with all received and one byte of the last
received slot flipped (corrupt), and with the same flip in the first basis
slot (corrupt: something beyond the basis is received); and masks chosen for
the number of erased and of compared targets (exactly 32, more than 32, both
in one set).

What the generator itself holds to on every case: the reference's return
value and, where it is 0, every slot after the call are the test-side
model's (tests/recover_model.py: the Lagrange formula over the first d
received slots), and a recovered slot is the codeword's.  Nothing here is run
by a test."""
import os
import random
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

SEED = 197
SZ = 32
SIZE_LIMIT = 1 << 20    # of a committed file
KINDS = ("p_erased", "all_data_erased", "all_parity_erased", "nothing_erased", "partial", "late_flip_d_plus_1",
         "late_flip_all_received", "basis_flip_d_plus_1", "basis_flip_all_received", "target_counts")
EXTREMES = ((1, 1), (1, 67), (67, 1), (67, 67))


def mask(rng, cnt, n_erased):
    m = [0] * cnt
    for j in rng.sample(range(cnt), n_erased):
        m[j] = 1
    return m


def make_cases(shredder_p):
    """[(kind, d, p, mask, corrupted slot or -1, byte)]"""
    rng = random.Random(SEED)
    pairs = [(d, int(shredder_p[d])) for d in range(1, 68)] + list(EXTREMES)
    out = []
    for d, p in pairs:
        cnt = d + p
        out.append(("p_erased", d, p, mask(rng, cnt, p), -1, 0))
        if p >= d:
            out.append(("all_data_erased", d, p, [1] * d + [0] * p, -1, 0))
        out.append(("all_parity_erased", d, p, [0] * d + [1] * p, -1, 0))
        out.append(("nothing_erased", d, p, [0] * cnt, -1, 0))
        out.append(("partial", d, p, mask(rng, cnt, p + 1), -1, 0))
        for n_erased, late, basis in ((p - 1, "late_flip_d_plus_1", "basis_flip_d_plus_1"),
                                      (0, "late_flip_all_received", "basis_flip_all_received")):
            m = mask(rng, cnt, n_erased)
            rcvd = [j for j in range(cnt) if not m[j]]
            assert len(rcvd) > d
            out.append((late, d, p, m, rcvd[-1], rng.randrange(SZ)))
            out.append((basis, d, p, m, rcvd[0], rng.randrange(SZ)))
    # the erased targets and the compared targets of a set: exactly 32, more than 32, both
    for d, p, n_erased in ((67, 67, 32), (67, 67, 35), (33, 33, 1), (64, 64, 32), (40, 67, 33), (2, 67, 34)):
        out.append(("target_counts", d, p, mask(rng, d + p, n_erased), -1, 0))
    return out


def run_reference(ref, blob):
    """the harness's output for the input blob"""
    from gen_packets import ref_defs
    from gen_reedsol import reference_sources
    root = os.path.dirname(os.path.abspath(ref))
    with tempfile.TemporaryDirectory() as tmp:
        exe, objs = os.path.join(tmp, "gen_reedsol_recover_ref"), []
        ref, jobs = os.path.abspath(ref), []
        for src in reference_sources(ref) + [os.path.join(HERE, "gen_reedsol_recover_ref.c")]:
            obj = os.path.join(tmp, os.path.basename(src)[:-2] + ".o")
            # -O1 after REF_DEFS' -O3: the unrolled transforms are long
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


def codeword(g, d, p):
    return [g["data"][i].tobytes() for i in range(d)] + [g["parity"][d - 1][j].tobytes() for j in range(p)]


def case_input(g, d, p, m, bad, at):
    """the slots as they go in"""
    slots = [b"\xA5" * SZ if e else s for s, e in zip(codeword(g, d, p), m)]
    if bad >= 0:
        assert not m[bad]
        s = bytearray(slots[bad])
        s[at] ^= 1
        slots[bad] = bytes(s)
    return slots


def main(ref):
    import recover_model as model
    g = np.load(os.path.join(HERE, "reedsol.npz"))
    cases = make_cases(g["shredder_parity"])
    blob = [struct.pack("<I", len(cases))]
    for _, d, p, m, bad, at in cases:
        blob.append(struct.pack("<III", d, p, SZ) + bytes(m) + b"".join(case_input(g, d, p, m, bad, at)))
    raw, pos = run_reference(ref, b"".join(blob)), 0
    ret, rec_at, recovered, failed, seen = [], [0], [], [], {}
    for k, (kind, d, p, m, bad, at) in enumerate(cases):
        r, = struct.unpack_from("<i", raw, pos)
        pos += 4
        after = [raw[pos + SZ * j:pos + SZ * (j + 1)] for j in range(d + p)]
        pos += SZ * (d + p)
        before = case_input(g, d, p, m, bad, at)
        want_code, want = model.recover(before, m, d)
        ok = model.REF_CODES[r] == want_code
        if r == 0:
            word = codeword(g, d, p)
            ok = ok and after == want and all(after[j] == word[j] for j in range(d + p) if m[j])
            recovered += [after[j] for j in range(d + p) if m[j]]
        if not ok:
            failed.append((k, kind, d, p))
        ret.append(r)
        rec_at.append(len(recovered))
        seen.setdefault(kind, set()).add(r)
    assert pos == len(raw)
    assert not failed, failed
    assert seen == {"p_erased": {0}, "all_data_erased": {0}, "all_parity_erased": {0}, "nothing_erased": {0}, "partial": {-2},
                    "late_flip_d_plus_1": {-1}, "late_flip_all_received": {-1}, "basis_flip_d_plus_1": {-1},
                    "basis_flip_all_received": {-1}, "target_counts": {0}}, seen
    n = len(cases)
    erased = np.zeros((n, 134), np.uint8)
    for k, c in enumerate(cases):
        erased[k, :len(c[3])] = c[3]
    out = os.path.join(HERE, "reedsol_recover.npz")
    np.savez_compressed(out, d=np.array([c[1] for c in cases], np.uint8), p=np.array([c[2] for c in cases], np.uint8),
                        erased=erased, corrupt=np.array([c[4] for c in cases], np.int16),
                        corrupt_at=np.array([c[5] for c in cases], np.uint8),
                        kind=np.array([KINDS.index(c[0]) for c in cases], np.uint8), ret=np.array(ret, np.int8),
                        rec_at=np.array(rec_at, np.uint32),
                        recovered=np.frombuffer(b"".join(recovered), np.uint8).reshape(-1, SZ), cases=np.array(n, np.uint32))
    size = os.path.getsize(out)
    print(out, size, "bytes,", n, "cases asserted, none failed")
    assert size <= SIZE_LIMIT, size


if __name__ == "__main__":
    main(sys.argv[1])
