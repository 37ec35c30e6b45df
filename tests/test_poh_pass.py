"""A pass of fd_ed25519_hip_poh_host (firedancer_amd/csrc/fd_poh_pass.h):
tests/poh_pass_main.c under ASan and UBSan judges, orders, cuts, stages and
scatters seven calls -- 48 microblocks whose k ties, with rejected and
unsupported ones among them and every third in state in `extra` (with `extra`,
without it and without out_hash), 16,385 microblocks without signatures, and
microblocks of 2^18 - 1, 2^18 and 2^18 + 1 signatures among small ones -- into
an order, an item staging and in and out blocks of exactly the sizes the
header states, and checks every pass: that it advances, keeps both bounds and
is greedy, the in block's alignment, overlap and size, every staged byte, and
that codes and states come back at the caller's indices.  A program of its
own: nothing is loaded into this interpreter."""
import subprocess

import san_build

CHUNK, SIGS = 16384, 1 << 18


def passes(mbs):
    """mbs: (k, signatures) of the microblocks that travel, in the caller's
    order -> (passes, microblocks, signatures) of the cut over them by
    descending k, then index"""
    order = sorted(range(len(mbs)), key=lambda i: (-mbs[i][0], i))
    n, m, ns = 0, 0, 0
    for i in order:
        if not n or m == CHUNK or ns + mbs[i][1] > SIGS:
            n, m, ns = n + 1, 0, 0
        m, ns = m + 1, ns + mbs[i][1]
    return n, len(mbs), sum(s for _, s in mbs)


def order_call(with_extra):
    """tests/poh_pass_main.c's table"""
    mbs = []
    for i in range(48):
        sigs = (0, 1, 3, 0, 2)[i % 5]
        hash_cnt = 1000 if i % 7 == 2 else (7, 3, 7, 0, 12, 3)[i % 6]
        k = (hash_cnt - 1 if hash_cnt else 0) if sigs else hash_cnt
        rejected = i % 11 == 4 or (i % 13 == 6 and sigs) or (i % 3 == 0 and not with_extra)
        if not rejected:
            mbs.append((k if k <= 100 else 0, sigs))
    return mbs


CALLS = [
    order_call(True), order_call(False), order_call(True),
    [(i % 3, 0) for i in range(16385)],
    [(8, SIGS - 1), (7, 1), (6, 1)],
    [(8, 1), (7, SIGS), (6, 1)],
    [(8, 1), (7, SIGS + 1), (6, 1)],
]


def test_passes_keep_their_bounds_and_buffers(tmp_path):
    assert [passes(c)[0] for c in CALLS] == [1, 1, 1, 2, 2, 3, 3]
    assert len(CALLS[0]) < 48 and len(CALLS[1]) < len(CALLS[0])
    exe = san_build.build("poh_pass_main.c", tmp_path / "poh_pass")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    want = [sum(passes(c)[i] for c in CALLS) for i in range(3)]
    assert r.stdout == "%d passes, %d microblocks, %d signatures\n" % tuple(want)
