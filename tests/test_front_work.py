"""The workspace layouts of the precompile, shred and packet fronts
(firedancer_amd/csrc/fd_front_work.h): tests/front_work_main.c under ASan and
UBSan checks, for n and ntxn in 0..67, 255, 256, 257 and 16384 (n_ent in 0,
1, ntxn, 8 ntxn; pkt_bytes in 0..64 and 1232 n), that every array is aligned,
that no two overlap, that the layout ends inside the public *_WORK_BYTES
macro and that every offset is the one the engine used before.  A program of
its own: nothing is loaded into this interpreter."""
import subprocess

import san_build


def test_layouts_fit_the_public_macros_and_have_not_moved(tmp_path):
    exe = san_build.build("front_work_main.c", tmp_path / "front_work")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout == "%d layouts\n" % (72 * (4 + 1 + 65 + 1))
