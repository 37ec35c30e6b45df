"""The workspace layout of the proof-of-history check (front_work_poh,
firedancer_amd/csrc/fd_front_work.h): tests/poh_work_main.c under ASan and
UBSan checks, for n in 0, 1, 2, 63, 64, 65, 257 and 16384 and n_sig in 0, 1, n,
20 n + 1, 127 n and 300, that the rows of hashes are 16-byte aligned, that
each array lies where the public header says and that the layout ends inside
FD_ED25519_HIP_POH_WORK_BYTES.  A program of its own: nothing is loaded into
this interpreter."""
import subprocess

import san_build


def test_layout_fits_the_public_macro(tmp_path):
    exe = san_build.build("poh_work_main.c", tmp_path / "poh_work")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout == "%d layouts\n" % (8 * 6)
