"""The workspace layout of the FEC seal (front_work_fec,
firedancer_amd/csrc/fd_front_work.h): tests/fec_work_main.c under ASan and
UBSan checks, for n_set in 0..67, 255, 256, 257 and 16384 and n in 0, 1, n_set,
64 n_set + 1 and SET_MAX n_set, that every array is aligned, that no two
overlap, that each lies where the public header says and that the layout ends
inside FD_ED25519_HIP_FEC_WORK_BYTES.  A program of its own: nothing is loaded
into this interpreter."""
import subprocess

import san_build


def test_layout_fits_the_public_macro(tmp_path):
    exe = san_build.build("fec_work_main.c", tmp_path / "fec_work")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout == "%d layouts\n" % (72 * 5)
