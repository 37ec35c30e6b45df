"""A pass of the FEC-set host wrappers (firedancer_amd/csrc/fd_fec_pass.h):
tests/fec_pass_main.c under ASan and UBSan cuts and stages three batches -- a
mix of sets of 1 to 134 shreds with empty, oversized, backward and
out-of-range ranges among them, 16,385 empty ranges ahead of one good set, and
130 sets of 134 whose shred total crosses 16,384 inside a set -- in the
seal's mode without and with keys, the parity's and the recovery's, into an
item staging and an in block of exactly the sizes the header states, and
checks every pass: that it advances and keeps both bounds, that the passes
tile the sets, the in block's alignment, overlap and size, and where and how
every shred of 0 to 4,000 bytes is staged.  A program of its own: nothing is
loaded into this interpreter."""
import subprocess

import san_build


def test_passes_keep_their_bounds_and_buffers(tmp_path):
    exe = san_build.build("fec_pass_main.c", tmp_path / "fec_pass")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    # a variant: the mix in one pass (9,045 + 134 shreds), the other two batches in two each (3; 122 + 8 sets of 134)
    assert r.stdout == "%d passes, %d shreds\n" % (4 * 5, 4 * (9045 + 134 + 3 + 134 * 130))
