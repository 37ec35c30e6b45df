"""The pinned block of a drop-in launch (firedancer_amd/csrc/fd_dropin_block.h):
tests/dropin_block_main.c under ASan and UBSan prints the layout for requests
n in 1, 2, 17, signatures a request in 1, 2, 16, message bytes in 0, 1, 15,
16, 17, 65536, 65537, nsig_h in 0, 1, all, and host scalars off, or on with a
host-scalar block of 0 bytes, of the host-decoded size and of the
device-decoded size at the drop-in engines' stride.  Every offset is held to
the formulas dropin_run had before the layout got a header (restated below in
Python integers), and the block to its documented shape:
    [off | sz | tfirst | tcnt | sigs | pubs | dig | msgs], 16 spare bytes,
    [codes | txn codes], then the host-scalar block
every array starting on a multiple of 16 (the per-request codes are the
bytes right behind the per-signature ones, one region: the formulas put them
at o_out + nsig), no two overlapping, need past the last byte.  A program of
its own: nothing is loaded into this interpreter."""
import os
import re
import subprocess

import san_build

HDR = os.path.join(san_build.REPO, "firedancer_amd", "csrc", "fd_ed25519_hip_internal.h")
DROPIN_CHUNK = 16384
FIELDS = ("o_off", "o_sz", "o_tf", "o_tc", "o_sig", "o_pub", "o_dig", "o_msg", "in_sz", "o_out", "o_tout", "o_hsb",
          "need")


def a16(x):
    return (x + 15) & ~15


def hs_bytes(stride, decode):
    """fd_ed25519_hip_private_hs_bytes, from the header's layout macros"""
    o_hs = 2 * a16(stride)
    if not decode:
        return o_hs + 19 * 4 * stride
    o_pflag = o_hs + 24 * 4 * stride + 8 * 40 * 4 * stride
    return a16(o_pflag + 2 * stride) + 16


def parent(n, nsig, nsig_h, nbytes, hsmode, hsb):
    """dropin_run's arithmetic as it stood in fd_ed25519_hip_engine.c"""
    ndig = nsig if hsmode else nsig_h
    o = {"o_off": 0}
    o["o_sz"] = a16(o["o_off"] + 8 * nsig)
    o["o_tf"] = a16(o["o_sz"] + 4 * nsig)
    o["o_tc"] = a16(o["o_tf"] + 4 * n)
    o["o_sig"] = a16(o["o_tc"] + 4 * n)
    o["o_pub"] = a16(o["o_sig"] + 64 * nsig)
    o["o_dig"] = a16(o["o_pub"] + 32 * nsig)
    o["o_msg"] = a16(o["o_dig"] + 64 * ndig)
    o["in_sz"] = o["o_msg"] + (0 if hsmode else nbytes)
    o["o_out"] = a16(o["in_sz"] + 16)
    o["o_tout"] = o["o_out"] + nsig
    o["need"] = o["o_tout"] + n + 16
    o["o_hsb"] = a16(o["need"])
    if hsmode:
        o["need"] = o["o_hsb"] + hsb
    return o


def test_block_layout_has_not_moved_and_keeps_its_shape(tmp_path):
    exe = san_build.build("dropin_block_main.c", tmp_path / "dropin_block")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    stride = int(re.search(r"#define\s+FD_ED25519_HS_STRIDE\s+(\d+)UL", open(HDR).read()).group(1))
    sizes = [hs_bytes(stride, True), hs_bytes(DROPIN_CHUNK, False)]
    assert [int(x) for x in lines[0].split()] == sizes
    seen = set()
    for line in lines[1:]:
        v = [int(x) for x in line.split()]
        n, nsig, nsig_h, nbytes, hsmode, hsb = v[:6]
        got = dict(zip(FIELDS, v[6:]))
        assert len(v) == 6 + len(FIELDS)
        assert got == parent(n, nsig, nsig_h, nbytes, hsmode, hsb), line
        seen.add(tuple(v[:6]))
        ndig = nsig if hsmode else nsig_h
        regions = [("o_off", 8 * nsig), ("o_sz", 4 * nsig), ("o_tf", 4 * n), ("o_tc", 4 * n), ("o_sig", 64 * nsig),
                   ("o_pub", 32 * nsig), ("o_dig", 64 * ndig), ("o_msg", 0 if hsmode else nbytes)]
        end = 0
        for name, size in regions:                       # the input, in the documented order
            assert got[name] % 16 == 0 and got[name] >= end, (name, line)
            end = got[name] + size
        assert got["in_sz"] == end, line
        assert got["o_out"] % 16 == 0 and got["o_out"] >= end + 16, line   # 16 spare bytes for the SHA-512 loader
        assert got["o_tout"] == got["o_out"] + nsig, line                 # [codes | txn codes]
        end = got["o_tout"] + n
        assert got["o_hsb"] % 16 == 0 and got["o_hsb"] >= end, line
        if hsmode:
            end = got["o_hsb"] + hsb
        assert got["need"] >= end, line
    want = {(n, n * per, h, b, s > 0, (0, 0, sizes[0], sizes[1])[s])
            for n in (1, 2, 17) for per in (1, 2, 16) for b in (0, 1, 15, 16, 17, 65536, 65537)
            for h in (0, 1, n * per) for s in range(4)}
    assert seen == want and len(lines) == 1 + 3 * 3 * 7 * 3 * 4
