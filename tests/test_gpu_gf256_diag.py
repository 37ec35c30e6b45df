"""GPU: the GF(2^8) product of the Reed-Solomon kernels (fd_reedsol_dev.h:
three v_perm_b32 lookups into a coefficient's 20 table bytes) and the recover
kernel's coefficient build (log_d, log_n and fd_reedsol_core_coef from the
log / exp tables in LDS), each directly, through libfd_ed25519_diag.so's
fd_ed25519_diag_reedsol (firedancer_amd/csrc/diag/fd_ed25519_diag_reedsol.hip)
on the table block the product library gives an engine.  Expected values are
reedsol_model.mul's and recover_model.lagrange's."""
import ctypes

import numpy as np
import pytest

import diag_util as du
import fec_wave_util as wave

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
COEF_IN, COEF_ROWS, STRIDE = 20, 134, 68


@pytest.fixture(scope="module")
def diag():
    d = du.Diag()
    d.lib.fd_ed25519_diag_reedsol.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulong]
    d.lib.fd_ed25519_diag_reedsol.restype = ctypes.c_int
    return d


@pytest.fixture(scope="module")
def tab():
    """the table block an engine uploads, from the product library"""
    from firedancer_amd import ed25519
    lib = ed25519.library()
    lib.fd_ed25519_hip_private_reedsol_tab_bytes.restype = ctypes.c_ulong
    lib.fd_ed25519_hip_private_reedsol_tables.argtypes = [ctypes.c_void_p]
    lib.fd_ed25519_hip_private_reedsol_tables.restype = None
    t = np.zeros(int(lib.fd_ed25519_hip_private_reedsol_tab_bytes()), np.uint8)
    assert len(t) == 161600
    lib.fd_ed25519_hip_private_reedsol_tables(t.ctypes.data)
    return t


def run(diag, tab, op, inp, out, n):
    rc = diag.lib.fd_ed25519_diag_reedsol(op, tab.ctypes.data, inp.ctypes.data, out.ctypes.data, n)
    assert rc == 0, f"fd_ed25519_diag_reedsol({op}) returned HIP error {rc}"


def test_every_product_in_every_byte_lane(diag, tab):
    """all 65,536 (c, v), v in each of the four byte lanes with three other bytes beside it, in one launch"""
    c, x, want = wave.product_rows()
    n = len(c)
    inp = np.ascontiguousarray(np.stack([c, x], axis=1), np.uint32)
    out = np.full(n + 64, FILL, np.uint32)
    run(diag, tab, 0, inp, out, n)
    bad = np.nonzero(out[:n] != want)[0]
    assert not len(bad), [(int(c[i]), hex(int(x[i])), hex(int(out[i])), hex(int(want[i]))) for i in bad[:8]]
    assert (out[n:] == FILL).all()


@pytest.mark.parametrize("n", [1, 255, 257])
def test_product_case_counts(diag, tab, n):
    """around the block of 256 lanes: the rows past n keep their fill"""
    c, x, want = wave.product_rows()
    pick = np.arange(n) * 251 % 65536
    inp = np.ascontiguousarray(np.stack([c[pick], x[pick]], axis=1), np.uint32)
    out = np.full(n + 64, FILL, np.uint32)
    run(diag, tab, 0, inp, out, n)
    assert (out[:n] == want[pick]).all() and (out[n:] == FILL).all()


def test_coefficients_of_chosen_bases(diag, tab):
    """50 bases of 1..67 slots within 134: every L[e][r] as a field element, every byte outside them untouched"""
    cases = wave.coef_cases()
    n = len(cases)
    inp = np.zeros((n, COEF_IN), np.uint32)
    want = np.full((n + 2, COEF_ROWS, STRIDE), FILL & 0xFF, np.uint8)
    for k, (basis, targets, coef) in enumerate(cases):
        inp[k, 0], inp[k, 1] = wave.COEF_CNT, len(basis)
        inp[k, 2:].view(np.uint8)[:len(basis)] = basis
        want[k, :len(targets), :len(basis)] = coef
    out = np.full((n + 2, COEF_ROWS * STRIDE // 4), FILL, np.uint32)
    run(diag, tab, 1, inp, out, n)
    got = out.view(np.uint8).reshape(n + 2, COEF_ROWS, STRIDE)
    bad = np.argwhere(got != want)
    assert not len(bad), [(int(k), len(cases[k][0]), int(r), int(i), int(got[k, r, i]), int(want[k, r, i])) for k, r, i in bad[:8]]


def test_argument_checks(diag, tab):
    inp, out = np.zeros((1, COEF_IN), np.uint32), np.zeros((1, COEF_ROWS * STRIDE // 4), np.uint32)
    call = diag.lib.fd_ed25519_diag_reedsol
    inp[0, 0] = 256                                                    # c above a byte
    assert call(0, tab.ctypes.data, inp.ctypes.data, out.ctypes.data, 1) == du.HIP_ERROR_INVALID_VALUE
    assert call(2, tab.ctypes.data, inp.ctypes.data, out.ctypes.data, 1) == du.HIP_ERROR_INVALID_VALUE
    for cnt, d, basis in ((135, 1, [0]), (134, 68, list(range(68))), (134, 0, []), (3, 3, [0, 1, 2]), (5, 2, [1, 1]),
                          (5, 2, [2, 1]), (5, 2, [0, 5])):
        inp[:] = 0
        inp[0, 0], inp[0, 1] = cnt, d
        inp[0, 2:].view(np.uint8)[:len(basis)] = basis
        assert call(1, tab.ctypes.data, inp.ctypes.data, out.ctypes.data, 1) == du.HIP_ERROR_INVALID_VALUE, (cnt, d)
    assert not out.any()
