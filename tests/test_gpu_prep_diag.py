"""What the hash, scalar and decode phases write into the work arrays dsm
reads -- k, sflag, hs, hflag, fix_list, pts, pflag, perm -- in every form:
the product's own kernels launched as those phases alone on host inputs
(Engine.diag_prep), every array read back and compared with the
plain-integer model (tests/prep_model.py; tests/test_prep_model.py pins the
model and the inputs on the CPU first).  Exact.

A whole verify shows one code per signature, which hides most of this: the
x of a non-canonical y, s' = 0 under d < 0, a k left over from the previous
chunk by a bad perm, the scalars stored beside S >= L when k has no pair.
Every temporary goes in filled with 0x55 bytes, so a row no kernel wrote --
one it should have, or one at an index >= n -- shows as the pattern.

Every launch is a window of one of two sets of 4200 signatures (hashed
messages, or digests k + t L): each size with cap = n and with cap = n + 3."""
import ctypes
import time

import numpy as np
import pytest

import dsm_model as dm
import prep_model as pm

pytestmark = pytest.mark.gpu

MAX_CHUNK = 8192
PAT8, PAT32 = 0x55, 0x55555555
KIND = {"wide": "wide", "fused1": "fused", "fused2": "fused", "r16": "r16", "r16_decode": "r16", "r16_full": "r16"}
ROWS = ("k", "sflag", "hflag", "pflag", "pts", "hs", "perm", "out", "fix_list")


@pytest.fixture(scope="module")
def engines():
    from firedancer_amd import ed25519
    made = {}

    def get(codes="avx512", half="extended", dsm="r16", close=False):
        key = (codes, half, dsm)
        if close:   # an engine one test alone uses
            return made.pop(key).close()
        if key not in made:
            made[key] = ed25519.Engine(0, max_chunk=MAX_CHUNK, dsm=dsm, compact=True, codes=codes, half=half)
        return made[key]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def lib():
    from firedancer_amd import ed25519
    return ed25519.library()


def launch(eng, form, inp, cap=None):
    return eng.diag_prep(pm.FORMS[form], inp["sigs"], inp["pubs"], inp["msgs"], inp["msg_off"], inp["msg_sz"],
                         inp["digests"], cap=cap)


def launches(eng, form, mode):
    """(inputs, model, arrays, n, cap) of every launch of a form"""
    pool_inp, pool_model = pm.pool(mode)
    nmax = eng.diag_prep_nmax(pm.FORMS[form])
    assert nmax >= 65
    for n, cap, start in pm.windows(KIND[form], nmax):
        inp, idx = pm.window(pool_inp, start, n)
        yield inp, pool_model.take(idx), launch(eng, form, inp, cap), n, cap


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), (what, len(bad), [(tuple(int(v) for v in b), int(got[tuple(b)]), int(want[tuple(b)])) for b in bad[:4]])


def is_pattern(arr, what):
    arr = np.ascontiguousarray(arr)
    bad = np.argwhere(arr.view(np.uint8) != PAT8)
    assert not len(bad), (what, "written", len(bad), bad[:4].tolist())


def check_past_n(a, n, what):
    """columns n .. cap of every array: never written"""
    for f in ROWS:
        is_pattern(a[f][..., n:], (what, f, "columns >= n"))


def check_hash(a, m, n, what):
    same(a["k"][:, :n], m.k, (what, "k"))
    same(a["sflag"][:n], m.sflag, (what, "sflag"))


def check_scalars(a, m, n, dbits, wide, what):
    found, dneg, hs = m.scalars(dbits)
    hflag, sf = a["hflag"][:n], m.sflag.astype(bool)
    assert not (hflag & ~np.uint8(3)).any(), (what, "hflag outside its bits")
    full = (hflag & pm.HF_FULL) != 0
    # a pair: never the full-length form, the sign, c and |d|; s' too under S < L
    assert not full[found].any(), (what, "FULL beside a pair", np.nonzero(full & found)[0][:4].tolist())
    same((hflag & pm.HF_DNEG)[found], dneg[found], (what, "d < 0"))
    same(a["hs"][:10, :n][:, found], hs[:10][:, found], (what, "c, |d|"))
    same(a["hs"][10:, :n][:, found & sf], hs[10:][:, found & sf], (what, "s_lo, s_hi"))
    # no pair: the full-length form exactly where the equation is reached
    same(full[~found], sf[~found], (what, "FULL without a pair"))
    if wide:
        assert a["fix_cnt"] == int(full.sum()) and a["work_ctr"] == 0, (what, a["fix_cnt"], int(full.sum()), a["work_ctr"])
        same(np.sort(a["fix_list"][:a["fix_cnt"]]), np.nonzero(full)[0], (what, "fix_list"))
        is_pattern(a["fix_list"][a["fix_cnt"]:], (what, "fix_list past fix_cnt"))
    else:   # the scan after dsm finds them by hflag
        assert a["fix_cnt"] == PAT32 and a["work_ctr"] == PAT32, (what, "fix words written")
        is_pattern(a["fix_list"], (what, "fix_list"))
    return int(full.sum()), int((~found).sum())


def check_points(a, m, n, cap, avx, what):
    pf, y, x = m.points(avx)
    same(a["pflag"][:, :n], pf, (what, "pflag"))
    pts = a["pts"].reshape(2, 20, cap)[:, :, :n]
    same(pts[:, 10:], y, (what, "y limbs"))
    ok = (pf & pm.PF_FAIL) == 0
    for which in (0, 1):
        got = pm.limbs_value(pts[which, :10])
        bad = np.nonzero(ok[which] & (got != x[which]))[0]
        assert not len(bad), (what, "x", "AR"[which], len(bad), [m.enc[i][which].hex() for i in bad[:4]])
    # tight by diag_limbs_ok's bound, failed decodes included
    unit = np.array([1 << 25 if l % 2 == 0 else 1 << 24 for l in range(10)], np.int64)[None, :, None]
    assert (np.abs(pts[:, :10].astype(np.int64)) <= unit + unit // 100).all(), (what, "x limbs not tight")
    return int(ok.sum())


def check_perm(a, inp, n, sorted_, what):
    if not sorted_:
        is_pattern(a["perm"], (what, "perm"))
        return
    perm = a["perm"][:n]
    same(np.sort(perm), np.arange(n), (what, "perm is a permutation"))
    key = np.array([pm.sort_bucket(int(s)) for s in inp["msg_sz"][perm]])
    assert (np.diff(key) <= 0).all(), (what, "hash order", key[:16].tolist())


def contract(lib, eng, a, inp, n, cap, dsm_form):
    """diag_dsm_check on the arrays repacked to stride n"""
    pts = np.ascontiguousarray(a["pts"].reshape(40, cap)[:, :n])
    args = [np.ascontiguousarray(a["sflag"][:n]), np.ascontiguousarray(a["hflag"][:n]),
            np.ascontiguousarray(a["pflag"][:, :n]), pts, np.ascontiguousarray(a["hs"][:, :n]),
            np.ascontiguousarray(a["k"][:, :n]), np.ascontiguousarray(inp["sigs"])]
    dbits = lib.fd_ed25519_hip_private_half_dbits(ctypes.c_void_p(eng._h))
    return lib.fd_ed25519_hip_private_diag_dsm_check(dsm_form, n, n, dbits, *[ctypes.c_void_p(x.ctypes.data) for x in args])


HASHING = ("wide", "fused1", "fused2", "r16", "r16_full")


@pytest.mark.parametrize("half", ["extended", "strict"])
@pytest.mark.parametrize("mode", ["hashed", "digests"])
@pytest.mark.parametrize("form", HASHING)
def test_k_sflag_and_scalars(engines, form, mode, half):
    """k and sflag of every item; c, |d|, the sign and the split s' where the
    model finds a pair; FULL exactly for the items without one under S < L;
    the fix words; perm; nothing at an index >= n"""
    eng, dbits = engines(half=half), 131 if half == "strict" else 151
    t, n_full, n_nopair, items = time.perf_counter(), 0, 0, 0
    for inp, m, a, n, cap in launches(eng, form, mode):
        what = (form, mode, half, n, cap)
        check_hash(a, m, n, what)
        f, q = check_scalars(a, m, n, dbits, form == "wide", what)
        n_full, n_nopair, items = n_full + f, n_nopair + q, items + n
        check_perm(a, inp, n, form == "wide" and mode == "hashed", what)
        check_past_n(a, n, what)
        if form != "r16_full":
            is_pattern(a["out"], (what, "out"))
        else:   # the full-length items' codes (no equation holds on these inputs), nothing else
            full = (a["hflag"][:n] & pm.HF_FULL) != 0
            same(a["out"][:n][full], expected_codes(m, False)[full], (what, "codes of the full-length items"))
            is_pattern(a["out"][:n][~full], (what, "out of the half-size items"))
    print(f"{form}/{mode}/{half}: {items} items, {n_nopair} without a pair, {n_full} FULL, {time.perf_counter() - t:.2f} s")
    if mode == "digests":
        assert 0 < n_full < n_nopair   # both arms of the sflag override


PRODUCERS = ("wide", "fused1", "fused2", "r16", "r16_decode", "r16_full")   # decode_kernel, prep_kernel's waves 1-2, decode16_wave


@pytest.mark.parametrize("codes", ["avx512", "portable"])
@pytest.mark.parametrize("form", PRODUCERS)
def test_decoded_points(engines, form, codes):
    """pflag of both points, y as fe_frombytes splits it, x mod p wherever the
    decode did not fail, every x limb tight; the decode blocks alone leave
    the scalar side untouched"""
    eng, t, good = engines(codes=codes), time.perf_counter(), 0
    for inp, m, a, n, cap in launches(eng, form, "hashed"):
        what = (form, codes, n, cap)
        good += check_points(a, m, n, cap, codes == "avx512", what)
        check_past_n(a, n, what)
        if form == "r16_decode":
            for f in ("k", "sflag", "hs", "hflag", "out", "perm"):
                is_pattern(a[f], (what, f, "written by the decode blocks"))
            assert a["fix_cnt"] == PAT32 and a["work_ctr"] == PAT32
    print(f"{form}/{codes}: {good} points decoded, {time.perf_counter() - t:.2f} s")
    assert good >= 100


@pytest.mark.parametrize("half", ["extended", "strict"])
@pytest.mark.parametrize("form", ["wide", "fused1", "fused2", "r16"])
def test_arrays_meet_the_dsm_contract(engines, lib, form, half):
    """what prep hands over is what the dsm kernels are documented to take
    (fd_ed25519_hip_private_diag_dsm_check), for the form that consumes it --
    the digests' k without a pair beside S >= L included"""
    eng = engines(half=half)
    refused = []
    for mode in ("hashed", "digests"):
        for inp, m, a, n, cap in launches(eng, form, mode):
            for dsm_form in pm.DSM_FORM[form]:
                if contract(lib, eng, a, inp, n, cap, dsm_form):
                    found = m.scalars(131 if half == "strict" else 151)[0]
                    bits = [(int(sum(int(a["hs"][w, j]) << (32 * w) for w in range(5))).bit_length(),
                             int(sum(int(a["hs"][5 + w, j]) << (32 * w) for w in range(5))).bit_length(),
                             int(m.sflag[j]), int(a["hflag"][j])) for j in range(n)
                            if not found[j] and not a["hflag"][j] & pm.HF_FULL]   # (bits of c, of |d|, sflag, hflag)
                    refused.append((mode, n, cap, dsm_form, bits[:6]))
    assert not refused, (len(refused), refused[:4])


def dsm_arrays(a, inp):
    return dict(sflag=a["sflag"], hflag=a["hflag"], pflag=a["pflag"], pts=a["pts"], hs=a["hs"], k=a["k"], S=inp["sigs"])


@pytest.mark.parametrize("form", ["wide", "fused1", "fused2", "r16"])
def test_the_halves_meet(engines, adversarial, halfsize, form):
    """diag_prep's arrays of the fixtures straight into diag_dsm in the same
    form: the golden codes"""
    eng = engines()
    for name, d, cnt in (("adversarial", adversarial, 257), ("halfsize", halfsize, None)):
        inp = pm.from_fixture(d, cnt)
        a = launch(eng, form, inp)
        x = dsm_arrays(a, inp)
        got = eng.diag_dsm(pm.DSM_FORM[form][0], x["sflag"], x["hflag"], x["pflag"], x["pts"], x["hs"], x["k"], x["S"])
        same(got, d["codes_avx512"][:inp["n"]], (form, name))


def test_full_length_items_in_prep16(engines, halfsize):
    """R16_FULL on halfsize.npz under the strict bound: prep16's hash waves
    leave the golden code for exactly the full-length items"""
    eng = engines(half="strict")
    inp = pm.from_fixture(halfsize)
    a = launch(eng, "r16_full", inp)
    full = (a["hflag"] & pm.HF_FULL) != 0
    m = pm.Model(inp)
    same(full, ~m.scalars(131)[0] & m.sflag.astype(bool), "FULL")
    assert full.sum() >= 50 and (~full).sum() >= 20
    same(a["out"][full], halfsize["codes_avx512"][full], "codes of the full-length items")
    is_pattern(a["out"][~full], "out of the half-size items")


def nopair_window(count=129, others=64):
    """digests whose k has no 151-bit pair (S >= L and S < L among them), then a few of the rest"""
    inp, m = pm.pool("digests")
    found = m.scalars(151)[0]
    idx = np.concatenate([np.nonzero(~found)[0][:count], np.nonzero(found)[0][:others]])
    win = dict(inp, n=len(idx), sigs=np.ascontiguousarray(inp["sigs"][idx]), pubs=np.ascontiguousarray(inp["pubs"][idx]),
               digests=np.ascontiguousarray(inp["digests"][idx]))
    return win, m.take(idx)


def expected_codes(m, portable):
    """no equation holds on these inputs: precheck's order, else ERR_MSG"""
    pf = m.points(not portable)[0]
    codes = [dm.precheck(int(m.sflag[i]), int(pf[0, i]), int(pf[1, i]), portable) for i in range(m.n)]
    return np.array([dm.ERR_MSG if c is None else c for c in codes], np.int8)


@pytest.mark.parametrize("codes", ["avx512", "portable"])
@pytest.mark.parametrize("dsm", ["wide", "quad", "oct", "r16", "auto"])
def test_regression_no_pair_through_a_whole_verify(engines, dsm, codes):
    """verify_digests_host on k without a 151-bit pair, S >= L and S < L, in
    every dsm form: scalar_one stores c = 0, |d| = 1 beside S >= L, so the
    half-size loops never see a scalar past their tables"""
    win, m = nopair_window()
    assert ((m.sflag == 0) & ~m.scalars(151)[0]).sum() >= 5 and ((m.sflag == 1) & ~m.scalars(151)[0]).sum() >= 5
    want = expected_codes(m, codes == "portable")
    assert {dm.ERR_SIG, dm.ERR_MSG} <= set(want.tolist())
    eng = engines(codes=codes, dsm=dsm)
    for n in (m.n, 64, 5, 1):
        same(eng.verify_digests_host(win["digests"][:n], win["sigs"][:n], win["pubs"][:n]), want[:n], (dsm, codes, n))
    engines(codes=codes, dsm=dsm, close=True)


@pytest.mark.parametrize("form", ["wide", "fused1", "fused2", "r16"])
def test_regression_no_pair_through_both_diagnostics(engines, form):
    """the same through diag_prep -> diag_dsm: c = 0, |d| = 1, d >= 0 and s' =
    S mod L stored beside S >= L, and the codes"""
    win, m = nopair_window()
    eng = engines()
    a = launch(eng, form, win)
    found = m.scalars(151)[0]
    gone = ~found & (m.sflag == 0)
    assert gone.sum() >= 5
    sp = [S % pm.L for S in m.Ss]
    rows = np.array([pm.words(0, 5) + pm.words(1, 5) + pm.words(s % 2**144, 5) + pm.words(s >> 144, 4) for s in sp],
                    np.uint32).T
    same(a["hs"][:, gone], rows[:, gone], (form, "scalars beside S >= L"))
    same(a["hflag"][gone], np.zeros(int(gone.sum()), np.uint8), (form, "hflag beside S >= L"))
    x = dsm_arrays(a, win)
    got = eng.diag_dsm(pm.DSM_FORM[form][0], x["sflag"], x["hflag"], x["pflag"], x["pts"], x["hs"], x["k"], x["S"])
    same(got, expected_codes(m, False), form)
