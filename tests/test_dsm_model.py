"""The plain-integer model of the dsm loops (tests/dsm_model.py) and the
diagnostic's validation, without a GPU:

  * the model's curve arithmetic against diag_util's affine helpers, and the
    discrete-logarithm shortcut the crafted cases carry against the point
    evaluation;
  * the model against the reference's verdicts: every signature of the
    golden fixtures, its scalars from the host record (hsrec) -- k =
    SHA-512(R || A || M) mod L and the full-length form where there is no
    record -- and its points and flags from hsdec_n, must give the
    fixture's code, in both code flavours;
  * fd_ed25519_hip_private_diag_dsm_check refuses each out-of-contract
    class, at the bound and one past it;
  * the split rule restated in Python equals the product's hssplit on the
    crafted scalars."""
import ctypes
import random

import numpy as np
import pytest

import diag_util as du
import dsm_model as dm
from diag_util import L

INVAL = -22


@pytest.fixture(scope="module")
def lib():
    from firedancer_amd import ed25519
    lb = ed25519.library()
    lb.fd_ed25519_hip_private_hsrec.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_ulong,
                                                ctypes.c_int, ctypes.c_void_p]
    lb.fd_ed25519_hip_private_hsdec_n.argtypes = [ctypes.c_void_p, ctypes.c_ulong, ctypes.c_int, ctypes.c_void_p,
                                                  ctypes.c_void_p]
    lb.fd_ed25519_hip_private_hsdec_n.restype = None
    return lb


@pytest.fixture(scope="module")
def crafted():
    return dm.crafted_half_cases()


def test_extended_arithmetic_is_the_affine_helpers():
    rng = random.Random(1)
    pts = [du.random_point(rng) for _ in range(4)] + du.TORSION + [du.BASE]
    for a in pts:
        for b in pts:
            assert dm.xaffine(dm.xadd(dm.xpt(a), dm.xpt(b))) == du.ed_add(a, b)
        assert dm.xaffine(dm.xdbl(dm.xpt(a))) == du.ed_add(a, a)
    for k in (0, 1, 2, 8, L - 1, L, rng.getrandbits(253)):
        assert dm.xaffine(dm.xmul(k, dm.xpt(pts[0]))) == du.ed_mul(k, pts[0])
        assert dm.xaffine(dm.base_mul(k)) == du.ed_mul(k, du.BASE)
    k1, k2 = rng.getrandbits(131), rng.getrandbits(151)
    assert dm.xaffine(dm.xmul2(k1, dm.xpt(pts[0]), k2, dm.xpt(pts[1]))) == \
        du.ed_add(du.ed_mul(k1, pts[0]), du.ed_mul(k2, pts[1]))
    assert du.ed_mul(8, du.ORDER8) == du.IDENT and du.ed_mul(4, du.ORDER8) == du.ORDER2
    assert dm.dl_point(5, 3) == du.ed_add(du.ed_mul(5, du.BASE), du.ed_mul(3, du.ORDER8))


def test_crafted_cases_cover_the_classes(crafted):
    cases, kinds = crafted
    exp = [dm.case_expect(c) for c in cases]
    assert len(cases) >= 2000
    n_valid = sum(k == "valid" for k in kinds)
    assert n_valid >= 500 and all(e == dm.SUCCESS for e, k in zip(exp, kinds) if k == "valid")
    # the near misses that can never cancel
    for kind in ("sp", "tors"):
        sel = [e for e, k in zip(exp, kinds) if k == kind]
        assert len(sel) >= 100 and all(e == dm.ERR_MSG for e in sel), kind
    for kind in ("win", "sign", "rneg"):
        sel = [e for e, k in zip(exp, kinds) if k == kind]
        assert len(sel) >= 100 and sum(e == dm.ERR_MSG for e in sel) >= 0.9 * len(sel), kind
    # the operands the end-to-end suite never reaches
    assert any(c["c"] == 0 for c in cases) and any(c["dm"] == 2**151 - 1 for c in cases)
    assert any(c["c"] == dm.pat(8, 131) for c in cases) and any(c["dm"] < 16 and c["dm"] for c in cases)
    assert any(c["sp"] == 0xffffff << 24 for c in cases) and any(c["c"] & (2**66 - 1) == 2**66 - 1 for c in cases)
    assert {c["A"][1] for c in cases} == set(range(8)) and {c["R"][1] for c in cases} == set(range(8))
    # order 2 alone in the sum: X == 0, so only Y == Z tells
    assert any((c["c"] * c["A"][1] + (-c["dm"] if c["dneg"] else c["dm"]) * c["R"][1]) % 8 == 4 and
               (c["sp"] - c["c"] * c["A"][0] - (-c["dm"] if c["dneg"] else c["dm"]) * c["R"][0]) % L == 0 for c in cases)


def test_discrete_log_shortcut_is_the_point_model(crafted):
    cases, _ = crafted
    full = dm.crafted_full_cases()
    sample = cases[::9] + full[::5]
    seen = set()
    for cs in sample:
        A, R = dm.dl_point(*cs["A"]), dm.dl_point(*cs["R"])
        assert du.on_curve(A) and du.on_curve(R)
        got = dm.model_code(cs, False, A, R)
        assert got == dm.case_expect(cs), cs
        seen.add((cs["full"], got))
    assert seen >= {(False, 0), (False, -3), (True, 0), (True, -3)}


@pytest.mark.parametrize("waves", [4, 8])
def test_split_model_and_rule(lib, crafted, waves):
    """the Python split rule equals hssplit on the crafted scalars, and the
    split sum over the supplied (doubled, rescaled) points is the half-size
    sum"""
    cases, _ = crafted
    for cs in cases:
        assert list(dm.hssplit(lib, dm.record(cs), waves)[:, 0]) == dm.split_rows(waves, cs["c"], cs["dm"], cs["sp"])
    rng = random.Random(3)
    sample = cases[::40]
    arrays, supplied = dm.pack_split(lib, waves, sample, rng)
    k = dm.SPLIT[waves]
    for j, (cs, (As, Rs)) in enumerate(zip(sample, supplied)):
        parts, chunks = dm.split_rule(waves, cs["c"], cs["dm"], cs["sp"])
        assert sum(v << (k["G"] * i) for i, v in enumerate(parts[:k["H"]])) == cs["c"]
        assert sum(v << (k["CB"] * q) for q, v in enumerate(chunks)) == cs["sp"]
        ok = dm.split_is_identity(waves, parts, cs["dneg"], chunks, As, Rs)
        assert (dm.SUCCESS if ok else dm.ERR_MSG) == dm.case_expect(cs)
        # the packed extended rows stand for the supplied points
        for i in range(1, k["H"]):
            for side, ext in ((0, As), (1, Rs)):
                row = (2 * i + side) * 40
                got = tuple(du.fe_val(arrays["pts"][row + 10 * c:row + 10 * c + 10, j]) for c in range(4))
                assert got == ext[i] and ext[i][2] != 1


# the strict bound too where it changes the form: at 131 bits halfsize.npz's and longd.npz's signatures have
# no record and take the full-length form
@pytest.mark.parametrize("name,dbits", [("adversarial", 151), ("vectors", 151), ("halfsize", 151), ("longd", 151),
                                        ("mixed_order", 151), ("adversarial", 131), ("halfsize", 131), ("longd", 131)])
def test_model_gives_the_reference_verdicts(lib, name, dbits):
    from conftest import load_golden
    d = load_golden(name)
    n = len(d["msg_sz"])
    rows = {avx: dm.fixture_cases(lib, d, avx, dbits) for avx in (True, False)}
    n_full = n_eval = 0
    for i in range(n):
        group = None   # the equation's verdict, evaluated once for both flavours
        for avx, want in ((True, d["codes_avx512"]), (False, d["codes_portable"])):
            cs, A, R, _, _ = rows[avx][i]
            code = dm.precheck(cs["sflag"], cs["af"], cs["rf"], not avx)
            if code is None:
                if group is None:
                    group = dm.model_code(cs, not avx, A, R)
                    n_eval += 1
                code = group
            assert code == int(want[i]), (name, i, avx, code, int(want[i]))
        n_full += rows[True][i][0]["full"]
    print(f"{name}: {n} signatures, {n_eval} equations evaluated, {n_full} full-length")
    assert n_eval > 0 and (dbits == 151 or n_full > 0)


# ---- the validation ------------------------------------------------------------

def check(lib, form, a, n_max=1 << 20, dbits=151, no_ks=False):
    n = len(a["sflag"])
    c = lambda x, t: np.ascontiguousarray(x, t)
    arrs = [c(a["sflag"], np.uint8), c(a["hflag"], np.uint8), c(a["pflag"], np.uint8), c(a["pts"], np.int32),
            c(a["hs"], np.uint32)]
    if "k" in a and not no_ks:
        arrs += [c(a["k"], np.uint32), c(a["S"], np.uint8)]
    ptrs = [ctypes.c_void_p(x.ctypes.data) for x in arrs] + [None] * (7 - len(arrs))
    return lib.fd_ed25519_hip_private_diag_dsm_check(form, n, n_max, dbits, *ptrs)


def good(n=3, dbits=151):
    rng = random.Random(5)
    cases = [dm.half_case(rng.getrandbits(131), rng.getrandbits(dbits), rng.getrandbits(253), (rng.randrange(L), 0),
                          (rng.randrange(L), 1)) for _ in range(n)]
    return cases


def ok_then_refused(lib, form, mk, at, past, **kw):
    assert check(lib, form, mk(at), **kw) == 0, at
    assert check(lib, form, mk(past), **kw) == INVAL, past


def test_refuses_c_d_and_s_beyond_their_bounds(lib):
    def mk(field, dbits=151):
        def f(v):
            cs = good(dbits=dbits)
            cs[1][field] = v
            return dm.pack_nonsplit(cs)
        return f
    for form in range(4):
        ok_then_refused(lib, form, mk("c"), 2**131 - 1, 2**131)
        ok_then_refused(lib, form, mk("dm"), 2**151 - 1, 2**151)
        ok_then_refused(lib, form, mk("dm", 131), 2**131 - 1, 2**131, dbits=131)   # the strict engine's
        ok_then_refused(lib, form, mk("sp"), 2**253 - 1, 2**253)              # s_lo + 2^144 s_hi < 2^253

    def slo(v):   # s_lo on its own: hs rows 10..14
        a = dm.pack_nonsplit(good())
        a["hs"][10:15, 2] = du.words(v, 5)
        return a
    ok_then_refused(lib, 0, slo, 2**144 - 1, 2**144)


def test_refuses_k_and_S_of_a_full_length_item(lib):
    def mk(field):
        def f(v):
            cs = good()
            cs[2] = dm.full_case(5, 7, (3, 0), (4, 0))
            cs[2][field] = v
            cs[2]["sflag"] = 1
            return dm.pack_nonsplit(cs)
        return f
    for form in range(4):
        ok_then_refused(lib, form, mk("k"), 2**253 - 1, 2**253)
        ok_then_refused(lib, form, mk("S"), L - 1, L)
    a = mk("S")(L)
    a["sflag"][2] = 0   # S >= L is what a clear sflag says
    assert check(lib, 0, a) == 0
    assert check(lib, 0, mk("k")(1), no_ks=True) == INVAL       # a full-length item needs k and S
    assert check(lib, 0, dm.pack_nonsplit(good()), no_ks=True) == 0
    for waves in (4, 8):                                         # the split forms have no full-length item
        a, _ = dm.pack_split(lib, waves, good(), random.Random(1))
        assert check(lib, waves, a) == 0
        a["hflag"][1] |= dm.HF_FULL
        assert check(lib, waves, a) == INVAL


def test_refuses_n_flags_and_forms(lib):
    a = dm.pack_nonsplit(good(3))
    assert check(lib, 1, a, n_max=3) == 0 and check(lib, 1, a, n_max=2) == INVAL
    empty = {k: v[:0] if k in ("sflag", "hflag", "S") else v[:, :0] for k, v in a.items()}
    assert check(lib, 1, empty) == INVAL
    for form in (-1, 5, 6, 7, 9, 16):
        assert check(lib, form, a) == INVAL
    assert check(lib, 0, a, dbits=130) == INVAL and check(lib, 0, a, dbits=152) == INVAL
    for field, at, past in (("sflag", 1, 2), ("hflag", 1, 4), ("pflag", 3, 4)):
        for v, want in ((at, 0), (past, INVAL)):
            b = dm.pack_nonsplit(good(3))
            if field == "pflag":
                b[field][1, 2] = v
            else:
                b[field][2] = v
            assert check(lib, 0, b) == want, (field, v)


def test_refuses_point_limbs_beyond_a_decode(lib):
    tight = du.TIGHT
    for limb in range(10):
        top = (1 << du.W[limb]) - 1
        for row, at, past in ((limb, tight[limb], tight[limb] + 1), (limb, -tight[limb], -tight[limb] - 1),
                              (10 + limb, top, top + 1), (10 + limb, -tight[limb], -tight[limb] - 1),
                              (20 + limb, tight[limb], tight[limb] + 1), (30 + limb, top, top + 1)):
            def mk(v):
                a = dm.pack_nonsplit(good())
                a["pts"][row, 1] = v
                return a
            ok_then_refused(lib, limb % 4, mk, at, past)
    for waves in (4, 8):
        for row in (0, 19, 40 + 5, 80, 80 + 39, waves * 40 - 1):
            limb = row % 10
            hi = (1 << du.W[limb]) - 1 if row < 80 and row % 40 >= 10 else tight[limb]
            for at, past in ((hi, hi + 1), (-tight[limb], -tight[limb] - 1)):
                def mk(v):
                    a, _ = dm.pack_split(lib, waves, good(), random.Random(1))
                    a["pts"][row, 2] = v
                    return a
                ok_then_refused(lib, waves, mk, at, past)


def test_refuses_split_scalars_that_would_shift_out_of_range(lib):
    """160 - 4 W - SH0 >= 8: W <= 22 (S = 4), W <= 14 (S = 8), W = (bits + 4) >> 2"""
    for waves, kw, longest in ((4, 3, 87), (8, 2, 55)):
        for q in range(waves):
            def mk(bits):
                a, _ = dm.pack_split(lib, waves, good(), random.Random(1))
                a["hs"][kw * q:kw * q + kw, 0] = du.words((1 << bits) - 1, kw)
                return a
            ok_then_refused(lib, waves, mk, longest, longest + 1)
    for q in range(4):   # S = 4: a chunk of s' is 72 bits, its third word 8
        def mk(v):
            a, _ = dm.pack_split(lib, 4, good(), random.Random(1))
            a["hs"][12 + 3 * q + 2, 1] = v
            return a
        ok_then_refused(lib, 4, mk, 0xff, 0x100)
