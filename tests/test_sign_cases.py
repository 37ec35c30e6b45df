"""CPU: what the case builders of tests/sign_model.py promise the GPU tests
of tests/test_gpu_sign_diag.py -- the digits every scalar class recodes to,
the sizes and ranges of every class -- and the Python signer against the
reference's sign KATs.  No GPU and no library."""
import json
import os

import sign_model as sm
from conftest import GOLDEN
from diag_util import BASE, L, P
import diag_util as du
import dsm_model as dm


def test_python_signer_matches_sign_kat():
    kats = json.load(open(os.path.join(GOLDEN, "sign_kat.json")))
    got = sm.sign_many([bytes.fromhex(k["priv"]) for k in kats], [bytes.fromhex(k["msg"]) for k in kats])
    for k, g in zip(kats, got):
        assert g["pub"].hex() == k["pub"] and g["sig"].hex() == k["sig"], k["priv"]
        assert g["S"] < L and g["r"] < L and g["k"] < L and 2**254 <= g["a"] < 2**255 and g["a"] % 8 == 0
        assert sm.encode(dm.xaffine(dm.base_mul(g["a"] % L))) == int.from_bytes(g["pub"], "little")


def test_base_points_match_the_affine_law():
    """the extended-coordinate multiply with one shared inversion, against du.ed_mul"""
    xs = [0, 1, 2, 128, L - 1, 2**252, 0x1234567 << 200]
    assert sm.base_points(xs) == [du.ed_mul(x, BASE) for x in xs]
    assert sm.base_points([L + 5]) == [du.ed_mul(5, BASE)]


def test_recode256_is_the_signed_radix():
    for s in (0, 1, 127, 128, 255, 256, 0x80 << 240, L - 1, int.from_bytes(b"\x80" * 31 + b"\x0f", "little")):
        d = sm.recode256(s)
        assert sum(f << (8 * j) for j, f in enumerate(d)) == s
        assert all(-128 <= f <= 127 for f in d[:31]) and 0 <= d[31] <= 16
    assert sm.recode256(128)[:2] == [-128, 1]


def test_table_model():
    t = sm.table()
    assert len(t) == 129 and t[0] == (1, 1, 0)
    assert sm.entry_point(t[1]) == BASE and sm.entry_point(t[128]) == du.ed_mul(128, BASE)
    for e in (1, 2, 77, 128):
        x, y = sm.entry_point(t[e])
        assert du.on_curve((x, y)) and t[e][2] == 2 * du.D * x * y % P


def test_base_scalars_cover_every_digit():
    xs, classes = sm.base_scalars()
    assert all(0 <= x < L for x in xs)
    assert len(xs) % 256 != 0                       # the last block is partial
    assert len(xs) > 256 * 8                        # several blocks
    want = {"edges", "small", "byte alone", "byte over ones", "repeated", "powers", "every byte", "top"}
    assert want <= set(classes)
    assert classes["small"][1] - classes["small"][0] == 129 + 128
    assert classes["powers"][1] - classes["powers"][0] == 2 * 253
    # position 31 admits 0x01 alone; every other position all five values, alone and over ones
    assert classes["byte alone"][1] - classes["byte alone"][0] == 31 * 5 + 1
    assert classes["byte over ones"][1] - classes["byte over ones"][0] == 31 * 5 + 1
    seen = [set() for _ in range(32)]
    runs = set()
    for x in xs:
        d = sm.recode256(x)
        for j, f in enumerate(d):
            seen[j].add(f)
        runs.add(sm.leading_zero_digits(d))
    for j in range(31):
        assert seen[j] == set(range(-128, 128)), (j, sorted(set(range(-128, 128)) - seen[j]))
    assert seen[31] == set(sm.TOP_DIGITS)           # 0 .. 16: all that a scalar below L admits
    assert {1, 2, 16, 31, 32} <= runs
    # digit -128 (table entry 128, negated) next to every kind of neighbour
    assert any(sm.recode256(x)[j] == -128 and sm.recode256(x)[j + 1] == -127 for x in xs for j in range(30))


def test_top_digit_17_needs_a_scalar_above_l():
    """the least scalar whose digit 31 is 17: top byte 0x10 over the least 31 bytes that carry out (0x7f .. 0x7f 0x80)"""
    least = (0x10 << 248) | int.from_bytes(b"\x80" + b"\x7f" * 30, "little")
    assert sm.recode256(least)[31] == 17 and sm.recode256(least - 1)[31] == 16 and least > L


def test_base_wide_scalars():
    xs = sm.base_wide_scalars()
    assert all(0 <= x < 2**256 for x in xs)
    assert {2**254, 2**255 - 8, 2**256 - 1} <= set(xs)
    for m in range(1, 16):
        assert {L * m - 1, L * m + 1} <= set(xs)
    assert 16 * L - 1 > 2**256 - 1                  # no further multiple fits
    assert len(xs) >= 300 + 30 + 3 and len(xs) % 256 != 0
    assert any(x % L == 0 for x in xs) and any(x % L == L - 1 for x in xs)


def test_muladd_triples():
    ts = sm.muladd_triples()
    s = set(ts)
    m = sm.M256
    assert {(k, a, r) for k in (0, 1, m) for a in (0, 1, m) for r in (0, 1, m)} <= s
    assert {(k, a, r) for k in (L - 1, L, L + 1) for a in (2**254, 2**255 - 8) for r in (L - 1, m)} <= s
    for w in range(8):
        one = 0xffffffff << (32 * w)
        assert (one, 0, 0) in s and (0, one, 0) in s and (0, 0, one) in s
    assert (m, m, m) in s and (m * m + m) % 2**256 == 0 and (m * m + m) >> 256 == m
    assert sum(1 for k, a, r in ts if (k * a + r) % L == 0) >= 40
    assert sum(1 for k, a, r in ts if (k * a + r) % L == L - 1) >= 40
    assert len(ts) >= 2000 + 27 + 12 and len(ts) % 256 != 0
    assert max(k * a + r for k, a, r in ts) == 2**512 - 2**256     # the largest value the product can take


def test_encode_cases():
    cases = sm.encode_cases()
    hi, lo = sm.encode_bound()
    names = {c[4].split(",")[0] for c in cases}
    assert {"identity", "order 2", "order 4", "order 4'", "order 8", "B", "random"} <= names
    for z in ("Z = 1", "Z plain", "Z unsigned", "Z at the bound"):
        assert any(z in c[4] for c in cases)
    signs = set()
    for X, Y, Z, pt, note in cases:
        z = du.fe_val(Z)
        assert z and du.fe_val(X) == pt[0] * z % P and du.fe_val(Y) == pt[1] * z % P, note
        assert all(abs(v) <= h for v, h in zip(X, hi["X"])) and all(abs(v) <= h for v, h in zip(Y, hi["Y"])), note
        assert du.within(Z, lo["Z"], hi["Z"]), note
        signs.add((pt[0] & 1, min(X) < 0, min(Y) < 0))
    assert {(0, False, False), (1, False, False), (0, True, True), (1, True, True)} <= signs
    assert any(pt[0] == 0 for *_, pt, _ in cases) and any(pt[1] == 0 for *_, pt, _ in cases)
    assert any(pt[1] == P - 1 for *_, pt, _ in cases)               # y next to p
    assert len(cases) % 256 != 0


def test_root_cases_reach_every_table_entry_of_either_sign():
    """the digits of a mod L and r over the 2048 root signatures take every value in [-128, 127]"""
    privs, msgs = sm.root_cases()
    assert len(privs) == len(msgs) == sm.ROOTS == 2048 and all(len(m) == 32 and len(p) == 32 for p, m in zip(privs, msgs))
    assert len(set(privs)) == 2048
    seen = set()
    for g in sm.root_signatures():
        for s in (g["a"] % L, g["r"]):
            seen.update(sm.recode256(s)[:31])
    assert seen == set(range(-128, 128))
