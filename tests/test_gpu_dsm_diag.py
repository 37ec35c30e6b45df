"""The seven dsm loops -- dsm_half_one in the one-lane kernel, dsm4, dsm8,
dsm16, dsm16s<4>, dsm16s<8> and the full-length dsm_full_core -- on chosen
scalars, points and flags: the product's own kernels launched as the dsm
phase alone on work arrays this test writes (Engine.diag_dsm), every code
compared with the plain-integer model (tests/dsm_model.py).  Exact.

The group equation is linear, so for chosen c, d, A = [a]B + T_A and R =
[r]B + T_R one of s', r, a is solved to make the sum the identity: the loop
must answer SUCCESS, and ERR_MSG for each one-step perturbation (s' +- 1, a
window of c or |d| changed by 1, the sign flag flipped, R negated, T_R
replaced so the sum is each non-identity torsion point -- the order-2 one
has X == 0).  The operand classes are in dsm_model.crafted_half_cases /
crafted_full_cases; tests/test_dsm_model.py (CPU) pins the model first."""
import random
import time

import numpy as np
import pytest

import dsm_model as dm
from diag_util import L

pytestmark = pytest.mark.gpu

NONSPLIT = ("wide", "quad", "oct", "r16")
MAX_CHUNK = 8192


@pytest.fixture(scope="module")
def engines():
    from firedancer_amd import ed25519
    made = {}

    def get(tables="compact", codes="avx512", half="extended"):
        key = (tables, codes, half)
        if key not in made:
            made[key] = ed25519.Engine(0, max_chunk=MAX_CHUNK, dsm="r16", compact=tables == "compact", codes=codes,
                                       half=half)
        return made[key]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def lib():
    from firedancer_amd import ed25519
    return ed25519.library()


@pytest.fixture(scope="module")
def crafted():
    """the crafted cases, their expected codes and their arrays per layout, built once"""
    cases, kinds = dm.crafted_half_cases()
    full = dm.crafted_full_cases()
    return dict(half=cases, kinds=kinds, full=full, arrays={}, exp=np.array([dm.case_expect(c) for c in cases], np.int8),
                exp_full=np.array([dm.case_expect(c) for c in full], np.int8))


def arrays_for(crafted, lib, layout):
    """layout: "nonsplit" (half-size and full-length cases, interleaved), 4, 8"""
    if layout not in crafted["arrays"]:
        if layout == "nonsplit":
            cases, exp = list(crafted["half"]), list(crafted["exp"])
            step = len(cases) // len(crafted["full"])
            for i, (cs, e) in enumerate(zip(crafted["full"], crafted["exp_full"])):   # scattered through the rest
                cases.insert(i * (step + 1), cs)
                exp.insert(i * (step + 1), e)
            crafted["arrays"][layout] = (dm.pack_nonsplit(cases), np.array(exp, np.int8), cases)
        else:
            a, _ = dm.pack_split(lib, layout, crafted["half"], random.Random(layout))
            crafted["arrays"][layout] = (a, crafted["exp"], crafted["half"])
    return crafted["arrays"][layout]


def run(eng, form, a):
    return eng.diag_dsm(dm.FORMS[form], a["sflag"], a["hflag"], a["pflag"], a["pts"], a["hs"], a.get("k"), a.get("S"))


def agree(got, exp, cases, what):
    bad = np.nonzero(got != exp)[0]
    assert not len(bad), (what, len(bad), len(exp), [(int(i), int(got[i]), int(exp[i]), cases[i]) for i in bad[:4]])


def layout_of(form):
    return "nonsplit" if form in NONSPLIT else int(form[-1])


ALL = [(f, t) for f in NONSPLIT for t in ("wide", "compact")] + [("split4", "compact"), ("split8", "compact")]


@pytest.mark.parametrize("form,tables", ALL)
def test_crafted_cases(engines, lib, crafted, form, tables):
    """every crafted case in one launch per form (the larger set), with the
    wide and the compact base tables"""
    a, exp, cases = arrays_for(crafted, lib, layout_of(form))
    eng = engines(tables)
    t = time.perf_counter()
    got = run(eng, form, a)
    print(f"{form}/{tables}: {len(exp)} cases ({int((exp == 0).sum())} SUCCESS, {int((exp == -3).sum())} ERR_MSG), "
          f"launch {time.perf_counter() - t:.2f} s")
    assert len(exp) >= 2000 and (exp == 0).sum() >= 500 and (exp == -3).sum() >= 1000
    agree(got, exp, cases, form)


@pytest.mark.parametrize("form", NONSPLIT + ("split4", "split8"))
def test_batch_sizes(engines, lib, crafted, form):
    """n in {1, 2, 3, 5, 63, 64, 65}: windows of the crafted set, each
    starting elsewhere so that every case meets a small launch"""
    a, exp, cases = arrays_for(crafted, lib, layout_of(form))
    eng, start = engines(), 0
    for rnd in range(3):
        for n in (1, 2, 3, 5, 63, 64, 65):
            idx = np.arange(start, start + n) % len(exp)
            agree(run(eng, form, dm.take(a, idx)), exp[idx], [cases[i] for i in idx], (form, n, start))
            start += 97 * n + 13


def d_length_cases(dbits, seed=3):
    rng = random.Random(seed)
    A = (rng.randrange(1, L), 3)
    out = []
    for dmag in dm.d_lengths(120, dbits):
        for sign in (1, -1):
            c, d = rng.getrandbits(131), sign * dmag
            tr = dm.solve_tr(c, d, A[1])
            a = A if tr is not None else (A[0], 0)
            sp = rng.randrange(L)
            R = (dm.solve_r(c, d, sp, a), tr or 0)
            out += [dm.half_case(c, d, sp, a, R), dm.half_case(c, d, (sp + 1) % L, a, R),
                    dm.half_case(c, -d, sp, a, R, dneg=int(d > 0))]
    return out


@pytest.mark.parametrize("form", NONSPLIT + ("split4", "split8"))
def test_d_lengths_sorted_and_interleaved(engines, lib, form):
    """|d| = 2^(b-1) and 2^b - 1 on both sides of every window step (W =
    33..38; 17..22 and 9..14 in the split forms): sorted by length, so waves
    share W, and interleaved, so waves of the one-lane, quad and oct forms
    hold one long lane among short ones and the reverse"""
    cases = d_length_cases(151)
    short = [c for c in cases if c["dm"] < 2**127]
    long_ = [c for c in cases if c["dm"] >= 2**150]
    assert short and long_
    rng = random.Random(1)
    mixed = list(cases)
    rng.shuffle(mixed)
    lone_long = [short[i % len(short)] for i in range(64)]
    lone_long[17] = long_[0]
    lone_short = [long_[i % len(long_)] for i in range(64)]
    lone_short[40] = short[0]
    eng = engines()
    for name, cs in (("sorted", cases), ("interleaved", mixed), ("one long", lone_long + lone_long[:7]),
                     ("one short", lone_short)):
        exp = np.array([dm.case_expect(c) for c in cs], np.int8)
        assert (exp == 0).any() and (exp == -3).any()
        if form in NONSPLIT:
            a = dm.pack_nonsplit(cs)
        else:
            a, _ = dm.pack_split(lib, int(form[-1]), cs, rng)
        agree(run(eng, form, a), exp, cs, (form, name))


@pytest.mark.parametrize("tables", ["wide", "compact"])
def test_wide_form_full_length_counts(engines, crafted, tables):
    """the one-lane kernel's fix_list: 0, 1, 63, 64, 65 full-length items
    scattered through an n that is no multiple of 64 (the head rounding and
    the work counter)"""
    eng, rng = engines(tables), random.Random(9)
    for nfull in (0, 1, 63, 64, 65):
        n = 199 + nfull
        where = set(rng.sample(range(n), nfull))
        half = iter(rng.sample(crafted["half"], n - nfull))
        full = iter(rng.sample(crafted["full"], nfull))
        cases = [next(full) if j in where else next(half) for j in range(n)]
        exp = np.array([dm.case_expect(c) for c in cases], np.int8)
        agree(run(eng, "wide", dm.pack_nonsplit(cases)), exp, cases, ("wide", nfull))


@pytest.mark.parametrize("codes", ["avx512", "portable"])
@pytest.mark.parametrize("form", NONSPLIT + ("split4", "split8"))
def test_precheck_order(engines, lib, crafted, form, codes):
    """all 2 x 4 x 4 flag combinations over an identity and a non-identity
    sum (and, where the form runs it, a full-length item), in both code
    flavours: the reference's order, whatever the equation says"""
    valid = [c for c, k in zip(crafted["half"], crafted["kinds"]) if k == "valid"][:3]
    miss = [c for c, k in zip(crafted["half"], crafted["kinds"]) if k == "sp"][:3]
    base = valid + miss + (crafted["full"][:2] if form in NONSPLIT else [])
    cases = [dict(b, sflag=s, af=af, rf=rf) for b in base for s in (0, 1) for af in range(4) for rf in range(4)]
    portable = codes == "portable"
    exp = np.array([dm.case_expect(c, portable) for c in cases], np.int8)
    assert set(exp.tolist()) == {0, -1, -2, -3}
    if form in NONSPLIT:
        a = dm.pack_nonsplit(cases)
    else:
        a, _ = dm.pack_split(lib, int(form[-1]), cases, random.Random(2))
    agree(run(engines(codes=codes), form, a), exp, cases, (form, codes))


def test_strict_engine_stops_at_131_bits(engines):
    """under FLAG_HALF_STRICT the same classes with |d| < 2^131, and a
    refusal (nothing launched) of a longer one"""
    from firedancer_amd import ed25519
    eng = engines(half="strict")
    cases = d_length_cases(131)
    exp = np.array([dm.case_expect(c) for c in cases], np.int8)
    for form in ("wide", "r16"):
        agree(run(eng, form, dm.pack_nonsplit(cases)), exp, cases, form)
    long_ = [c for c in d_length_cases(151) if c["dm"] >= 2**131][:1]
    with pytest.raises(ed25519.HipError):
        run(eng, "r16", dm.pack_nonsplit(cases[:5] + long_))
    with pytest.raises(ed25519.HipError):   # and n beyond what the engine's forms admit
        run(eng, "quad", dm.take(dm.pack_nonsplit(cases), np.arange(MAX_CHUNK + 1) % len(cases)))


@pytest.mark.parametrize("form", NONSPLIT + ("split4", "split8"))
def test_adversarial_fixture_through_the_diagnostic(engines, lib, adversarial, form):
    """the tie to the real path: the arrays built from hsrec / hsdec_n for
    adversarial.npz (those tests/test_dsm_model.py feeds the model) give
    the golden codes in every form"""
    rows = dm.fixture_cases(lib, adversarial, True, 151)
    keep = [i for i, r in enumerate(rows) if form in NONSPLIT or not r[0]["full"]]
    cases = [rows[i][0] for i in keep]
    pts = [(rows[i][1], rows[i][2]) for i in keep]
    want = adversarial["codes_avx512"][keep].astype(np.int8)
    assert len(keep) >= 990
    if form in NONSPLIT:
        a = dm.pack_nonsplit(cases, pts)
        for j, i in enumerate(keep):   # hsdec_n's own limbs, not a re-encoding of their values
            a["pts"][:20, j], a["pts"][20:, j] = rows[i][3], rows[i][4]
    else:
        a, _ = dm.pack_split(lib, int(form[-1]), cases, random.Random(4), pts)
    agree(run(engines(), form, a), want, cases, form)
