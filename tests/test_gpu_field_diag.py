"""Device field arithmetic on chosen limb vectors (libfd_ed25519_diag.so):
every function of fd25519_fe.h, fe_sq_sh of fd25519_ge4.h and the
lane-split field of fd25519_r16.h, one function per kernel, against
Python integers.

A verify only hands these functions limbs derived from a hash or a
decompressed point.  Here the operands sit at the documented limb bounds,
stand for the special values of the field in several representations, and
are chosen so that a column carry lands exactly on a chain's edges.  Per
case the test asserts

  * the value of the output limbs is the exact result mod p;
  * fe_tobytes of the output is the canonical encoding, and fe_iszero /
    fe_isodd agree with it;
  * every output limb lies in the interval tests/bounds_model.py derives for
    the operation from the hull of the case's input class -- and, the model
    being an exact restatement when its inputs are points, that the device's
    limbs are the very limbs the model computes for that case.

The last ties the interval proofs of tests/test_bounds.py to the device
code: a limb outside the model's interval fails even when the value is
right.  No tolerances; every case is checked."""
import random

import pytest

import bounds_model as bm
import diag_util as du
from diag_util import P, Diag, s32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def diag():
    return Diag()


def e(k, v=1):
    z = [0] * 10
    z[k] = v
    return z


def carry_patterns():
    """class (d): limb vectors whose limbs are the column sums of a product
    with (1, 0, .., 0) and of fe_carry: a column (with what the chain carried
    into it) exactly at 2^w - 1, 2^w, -1, -2^w (the floor chains' edges) and
    at +-2^(w-1) and one off (the centered chains' rounding boundary), alone
    and rippling through every column, across the 4 -> 5 join and the 19 x
    wrap from limb 9 into limb 0.  All within 3.3x."""
    W = du.W
    out = []
    for k in range(10):
        w = W[k]
        for t in (2**w - 1, 2**w, 2**w + 1, -1, -2**w, -2**w - 1, 2**(w - 1) - 1, 2**(w - 1), -2**(w - 1),
                  -2**(w - 1) - 1, 3 * 2**(w - 1) - 1, 3 * 2**(w - 1), -3 * 2**(w - 1), -3 * 2**(w - 1) - 1):
            out.append(e(k, t))
    full = [2**w - 1 for w in W]
    half = [2**(w - 1) - 1 for w in W]
    for base in (full, half):
        for k in range(10):
            for d in (1, 2, -1):
                v = list(base)
                v[k] += d
                out.append(v)
                out.append([-x for x in v])
    # the wrap: 19 x (carry out of limb 9) lands limb 0 exactly on 2^26 - 1, 2^26 and the rounding boundary
    for l0 in (2**26 - 20, 2**26 - 19, 2**26 - 18, 2**25 - 20, 2**25 - 19, 2**25 - 18):
        for k in (5, 9):
            v = list(full)
            v[0] = l0
            v[k] += 1
            out.append(v)
    for l9 in (2**24 - 1, 2**24, 2**25 - 1, 2**25):
        for l0 in (2**25 - 19, 2**25 - 20, 2**26 - 19, 2**26 - 20, -2**25 - 19, -2**25 - 20):
            v = e(9, l9)
            v[0] = l0
            out.append(v)
    lo = [-x for x in du.B33]
    assert all(du.within(v, lo, du.B33) for v in out)
    return out


def sq_columns(f, s):
    """the column sums of s f^2 as fe_sq / fe_sq2 / fe_sqs_u<S> / fe_sq_sh form them"""
    col = [0] * 10
    for i in range(10):
        for j in range(i, 10):
            m = (2 if (i & 1 and j & 1) else 1) * (19 if i + j >= 10 else 1)
            x = s * f[i] if i == j else 2 * s * f[i]
            col[(i + j) % 10] += x * m * f[j]
    return col


def floor_totals(col):
    """what each step of the unsigned forms' two floor chains splits
    (fd25519_fe.h fe_sqs_u / fe_mul19_u, fe_join_u): the column sum plus the
    carry into it, the 4 -> 5 join and the 19 x wrap into limb 0"""
    W, tot, c = du.W, {}, 0
    for k in range(5):
        tot["A", k] = t = col[k] + c
        c = t >> W[k]
    c4, c = c, 0
    for k in range(5, 10):
        tot["B", k] = t = col[k] + c
        c = t >> W[k]
    tot["join", 5] = c4 + (tot["B", 5] & ((1 << 25) - 1))
    tot["wrap", 0] = 19 * c + (tot["A", 0] & ((1 << 26) - 1))
    return tot


def centered_totals(col):
    """a plain centered chain over the columns (the device's fe_carry_wide
    carries limbs 0 and 4 twice; between those it rounds the same way)"""
    W, tot, c = du.W, {}, 0
    for k in range(10):
        tot["C", k] = t = col[k] + c
        c = (t + (1 << (W[k] - 1))) >> W[k]
    return tot


def sq_carry_operands(s, hi, centered):
    """class (d) for the squarings, whose columns are not their operand's
    limbs: operands f (0 <= f <= hi limb by limb) built so that, in the chain
    restated above, a column of s f^2 with the carry into it is exactly on
    an edge -- 2^w - 1 and 2^w for the floor chains (every column that takes
    a carry, the join and the wrap), 2^(w-1) - 1 and 2^(w-1), the rounding
    boundary, for the centered ones.  A two-limb operand a e_i + b e_j puts
    2 s a b (times the column's factors) into column i + j, about 2^51, so
    that its carry is the edge of column i + j + 1; b is found by bisection
    (the total is monotone in b).  Returns (operands, edges reached,
    edges wanted)."""
    W = du.W
    totals = centered_totals if centered else floor_totals
    targets = []
    for m in range(1, 10):
        key = ("C", m) if centered else ("join", 5) if m == 5 else ("A" if m < 5 else "B", m)
        w = W[m] - 1 if centered else W[m]
        targets += [(key, m - 1, (1 << w) - 1), (key, m - 1, 1 << w)]
    if not centered:
        targets += [(("wrap", 0), 9, (1 << 26) - 1), (("wrap", 0), 9, 1 << 26)]
    a_cands = [(1 << sh) + d for sh in (24, 23, 22, 21, 20, 19, 18) for d in (1, 3, 0, 12345, 7)] + list(range(1, 40))
    out, reached = [], set()
    for key, src, edge in targets:
        found = None
        for i in range(10):
            j = (src - i) % 10
            if i == j:
                continue
            for a in a_cands:
                if a > hi[i]:
                    continue

                def make(b, i=i, j=j, a=a):
                    f = [0] * 10
                    f[i], f[j] = a, b
                    return f
                lo_b, hi_b = 0, hi[j]
                while lo_b < hi_b:
                    mid = (lo_b + hi_b) // 2
                    if totals(sq_columns(make(mid), s))[key] >= edge:
                        hi_b = mid
                    else:
                        lo_b = mid + 1
                if totals(sq_columns(make(lo_b), s))[key] == edge:
                    found = make(lo_b)
                    break
            if found:
                break
        if found:
            out.append(found)
            reached.add((key, edge))
    return out, reached, {(k, e_) for k, _, e_ in targets}


def unsigned_2x():
    """what the _u forms return: limbs in [0, 2^w), limbs 1 and 6 up to 2^10 above"""
    return [(1 << w) - 1 + (1 << 10 if k in (1, 6) else 0) for k, w in enumerate(du.W)]


# op -> (bound of f, bound of g or None, exact result, bounds_model restatement).
# The input bounds: fd25519_fe.h:22 "mul/sq accept inputs <= 3.3x" (both
# operands; tests/test_bounds.py asserts the model accepts them), and tight
# operands (fd25519_fe.h:19, <= 1.01x) where the factor 2 is folded into the
# left operands (fe_sq2, fe_sq2_u; fe_sq_sh, fd25519_ge4.h:55-56 "inputs
# tight there").  fe_carry / fe_tobytes: fd25519_fe.h:375 "any input within
# the mul bounds is accepted".
OPS = {
    "mul": (du.B33, du.B33, lambda f, g: f * g, lambda f, g: bm.fe_mul(f, g)),
    "mul19": (du.B33, du.B33, lambda f, g: f * g, lambda f, g: bm.fe_mul19(f, g, bm.fe_19(g))),
    "sq": (du.B33, None, lambda f, g: f * f, lambda f, g: bm.fe_sqs(f)),
    "sq2": (du.TIGHT, None, lambda f, g: 2 * f * f, lambda f, g: bm.fe_sqs(f, 2)),
    "mul_u": (du.B33, du.B33, lambda f, g: f * g, lambda f, g: bm.fe_mul_u(f, g)),
    "sq_u": (du.B33, None, lambda f, g: f * f, lambda f, g: bm.fe_sqs_u(f)),
    "sq2_u": (du.TIGHT, None, lambda f, g: 2 * f * f, lambda f, g: bm.fe_sqs_u(f, 2)),
    "carry": (du.B33, None, lambda f, g: f, lambda f, g: bm.fe_carry(f)),
    "ident": (du.B33, None, lambda f, g: f, lambda f, g: list(f)),
}


# the squarings' own chains: op -> (the folded factor S, centered chain)
SQ_CHAINS = {"sq": (1, True), "sq2": (2, True), "sq_u": (1, False), "sq2_u": (2, False)}


def sq_carry_class(s, hi, centered):
    """the operands of sq_carry_operands and their negatives (the same columns)"""
    fs = sq_carry_operands(s, hi, centered)[0]
    return fs + [[-x for x in f] for f in fs]


def classes_for(op):
    """{class name: [(f, g)]}, g None for the one-operand forms"""
    bf, bg, _, _ = OPS[op]
    rng = random.Random(sum(map(ord, op)) + 61)
    cl = {}
    fa, fb, fc = du.fe_random(rng, 300, bf), du.fe_extremes(bf), du.fe_special_reps(bf)
    fd = carry_patterns() if bf is du.B33 else [v for v in carry_patterns() if du.within(v, [-x for x in bf], bf)]
    if bg is None:
        cl["random"] = [(f, None) for f in fa]
        cl["extremes"] = [(f, None) for f in fb]
        cl["special"] = [(f, None) for f in fc]
        cl["carries"] = [(f, None) for f in fd]
        if op in SQ_CHAINS:
            cl["sq_carries"] = [(f, None) for f in sq_carry_class(SQ_CHAINS[op][0], bf, SQ_CHAINS[op][1])]
        if op == "sq2_u":   # ge_p2_dbl squares an unsigned-form Z (fd25519_ge.h:85 "|Z| <= 2x")
            u = unsigned_2x()
            cl["unsigned"] = [(f, None) for f in du.fe_random(rng, 100, u, [0] * 10) + du.fe_extremes(u, [0] * 10)]
    else:
        ga, gb, gc = du.fe_random(rng, 300, bg), du.fe_extremes(bg), du.fe_special_reps(bg)
        cl["random"] = list(zip(fa, ga))
        cl["extremes"] = [(f, g) for f in fb for g in gb]
        cl["special"] = [(f, gc[(7 * i + s) % len(gc)]) for i, f in enumerate(fc) for s in (0, 3)]
        one = [e(0, 1), e(0, -1), e(0, 2), e(0, 2**13), e(0, -2**12)]
        cl["carries"] = [(o, g) for o in one for g in fd] + [(f, o) for o in one[:2] for f in fd]
    return cl


def check_outputs(op, label, pairs, out, want_of, model):
    """the three assertions for one class"""
    fs = [f for f, _ in pairs]
    gs = [g for _, g in pairs if g is not None]
    iv = model(du.hull(fs), du.hull(gs) if gs else None)
    for (f, g), o in zip(pairs, out):
        h = [s32(v) for v in o[:10]]
        fv = du.fe_val(f)
        want = want_of(fv, du.fe_val(g) if g is not None else None) % P
        ctx = (op, label, f, g)
        assert du.fe_val(h) == want, ctx
        assert [int(v) for v in o[10:18]] == du.canonical_words(want), ctx
        assert int(o[18]) == (1 if want == 0 else 0) and int(o[19]) == (want & 1), ctx
        assert du.inside(h, iv), (ctx, h, iv)
        exact = model(du.point_iv(f), du.point_iv(g) if g is not None else None)
        assert h == [lo for lo, _ in exact] and all(lo == hi for lo, hi in exact), (ctx, h, exact)


@pytest.mark.parametrize("op", list(OPS))
def test_fe_operation(diag, op):
    _, _, want_of, model = OPS[op]
    total = 0
    for label, pairs in classes_for(op).items():
        out = diag.run("fe", op, [list(f) + (list(g) if g is not None else []) for f, g in pairs])
        check_outputs(op, label, pairs, out, want_of, model)
        total += len(pairs)
    print(f"fe_{op}: {total} cases")


@pytest.mark.parametrize("sh", [0, 1])
def test_fe_sq_sh(diag, sh):
    rng = random.Random(62 + sh)
    bnd = du.TIGHT if sh else du.B33
    classes = {"random": du.fe_random(rng, 300, bnd), "extremes": du.fe_extremes(bnd),
               "special": du.fe_special_reps(bnd),
               "carries": [v for v in carry_patterns() if du.within(v, [-x for x in bnd], bnd)],
               "sq_carries": sq_carry_class(1 + sh, bnd, True)}
    total = 0
    for label, fs in classes.items():
        pairs = [(f, None) for f in fs]
        out = diag.run("fe", "sq_sh", [list(f) + [sh] for f in fs])
        check_outputs(f"sq_sh{sh}", label, pairs, out, lambda f, g: (1 + sh) * f * f,
                      lambda f, g: bm.fe_sqs(f, 1 + sh))
        total += len(fs)
    print(f"fe_sq_sh({sh}): {total} cases")


def test_fe_frombytes(diag):
    rng = random.Random(63)
    vals = [0, 1, P - 1, P, P + 1, 2**255 - 1, 2**255 - 20, 2**254, 2**255 - 19 + 2**128]
    vals += [(1 << du.OFF[i]) - 1 for i in range(1, 10)] + [1 << du.OFF[i] for i in range(1, 10)]
    vals += [rng.getrandbits(255) for _ in range(300)]
    xs = [v | (b << 255) for v in vals for b in (0, 1)]      # bit 255 is ignored
    out = diag.run("fe", "frombytes", [du.words(x, 8) for x in xs])
    iv = bm.frombytes()
    for x, o in zip(xs, out):
        h = [s32(v) for v in o[:10]]
        want = (x % 2**255) % P
        assert du.fe_int(h) == x % 2**255, hex(x)          # the plain digits, values >= p kept as they are
        assert du.inside(h, iv), (hex(x), h)
        assert [int(v) for v in o[10:18]] == du.canonical_words(want), hex(x)
        assert int(o[18]) == (want == 0) and int(o[19]) == (want & 1), hex(x)
    print(f"fe_frombytes: {len(xs)} cases")


def model_invert(z):
    """fd25519_fe.h fe_invert over intervals"""
    t = bm.fe_pow22523(z)
    for _ in range(3):
        t = bm.fe_hull(t, bm.fe_sqs_u(t))
    return bm.fe_mul(t, bm.fe_mul(bm.fe_sqs(z), z))


def pow_exact(z):
    """fe_pow22523's chain limb for limb (bounds_model's own version stops
    each run of squarings at the intervals' fixed point)"""
    def sqn(f, n):
        for _ in range(n):
            f = bm.fe_sqs_u(f)
        return f
    m = bm.fe_mul_u
    t0 = sqn(z, 1)
    t1 = m(z, sqn(t0, 2))
    t0 = m(t0, t1)
    t0 = m(t1, sqn(t0, 1))
    t0 = m(sqn(t0, 5), t0)
    t1 = m(sqn(t0, 10), t0)
    t1 = m(sqn(t1, 20), t1)
    t0 = m(sqn(t1, 10), t0)
    t1 = m(sqn(t0, 50), t0)
    t1 = m(sqn(t1, 100), t1)
    t0 = m(sqn(t1, 50), t0)
    return m(sqn(t0, 2), z)


def invert_exact(z):
    t = pow_exact(z)
    for _ in range(3):
        t = bm.fe_sqs_u(t)
    return bm.fe_mul(t, bm.fe_mul(bm.fe_sqs(z), z))


def pow_operands():
    """z in {1, 2 (a non-residue: p = 5 mod 8), p - 1, sqrt(-1), 0, random},
    tight limbs at both signs: the centered digits of z, and the negated
    centered digits of -z"""
    rng = random.Random(64)
    zs = [1, 2, P - 1, du.SQRTM1, P - du.SQRTM1, 0, 2**254, (P - 1) // 2, 3]
    assert pow(2, (P - 1) // 2, P) == P - 1
    zs += [rng.randrange(P) for _ in range(60)]
    out = []
    for z in zs:
        out.append(du.fe_centered(z))
        out.append([-x for x in du.fe_centered(-z % P)])
        out.append([-x for x in du.fe_centered(P - z)] if z else du.fe_centered(P, True))
    out += du.fe_extremes(du.TIGHT)
    lo = [-x for x in du.TIGHT]
    assert all(du.within(v, lo, du.TIGHT) for v in out) and len(out) <= 300
    return out


@pytest.mark.parametrize("op", ["pow22523", "invert"])
def test_fe_exponentiations(diag, op):
    zs = pow_operands()
    exp = 2**252 - 3 if op == "pow22523" else P - 2
    model, exact = (bm.fe_pow22523, pow_exact) if op == "pow22523" else (model_invert, invert_exact)
    out = diag.run("fe", op, zs)
    iv = model(du.hull(zs))
    for n, (z, o) in enumerate(zip(zs, out)):
        h = [s32(v) for v in o[:10]]
        want = pow(du.fe_val(z), exp, P)
        assert du.fe_val(h) == want, (op, z)
        assert [int(v) for v in o[10:18]] == du.canonical_words(want), (op, z)
        assert int(o[18]) == (want == 0) and int(o[19]) == (want & 1), (op, z)
        assert du.inside(h, iv), (op, z, h, iv)
        if n % 40 == 0:   # the chain restated limb for limb (265 products in Python: a few cases)
            assert h == [lo for lo, _ in exact(du.point_iv(z))], (op, z)
    print(f"fe_{op}: {len(zs)} cases")


# ---- the lane-split field (fd25519_r16.h) ------------------------------------

def r16_operands(rng):
    top = du.R16_IN - 1
    ops = [[rng.randrange(du.R16_IN) for _ in range(16)] for _ in range(300)]
    ops += [du.r16_random_tight(rng) for _ in range(60)]
    ops += [[top] * 16, [top] + [0] * 15, [0] * 15 + [top], [du.R16_TIGHT] * 16, [0] * 16, [1] + [0] * 15,
            [top if c % 2 else 0 for c in range(16)], [0 if c % 2 else top for c in range(16)]]
    ops += [[du.R16_TIGHT if c == k else 0 for c in range(16)] for k in range(16)]
    ops += [du.r16_digits(v) for v in (P - 1, P, P + 1, 2 * P, 2**255 - 1, 2**256 - 1, 15 * P, 16 * P - 1)]
    assert all(0 <= min(x) and max(x) < du.R16_IN for x in ops)
    return ops


def check_r16_rows(ctx, xs, out, wants):
    for x, o, want in zip(xs, out, wants):
        l = [int(v) for v in o[:16]]
        assert du.r16_val(l) == want, (ctx, x, l)
        assert all(v <= m for v, m in zip(l, du.R16_OUT_MAX)), (ctx, x, l)
        assert [int(v) for v in o[16:24]] == du.canonical_words(want), (ctx, x)     # r16_digits / r16_words
        assert int(o[24]) == (want == 0), (ctx, x)                                  # r16_iszero


def test_r16_mul_sq(diag):
    rng = random.Random(65)
    fs = r16_operands(rng)
    gs = fs[7:] + fs[:7]
    pairs = list(zip(fs, gs)) + [(f, g) for f in fs[360:368] for g in fs[360:368]]
    out = diag.run("r16", "mul", [f + g for f, g in pairs])
    check_r16_rows("mul", pairs, out, [du.r16_val(f) * du.r16_val(g) % P for f, g in pairs])
    out = diag.run("r16", "sq", fs)
    check_r16_rows("sq", fs, out, [du.r16_val(f) ** 2 % P for f in fs])
    # one row of four alone in its wave, and a count that is no multiple of four
    for n in (1, 2, 3, 5):
        out = diag.run("r16", "mul", [f + g for f, g in pairs[:n]])
        check_r16_rows("mul", pairs[:n], out, [du.r16_val(f) * du.r16_val(g) % P for f, g in pairs[:n]])
    print(f"r16_mul: {len(pairs)} cases, r16_sq: {len(fs)} cases")


def iszero_cases():
    rng = random.Random(66)
    xs = []
    for k in range(16):
        xs += du.r16_splits(k * P, rng, 4)                 # k p in four limb splits below 2^19
        for d in (-1, 1):
            if k * P + d >= 0:
                xs += du.r16_splits(k * P + d, rng, 2)
    for j in list(range(1, 9)) + [2**15, 2**16 - 1]:
        for s in (-1, 1):
            xs += du.r16_splits(P + s * (j << 16), rng, 2)
    xs += [[rng.randrange(du.R16_IN) for _ in range(16)] for _ in range(200)]
    xs += [[du.R16_IN - 1] * 16, [0] * 16]
    return xs


def test_r16_iszero_and_digits(diag):
    xs = iszero_cases()
    out = diag.run("r16", "ident", xs)
    zeros = 0
    for x, o in zip(xs, out):
        want = du.r16_val(x)
        assert [int(v) for v in o[:16]] == x
        assert int(o[24]) == (want == 0), (x, du.r16_int(x) // P, du.r16_int(x) % P)
        assert [int(v) for v in o[16:24]] == du.canonical_words(want), x
        zeros += want == 0
    assert zeros >= 64
    print(f"r16_iszero / r16_digits: {len(xs)} cases, {zeros} multiples of p")


def test_r16_from_fe(diag):
    rng = random.Random(67)
    fs = du.fe_random(rng, 200, du.B33) + du.fe_extremes(du.B33) + du.fe_special_reps(du.B33)
    out = diag.run("r16", "from_fe", fs)
    for f, o in zip(fs, out):
        want = du.fe_val(f)
        assert [int(v) for v in o[:16]] == [(want >> (16 * c)) & 0xffff for c in range(16)], f
        assert int(o[24]) == (want == 0), f
    print(f"r16_from_fe: {len(fs)} cases")


def test_r16_pow22523(diag):
    rng = random.Random(68)
    zs = [1, 2, P - 1, du.SQRTM1, 0, 3] + [rng.randrange(P) for _ in range(40)]
    xs = [du.r16_digits(z) for z in zs] + [du.r16_random_tight(rng) for _ in range(40)]
    xs += [[du.R16_TIGHT] * 16, [du.R16_IN - 1] * 16]
    out = diag.run("r16", "pow22523", xs)
    check_r16_rows("pow22523", xs, out, [pow(du.r16_val(x), 2**252 - 3, P) for x in xs])
    print(f"r16_pow22523: {len(xs)} cases")
