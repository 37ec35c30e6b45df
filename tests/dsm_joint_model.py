"""Plain-integer restatement of the half-size dsm loop's joint form
(fd_ed25519_kernels.hip, dsm_half_one): c and |d| in signed 2-bit windows,
one addition per window from a 12-slot lane table of a A' + r R'.  Test
infrastructure, no product code.

  digits   x << (160 - 2 W2), recode160<2>: digits in [-2, 1], popped from
           the top, the first one read unsigned (& 3, in [0, 2])
  W2       max(66, ceil((bits(|d|) + 1) / 2)), at most 76
  class    the pair (a, r) up to the common sign s = (a < 0 or (a == 0 and
           r < 0)): (a', r') with a' in {0, 1, 2}, r' in [-2, 2]
  slot     5 a' + r' - 1, 0..11; (0, 0) is the shared identity (-1 here)"""
import dsm_model as dm

W2_MIN, W2_MAX = 66, 76


def w2_of(dmag):
    return max(W2_MIN, (dmag.bit_length() + 2) >> 1)


def digits2(x, w2):
    """the w2 digits of x < 2^(2 w2 - 1), most significant first, as the
    device pops them (160-bit recoding, the top one & 3)"""
    assert 0 <= x < 1 << (2 * w2 - 1) and W2_MIN <= w2 <= W2_MAX
    v = x << (160 - 2 * w2)
    assert v < 1 << 160
    out, carry = [], 0
    for q in range(80):
        e = ((v >> (2 * q)) & 3) + carry
        carry = (e + 2) >> 2
        e -= carry << 2
        out.append(e)
    out[79] &= 3
    assert all(e == 0 for e in out[:80 - w2])
    return out[:79 - w2:-1]


def normalise(a, r):
    """(a, r) -> (s, a', r')"""
    s = a < 0 or (a == 0 and r < 0)
    return (1, -a, -r) if s else (0, a, r)


def slot(a, r):
    return 5 * a + r - 1


def windows(c, dmag, w2=None):
    """per window, most significant first: (s, a', r')"""
    w2 = w2 or w2_of(dmag)
    return [normalise(a, r) for a, r in zip(digits2(c, w2), digits2(dmag, w2))]


def possible_classes():
    """what the digit ranges admit: top pairs in [0, 2]^2, the others in
    [-2, 1]^2; {(a', r'): set of "top" / "low"}"""
    out = {}
    for where, rng in (("top", range(0, 3)), ("low", range(-2, 2))):
        for a in rng:
            for r in rng:
                _, an, rn = normalise(a, r)
                out.setdefault((an, rn), set()).add(where)
    return out


def build_table(A1, R1):
    """the device's build order on extended points: {slot: point}; the class
    (1, -2) stored as the negative of 2R' - A'"""
    xadd, xdbl, xneg = dm.xadd, dm.xdbl, dm.xneg
    t = {slot(1, 0): A1, slot(0, 1): R1}
    R2 = xdbl(R1)
    t[slot(0, 2)] = R2
    t[slot(1, 2)] = xadd(R2, A1)
    t[slot(1, -2)] = xneg(xadd(R2, xneg(A1)))
    t[slot(1, 1)] = xadd(A1, R1)
    t[slot(1, -1)] = xadd(A1, xneg(R1))
    A2 = xdbl(A1)
    t[slot(2, 0)] = A2
    t[slot(2, 1)] = xadd(A2, R1)
    t[slot(2, -1)] = xadd(A2, xneg(R1))
    t[slot(2, 2)] = xadd(t[slot(2, 1)], R1)
    return t


def joint_sum(c, dmag, A1, R1, w2=None):
    """[c]A1 + [dmag]R1 as the loop evaluates it"""
    tab = build_table(A1, R1)
    acc = None
    for s, a, r in windows(c, dmag, w2):
        e = dm.XIDENT if (a, r) == (0, 0) else tab[slot(a, r)]
        e = dm.xneg(e) if s else e
        acc = e if acc is None else dm.xadd(dm.xdbl(dm.xdbl(acc)), e)
    return acc
