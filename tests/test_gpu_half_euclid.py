"""The half-size scalar search on the device against the big-integer Euclid
of tests/half_euclid_model.py (through the diagnostic
fd_ed25519_hip_diag_half_scalars, whose pairs have also passed the kernel's
integer re-check), at batch sizes below, at and above one wave and one
block, with lanes that take the even-t fix-up beside lanes that do not and
one lane with a quotient of 2^30 among ordinary ones, so that the wave runs
every path; then whole verifications of the fixtures without a strict pair,
with a long d, and of random signatures, under the default and the strict
bound."""
import numpy as np
import pytest

import half_euclid_model as hm
from conftest import oracle_many
from test_gpu_parity import _random_set

pytestmark = pytest.mark.gpu

MODES = {"extended": 151, "strict": 131}


@pytest.fixture(scope="module", params=list(MODES))
def engine(request):
    from firedancer_amd import ed25519
    e = ed25519.Engine(0, max_chunk=1 << 12, half=request.param)
    yield e, MODES[request.param]
    e.close()


@pytest.fixture(scope="module")
def pool():
    """257 k: a random one, a 2^30 quotient (the 24th of the expansion, in
    the second round), then longd.npz, and shares of halfsize.npz,
    adversarial.npz, mixed_order.npz and random k in turn"""
    big = next(k for k, pos, q in hm.big_quotient_ks() if pos == 23 and q == 2**30)
    assert 2**30 in hm.pair(big)[2]
    rnd = hm.random_ks(200, seed=77)
    fx = [hm.fixture_ks((nm,)) for nm in ("halfsize", "adversarial", "mixed_order")]
    ks = [rnd[0], big] + hm.fixture_ks(("longd",))
    i = 0
    while len(ks) < 257:
        ks += [fx[0][i], fx[1][7 * i], fx[2][31 * i], rnd[1 + i]]
        i += 1
    return ks[:257]


def check(engine, ks):
    e, dbits = engine
    out = e.diag_half_scalars(hm.k_array(ks))
    assert out.shape == (len(ks), 12)
    n_found = 0
    for k, o in zip(ks, out):
        c, d = hm.pair_cd(k)
        f = hm.found(c, d, dbits)
        got_f, got_c, got_d = hm.unpack(o)
        assert got_f == f, (hex(k), dbits, got_f, f)
        if f:
            n_found += 1
            assert (got_c, got_d) == (c, d), (hex(k), dbits)
    return n_found


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_device_pairs(engine, pool, n):
    ks = pool[:n]
    if n >= 63:
        fix = [hm.takes_fixup(k) for k in ks[:63]]
        assert any(fix) and not all(fix)            # both kinds of lane in the first wave
        assert 2**30 in hm.pair(ks[1])[2]           # and the lane that leaves the fused update
    assert check(engine, ks) > 0 or n == 1


def test_device_pairs_all_fixture_k(engine):
    ks = hm.fixture_ks() + hm.quotient_edge_ks() + hm.golden_ratio_ks() + [k for k, _, _ in hm.big_quotient_ks()]
    assert check(engine, ks) > 0.9 * len(ks)


def test_verify_codes(engine, oracle, halfsize, longd):
    e, _ = engine
    rnd = _random_set(oracle, 3000, seed=41)
    for name, d, want in (("halfsize", halfsize, halfsize["codes_avx512"]), ("longd", longd, longd["codes_avx512"]),
                          ("random", rnd, oracle_many(oracle, rnd, 0))):
        got = e.verify_host(d["msgs"], d["msg_off"], d["msg_sz"], d["sigs"], d["pubs"])
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (name, [(int(i), int(got[i]), int(want[i])) for i in bad[:8]])
