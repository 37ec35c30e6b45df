"""GPU: the leader signatures of Merkle shreds (fd_ed25519_hip_shreds_host /
_dev, include/fd_ed25519_hip.h Part 2c) against the test-side model of the
resolver's rules (shred_model.judge: hashlib and the reference's compiled
verify).  A small engine: compact tables, 512-signature chunks."""
import numpy as np
import pytest

import shred_model as model
from shred_util import Leader, every_depth, fixture, mutated, rule_cases

pytestmark = pytest.mark.gpu

MAX_CHUNK = 512


@pytest.fixture(scope="module")
def ed():
    from firedancer_amd import ed25519
    return ed25519


@pytest.fixture(scope="module")
def eng(ed):
    e = ed.Engine(0, max_chunk=MAX_CHUNK, compact=True)
    yield e
    e.close()


class Pool:
    """shreds with their leader keys and the model's verdicts, computed once"""

    def __init__(self, oracle):
        verify = model.verifier(oracle)
        self.shreds, self.keys, self.names = [], [], []
        fx, fx_pub = fixture()
        cases, case_pub = rule_cases(oracle)
        deep, deep_pub = every_depth(oracle)
        self.add("fixture", fx, fx_pub)
        self.add("case", [s for _, s, _ in cases], case_pub, [n for n, _, _ in cases])
        self.add("depth", deep, deep_pub)
        self.add("mutation", mutated()[:600], fx_pub)
        judged = [model.judge(verify, s, k) for s, k in zip(self.shreds, self.keys)]
        self.codes = np.array([c for c, _ in judged], np.int8)
        self.roots = np.array([list(r) if r else [0] * 32 for _, r in judged], np.uint8)

    def add(self, kind, shreds, pub, names=None):
        self.names += [f"{kind}:{names[i] if names else i}" for i in range(len(shreds))]
        self.shreds += list(shreds)
        self.keys += [pub] * len(shreds)

    def of(self, kind):
        return [i for i, n in enumerate(self.names) if n.startswith(kind + ":")]


@pytest.fixture(scope="module")
def pool(oracle):
    return Pool(oracle)


def check_host(eng, pool, pick):
    codes, roots = eng.shreds_host([pool.shreds[i] for i in pick], [pool.keys[i] for i in pick])
    bad = np.nonzero(codes != pool.codes[pick])[0]
    assert len(bad) == 0, [(pool.names[pick[i]], int(codes[i]), int(pool.codes[pick[i]])) for i in bad[:10]]
    bad = np.nonzero((roots != pool.roots[pick]).any(axis=1))[0]
    assert len(bad) == 0, [pool.names[pick[i]] for i in bad[:10]]


def test_fixture_shreds(eng, pool):
    """the reference's 480 captured shreds: all accepted, the model's roots"""
    pick = pool.of("fixture")
    assert len(pick) == 480 and not pool.codes[pick].any() and len({bytes(r) for r in pool.roots[pick]}) == 7
    check_host(eng, pool, pick)


def test_rule_edges(eng, pool, oracle):
    pick = pool.of("case")
    want = np.array([w for _, _, w in rule_cases(oracle)[0]], np.int8)
    assert (pool.codes[pick] == want).all()      # every builder-signed case verifies in the model
    check_host(eng, pool, pick)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_batch_sizes(eng, pool, n):
    """around the stage kernel's 64-lane blocks and the finish kernel's 256"""
    src = pool.of("case") + pool.of("fixture")
    check_host(eng, pool, [src[(7 * i + 3 * n) % len(src)] for i in range(n)])


def test_mixed_batch_spans_three_chunks(eng, pool):
    pick = (pool.of("fixture") + pool.of("case") + pool.of("depth") + pool.of("mutation"))[:1100]
    rng = np.random.default_rng(53)
    pick = [pick[i] for i in rng.permutation(len(pick))]
    assert len(pick) == 1100 > 2 * MAX_CHUNK
    assert set(pool.codes[pick].tolist()) == {0, model.ERR_PARSE, model.UNSUPPORTED, model.ERR_HEADER, model.ERR_SIGNATURE}
    check_host(eng, pool, pick)


def test_only_rejected_shreds(eng, pool):
    pick = [i for i in range(len(pool.codes)) if pool.codes[i] in (model.ERR_PARSE, model.ERR_HEADER)][:200]
    assert len(pick) == 200 and not pool.roots[pick].any()
    check_host(eng, pool, pick)


def test_only_unsupported_shreds(eng, pool):
    pick = [i for i in range(len(pool.codes)) if pool.codes[i] == model.UNSUPPORTED]
    assert len(pick) >= 40
    check_host(eng, pool, pick)


def test_every_tree_depth(eng, pool):
    pick = pool.of("depth")
    assert len(pick) == 31 and not pool.codes[pick].any()
    check_host(eng, pool, pick)


def run_dev(eng, ed, shreds, keys, roots=True, sig_out=True, spread=False):
    """fd_ed25519_hip_shreds_dev on device-resident inputs -> (out, roots,
    sig_out); spread: shred i starts at byte i mod 16 of a 16-byte line"""
    n, buf, off = len(shreds), bytearray(), []
    for i, s in enumerate(shreds):
        if spread:
            buf += bytes((i - len(buf)) % 16)
        off.append(len(buf))
        buf += s
    d_buf = eng.alloc(len(buf) + 16).upload(np.frombuffer(bytes(buf) + bytes(16), np.uint8))   # readable 16 bytes past
    d_off = eng.alloc(8 * n).upload(np.array(off, np.uint64))
    d_sz = eng.alloc(4 * n).upload(np.array([len(s) for s in shreds], np.uint32))
    d_keys = eng.alloc(32 * n).upload(np.frombuffer(b"".join(keys), np.uint8))
    d_work = eng.alloc(ed.shred_work_bytes(n))
    d_out = eng.alloc(n + 8).upload(np.full(n + 8, 0x55, np.int8))
    d_roots = eng.alloc(32 * (n + 1)).upload(np.full(32 * (n + 1), 0x55, np.uint8))
    d_sig = eng.alloc(n + 8).upload(np.full(n + 8, 0x55, np.int8))
    assert d_work.ptr % 16 == 0 and d_buf.ptr % 16 == 0 and d_keys.ptr % 16 == 0
    eng.shreds_dev(n, d_buf.ptr, d_off.ptr, d_sz.ptr, d_keys.ptr, d_work.ptr, d_out.ptr, d_roots.ptr if roots else None,
                   d_sig.ptr if sig_out else None)
    eng.sync()
    got = d_out.download(np.int8, n + 8), d_roots.download(np.uint8, 32 * (n + 1)), d_sig.download(np.int8, n + 8)
    for b in (d_buf, d_off, d_sz, d_keys, d_work, d_out, d_roots, d_sig):
        b.free()
    # nothing written past the n results, and nothing at all into an output that was not given
    assert (got[0][n:] == 0x55).all() and (got[1][32 * n if roots else 0:] == 0x55).all()
    assert (got[2][n if sig_out else 0:] == 0x55).all()
    return got[0][:n], got[1][:32 * n].reshape(n, 32), got[2][:n]


def test_every_byte_offset(eng, ed, pool):
    """shreds starting at bytes 0..15 of a 16-byte line, every kind among them"""
    pick = (pool.of("depth") + pool.of("case") + pool.of("fixture")[:40] + pool.of("mutation")[:60])
    out, roots, _ = run_dev(eng, ed, [pool.shreds[i] for i in pick], [pool.keys[i] for i in pick], spread=True)
    assert (out == pool.codes[pick]).all() and (roots == pool.roots[pick]).all()


def test_shreds_dev_without_optional_outputs(eng, ed, pool):
    pick = pool.of("fixture")[:70] + pool.of("case")
    shreds, keys = [pool.shreds[i] for i in pick], [pool.keys[i] for i in pick]
    out, _, _ = run_dev(eng, ed, shreds, keys, roots=False, sig_out=False)
    assert (out == pool.codes[pick]).all()
    out, roots, sig = run_dev(eng, ed, shreds, keys)
    assert (out == pool.codes[pick]).all() and (roots == pool.roots[pick]).all()
    assert (sig[pool.codes[pick] != model.ERR_SIGNATURE] == 0).all()


def test_verify_level_rejects(eng, ed, oracle, adversarial):
    """S >= L, a small-order key, an undecodable R as a shred's signature and
    leader: ERR_SIGNATURE each, sig_out the reference's own code (none of
    these depends on the message)"""
    d, ld = adversarial, Leader(oracle, 59)
    shreds, keys, want_sig = [], [], []
    for tag in ("S_plus_L", "A_small_order", "R_undecodable"):
        rows = [i for i in np.nonzero(d["tags"] == tag)[0] if d["codes_avx512"][i] not in (0, -3)][:3]
        assert len(rows) == 3, tag
        for i in rows:
            s = bytearray(ld.shred(bool(i & 1), 6, 3))
            s[:64] = d["sigs"][i].tobytes()
            code, root = model.root(bytes(s))
            assert code == 0
            ref = oracle.oracle_ed25519_verify(root, 32, bytes(s[:64]), d["pubs"][i].tobytes(), 0)
            assert ref == d["codes_avx512"][i]
            shreds.append(bytes(s))
            keys.append(d["pubs"][i].tobytes())
            want_sig.append(ref)
    valid = ld.shred(True, 6, 3)
    shreds.append(valid)
    keys.append(ld.pub)
    want_sig.append(0)
    out, roots, sig = run_dev(eng, ed, shreds, keys)
    assert out.tolist() == [model.ERR_SIGNATURE] * 9 + [0] and sig.tolist() == want_sig
    assert all(bytes(r) == model.root(s)[1] for r, s in zip(roots, shreds))


def test_wrong_leader_key(eng, oracle):
    a, b = Leader(oracle, 61), Leader(oracle, 67)
    s = a.shred(False, 7, 5)
    codes, roots = eng.shreds_host([s, s, s], [a.pub, b.pub, a.pub])
    assert codes.tolist() == [0, model.ERR_SIGNATURE, 0]
    assert all(bytes(r) == model.root(s)[1] for r in roots)


def test_one_key_for_all_and_an_empty_batch(eng, pool):
    shreds, pub = fixture()
    codes, roots = eng.shreds_host(shreds[:5], pub)
    assert not codes.any() and (roots == pool.roots[:5]).all()
    codes, roots = eng.shreds_host([], [])
    assert len(codes) == 0 and roots.shape == (0, 32)
