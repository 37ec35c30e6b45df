"""GPU: the Ed25519 precompile instructions of raw transactions
(fd_ed25519_hip_precompile_host / _dev, include/fd_ed25519_hip.h Part 2b)
against the test-side model of fd_precompile_ed25519_verify
(precompile_model.judge: the reference's compiled parser and verify).  A
small engine: compact tables, 512-signature chunks."""
import random

import numpy as np
import pytest

import precompile_model as model
from precompile_util import Builder, max_entries_txn, rule_cases
from txn_util import Signer, ref_lib

pytestmark = pytest.mark.gpu

MAX_CHUNK = 512


@pytest.fixture(scope="module")
def ref():
    lib = ref_lib()
    if lib is None:
        pytest.skip("oracle/_ref not built")
    return lib


@pytest.fixture(scope="module")
def ed():
    from firedancer_amd import ed25519
    return ed25519


@pytest.fixture(scope="module")
def eng(ed):
    e = ed.Engine(0, max_chunk=MAX_CHUNK, compact=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases(oracle, ref):
    """the rule-edge transactions with the model's verdicts, computed once"""
    c = rule_cases(oracle)
    return [n for n, _ in c], [p for _, p in c], [model.judge(ref, p) for _, p in c]


def expect(judged):
    return np.array([j[0] for j in judged], np.int8), np.array([j[1] for j in judged], np.uint8)


def assert_same(got, want, names=None):
    for g, w in zip(got, want):
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, [(int(i), names[i] if names else "", int(g[i]), int(w[i])) for i in bad[:10]]


def test_rule_edges(eng, cases):
    """every rule-edge case (tests/test_precompile_plan.py pins what each reaches), one batch"""
    names, payloads, judged = cases
    assert_same(eng.precompile_host(payloads), expect(judged), names)
    want = dict(zip(names, judged))
    # priority: entry order inside an instruction, instruction order across them
    assert want["prio_sig_then_offset"][:2] == (-3, 0) and want["prio_offset_then_sig"][:2] == (-4, 0)
    assert want["prio_second_instr_fails"][:2] == (-3, 2) and want["prio_both_instr_fail"][:2] == (-3, 0)


@pytest.mark.parametrize("ntxn", [1, 256, 257])
def test_batch_sizes(eng, cases, ntxn):
    """one transaction, a full stage block's multiple and one more"""
    names, payloads, judged = cases
    pick = [(7 * i + 13) % len(payloads) for i in range(ntxn)]
    assert_same(eng.precompile_host([payloads[i] for i in pick]), expect([judged[i] for i in pick]),
                [names[i] for i in pick])


def test_verify_level_rejects(eng, ref, oracle, adversarial):
    """S >= L, a small-order key, an undecodable R, a non-canonical key: each
    ERR_SIGNATURE whatever fd_ed25519_verify's own code; the valid twin 0."""
    d, sg, payloads, tags = adversarial, Signer(oracle, 23), [], []
    for tag in ("valid", "S_plus_L", "A_small_order", "R_undecodable", "A_noncanonical"):
        rows = [i for i in np.nonzero(d["tags"] == tag)[0] if d["msg_sz"][i] <= 700 and d["codes_avx512"][i] != -3][:3]
        assert len(rows) == 3, tag
        for i in rows:
            off, sz = int(d["msg_off"][i]), int(d["msg_sz"][i])
            b = Builder(sg)
            b.add_inline([(d["sigs"][i].tobytes(), d["pubs"][i].tobytes(), d["msgs"][off:off + sz].tobytes())])
            payloads.append(b.build())
            tags.append(tag)
    judged = [model.judge(ref, p) for p in payloads]
    assert [j[0] for j in judged] == [0 if t == "valid" else -3 for t in tags]
    assert_same(eng.precompile_host(payloads), expect(judged), tags)


def test_no_precompile_instruction_at_all(eng, oracle, ref):
    sg = Signer(oracle, 29)
    payloads = []
    for i in range(70):
        b = Builder(sg, v0=bool(i & 1))
        b.add(bytes(i % 40), prog=2)
        payloads.append(b.build())
    from firedancer_amd import ed25519 as ed
    assert sum(ed.precompile_count(p) for p in payloads) == 0
    assert all(model.judge(ref, p)[:2] == (0, 0xFF) for p in payloads)
    codes, instr = eng.precompile_host(payloads)
    assert not codes.any() and (instr == 0xFF).all()


def test_only_rejected_payloads(eng, cases, ref):
    _, payloads, _ = cases
    bad = [p + b"\x00" for p in payloads[:40]] + [b"", b"\x01", payloads[0][:50]]
    assert all(model.walk(ref, p) is None for p in bad)
    codes, instr = eng.precompile_host(bad)
    assert (codes == model.PARSE_FAILED).all() and (instr == 0xFF).all()


def test_most_entries_of_one_payload(eng, ed, oracle, ref):
    """the most entries a 1232-byte payload carries (more than the 64 an
    instruction table has rows), all aliasing one signature, key and message;
    and the same with the last entry's message one byte longer than the data"""
    payload, n = max_entries_txn(oracle)
    assert n > 64 and ed.precompile_count(payload) == n
    cut = bytearray(payload)
    cut[-97 - 14 + 10] += 1          # the last entry's msg_data_sz
    judged = [model.judge(ref, payload), model.judge(ref, bytes(cut))]
    assert [j[:2] for j in judged] == [(0, 0xFF), (-4, 0)] and len(judged[1][2]) == n
    assert_same(eng.precompile_host([payload, bytes(cut)]), expect(judged))


@pytest.fixture(scope="module")
def mixed(oracle, ref):
    """about 300 transactions of 0..9 distinct-key entries in one or two
    precompile instructions, a fifth of them corrupted"""
    rng, sg, payloads = random.Random(31), Signer(oracle, 31), []
    for t in range(300):
        n = rng.randrange(10)
        b = Builder(sg, v0=rng.random() < 0.3 and n <= 6, accts=[model.ED25519_ID])   # nine entries fill a legacy payload
        hurt = rng.randrange(6) if rng.random() < 0.2 else -1
        trip = [b.signed(bytes(rng.getrandbits(8) for _ in range(rng.randrange(1, 4 if n > 6 else 40))),
                         flip=(hurt == 0 and i == n // 2)) for i in range(n)]
        split = rng.randrange(n + 1) if n and rng.random() < 0.4 else n
        for part in (trip[:split], trip[split:]):
            if part:
                b.add_inline(part)
        if hurt == 1 and b.instrs:      # a signature offset past the data
            prog, a, data = b.instrs[-1]
            b.instrs[-1] = (prog, a, data[:2] + b"\xff\x7f" + data[4:])
        if hurt == 2 and b.instrs:      # a key looked up in an instruction that is not there
            prog, a, data = b.instrs[0]
            b.instrs[0] = (prog, a, data[:8] + b"\x40\x00" + data[10:])
        if hurt == 3 and b.instrs:      # one more entry than the data holds
            prog, a, data = b.instrs[0]
            b.instrs[0] = (prog, a, bytes([200]) + data[1:])
        if hurt == 4:
            b.add(bytes(3))             # a header that fails behind everything else
        p = b.build()
        payloads.append(p + b"\x00" if hurt == 5 else p)
    assert max(len(p) for p in payloads) <= 1233
    judged = [model.judge(ref, p) for p in payloads]
    seen = {j[0] for j in judged}
    assert seen == {0, -3, -4, -5, model.PARSE_FAILED}, seen
    assert sum(j[0] == 0 for j in judged) > 200
    return payloads, judged


def test_mixed_batch_spans_chunks(eng, ed, mixed):
    payloads, judged = mixed
    assert sum(ed.precompile_count(p) for p in payloads) > 2 * MAX_CHUNK
    assert_same(eng.precompile_host(payloads), expect(judged))


def run_dev(eng, ed, payloads, ent_first):
    """fd_ed25519_hip_precompile_dev on device-resident inputs -> (txn_out, instr_out, ent_out)"""
    from firedancer_amd.tile import pack_payloads
    buf, off, sz = pack_payloads(payloads)
    ntxn, n_ent = len(payloads), int(ent_first[-1])
    d_buf = eng.alloc(len(buf) + 16).upload(buf)       # readable 16 bytes past the last payload
    d_off, d_sz = eng.alloc(8 * ntxn).upload(off), eng.alloc(4 * ntxn).upload(sz)
    d_first = eng.alloc(4 * (ntxn + 1)).upload(np.asarray(ent_first, np.uint32))
    d_work = eng.alloc(ed.precompile_work_bytes(ntxn, n_ent))
    d_txn, d_instr = eng.alloc(ntxn).upload(np.full(ntxn, 0x55, np.int8)), eng.alloc(ntxn).upload(np.zeros(ntxn, np.uint8))
    d_ent = eng.alloc(n_ent + 8).upload(np.full(n_ent + 8, 0x55, np.int8))
    assert d_work.ptr % 16 == 0
    eng.precompile_dev(ntxn, d_buf.ptr, d_off.ptr, d_sz.ptr, d_first.ptr, n_ent, d_work.ptr, d_txn.ptr, d_instr.ptr,
                       d_ent.ptr)
    eng.sync()
    out = d_txn.download(np.int8, ntxn), d_instr.download(np.uint8, ntxn), d_ent.download(np.int8, n_ent + 8)
    for b in (d_buf, d_off, d_sz, d_first, d_work, d_txn, d_instr, d_ent):
        b.free()
    assert (out[2][n_ent:] == 0x55).all()              # nothing written past the entries
    return out[0], out[1], out[2][:n_ent]


def test_precompile_dev_direct(eng, ed, mixed):
    """the device entry point on its own: the same codes, and ent_out per entry"""
    payloads, judged = mixed
    first = np.concatenate([[0], np.cumsum([ed.precompile_count(p) for p in payloads])])
    txn, instr, ent = run_dev(eng, ed, payloads, first)
    assert_same((txn, instr), expect(judged))
    want_ent = np.array([c for j in judged for c in j[2]], np.int8)
    assert len(want_ent) == first[-1]
    assert_same((ent,), (want_ent,))


def test_reservation_one_too_small(eng, ed, mixed):
    """one transaction's reservation an entry short: BAD_RESERVATION for it
    alone, every slot of it marked, its neighbours' codes unchanged"""
    payloads, judged = mixed
    cnt = np.array([ed.precompile_count(p) for p in payloads])
    t = int(np.nonzero((cnt >= 2) & (np.array([j[0] for j in judged]) == 0))[0][5])
    cnt[t] -= 1
    first = np.concatenate([[0], np.cumsum(cnt)])
    txn, instr, ent = run_dev(eng, ed, payloads, first)
    want_txn, want_instr = expect(judged)
    want_txn[t], want_instr[t] = model.BAD_RESERVATION, 0xFF
    assert_same((txn, instr), (want_txn, want_instr))
    want_ent = np.array([c for i, j in enumerate(judged)
                         for c in ([model.BAD_RESERVATION] * int(cnt[t]) if i == t else j[2])], np.int8)
    assert_same((ent,), (want_ent,))
