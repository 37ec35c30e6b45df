"""From received shreds to a checked proof-of-history chain, every stage on the
GPU: the capture's 480 shreds with half of every FEC set erased ->
fec_recover_host -> fec_seal_host without keys -> shreds_host under the
leader's key (480 zeros) -> the data shreds' payloads laid end to end ->
poh_blocks_host and poh_host."""
import struct

import numpy as np
import pytest

import poh_model as model
import poh_util as util
import recover_util
from shred_util import fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from firedancer_amd import ed25519
    e = ed25519.Engine(0, max_chunk=512, compact=True)
    yield e
    e.close()


def test_recovered_shreds_carry_a_chain_that_verifies(eng):
    cases = recover_util.captured("mixed")
    codes, sets = eng.fec_recover_host([st for _, st, _ in cases], [m for m, _, _ in cases])
    assert not codes.any()
    codes, sets, _, _ = eng.fec_seal_host(sets, None)
    assert not codes.any()
    shreds = [s for st in sets for s in st]
    assert len(shreds) == 480
    codes, _ = eng.shreds_host(shreds, fixture()[1])
    assert codes.tolist() == [0] * 480
    data = sorted((struct.unpack_from("<I", s, 0x49)[0], bytes(s[0x58:struct.unpack_from("<H", s, 0x56)[0]]))
                  for s in shreds if s[0x40] & 0xF0 == 0x80)
    block = b"".join(p for _, p in data)
    assert block == util.captured_block()

    # the capture's first microblock chains from the zero hash; a caller who does not know a block's true
    # predecessor learns so at microblock 0
    last_hdr = model.walk(block)[1][-1]
    codes, first_bad, last = eng.poh_blocks_host([block, block], [bytes(32), b"\x5a" * 32])
    assert codes.tolist() == [0, model.ERR_HASH] and first_bad.tolist() == [0xFFFFFFFF, 0]
    assert last[0].tobytes() == last[1].tobytes() == block[last_hdr + 8:last_hdr + 40]

    d = util.captured()
    rest = util.Desc(d.buf, d.hdr_off[1:], d.in_off[1:], d.sig_first[1:] - d.sig_first[1], d.sig_off[d.sig_first[1]:])
    codes, states = eng.poh_host(*rest.args())
    assert codes.tolist() == [0] * 63
    assert np.array_equal(states, np.array([np.frombuffer(d.buf[int(h) + 8:int(h) + 40], np.uint8) for h in rest.hdr_off]))
