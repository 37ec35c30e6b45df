"""Python mirror of the reference's ed25519 verify interface, backed by the
MI355X library libfd_ed25519_hip (C-ABI, include/fd_ed25519_hip.h).

Mirrors src/ballet/ed25519/fd_ed25519.h:96-138 of tigarcia/firedancer:

    verify(msg, sig, public_key)                    -> fd_ed25519_verify
    verify_batch_single_msg(msg, signatures, pubs)  -> fd_ed25519_verify_batch_single_msg
    strerror(err)                                   -> fd_ed25519_strerror

with the same argument meaning and return codes (SUCCESS 0, ERR_SIG -1,
ERR_PUBKEY -2, ERR_MSG -3), plus the batch Engine the verify tile and
bench.py drive.  There is no CPU fallback: importing this module without the
built library raises.
"""
import ctypes
import os

import numpy as np

SUCCESS = 0
ERR_SIG = -1
ERR_PUBKEY = -2
ERR_MSG = -3

FLAG_CODES_PORTABLE = 1
FLAG_HALF_STRICT = 2     # half-size |d| < 2^131 only (full-length form for the rest): tests / A-B
FLAG_DSM_QUAD = 4        # dsm with a quad of lanes per signature at every chunk size
FLAG_DSM_WIDE = 8        # dsm with one lane per signature at every chunk size
FLAG_DSM_OCT = 16        # dsm with two quads of lanes per signature at every chunk size
FLAG_ONE_STREAM = 32     # no decode side stream / second lane: for engines whose batches overlap one another
FLAG_NO_OVERLAP = 64     # a large chunk's phases in sequence (no decode side stream): tests / A-B
FLAG_NO_PIPELINE = 128   # a multi-chunk call on one set of work arrays (no second lane): tests / A-B
FLAG_COMPACT_TABLES = 256  # radix-2^16 base tables (2 x 8 MiB, shared) instead of radix 2^24 (2 x 2 GiB)
FLAG_DSM_R16 = 512       # dsm16 (field arithmetic over 16 lanes, two waves per signature) at every chunk size

# phases of a verify launch (FD_ED25519_HIP_PHASE_CNT, include/fd_ed25519_hip.h)
PHASES = ("hash", "scalar", "decode", "dsm")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FD_ED25519_HIP_LIB", os.path.join(_HERE, "_lib", "libfd_ed25519_hip.so"))

if not os.path.exists(LIB_PATH):
    raise ImportError(f"libfd_ed25519_hip not built: {LIB_PATH} missing "
                      "(run `python -c 'import __graft_entry__ as g; g.build()'`); there is no CPU fallback")

_lib = ctypes.CDLL(LIB_PATH, use_errno=True)   # errno: shlink create / join report why they failed

_u8p = ctypes.c_void_p
_lib.fd_ed25519_verify.argtypes = [ctypes.c_char_p, ctypes.c_ulong, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p]
_lib.fd_ed25519_verify.restype = ctypes.c_int
_lib.fd_ed25519_verify_batch_single_msg.argtypes = [ctypes.c_char_p, ctypes.c_ulong, ctypes.c_char_p, ctypes.c_char_p,
                                                    ctypes.c_void_p, ctypes.c_ubyte]
_lib.fd_ed25519_verify_batch_single_msg.restype = ctypes.c_int
_lib.fd_ed25519_strerror.argtypes = [ctypes.c_int]
_lib.fd_ed25519_strerror.restype = ctypes.c_char_p
_lib.fd_ed25519_hip_engine_new.argtypes = [ctypes.c_int, ctypes.c_ulong, ctypes.c_int]
_lib.fd_ed25519_hip_engine_new.restype = ctypes.c_void_p
_lib.fd_ed25519_hip_engine_delete.argtypes = [ctypes.c_void_p]
_lib.fd_ed25519_hip_engine_set_forms.argtypes = [ctypes.c_void_p, ctypes.c_ulong, ctypes.c_ulong]
_lib.fd_ed25519_hip_engine_set_r16_max.argtypes = [ctypes.c_void_p, ctypes.c_ulong]
_lib.fd_ed25519_hip_engine_stream.argtypes = [ctypes.c_void_p]
_lib.fd_ed25519_hip_engine_stream.restype = ctypes.c_void_p
_lib.fd_ed25519_hip_engine_sync.argtypes = [ctypes.c_void_p]
_lib.fd_ed25519_hip_verify_dev.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 7
_lib.fd_ed25519_hip_txn_combine_dev.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 5
_lib.fd_ed25519_hip_verify_host.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 6
_lib.fd_ed25519_hip_verify_txns_host.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 9
_lib.fd_ed25519_hip_sign_dev.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 7
_lib.fd_ed25519_hip_gen_dev.argtypes = [ctypes.c_void_p, ctypes.c_ulong, ctypes.c_ulong, ctypes.c_ulong, _u8p,
                                        ctypes.c_ulong] + [_u8p] * 5
_lib.fd_ed25519_hip_corrupt_dev.argtypes = [ctypes.c_void_p, ctypes.c_ulong, ctypes.c_ulong, ctypes.c_ulong,
                                            ctypes.c_uint] + [_u8p] * 8
_lib.fd_ed25519_hip_engine_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
_lib.fd_ed25519_hip_engine_timing_read.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double),
                                                   ctypes.POINTER(ctypes.c_ulong)]
_lib.fd_ed25519_hip_engine_check_base_tables.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulong)]
_lib.fd_ed25519_hip_engine_base_entry.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_ulong,
                                                  ctypes.POINTER(ctypes.c_int)]
BASE_TABLE_BITS = 24     # FD_ED25519_HIP_BASE_TABLE_BITS
BASE_TABLE_SHIFT = 144   # FD_ED25519_HIP_BASE_TABLE_SHIFT
_lib.fd_ed25519_hip_dev_alloc.argtypes = [ctypes.c_void_p, ctypes.c_ulong]
_lib.fd_ed25519_hip_dev_alloc.restype = ctypes.c_void_p
_lib.fd_ed25519_hip_dev_free.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
_lib.fd_ed25519_hip_memcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulong,
                                       ctypes.c_int]
_lib.fd_ed25519_hip_device_clock_mhz.argtypes = [ctypes.c_void_p]
_lib.fd_ed25519_hip_diag_half_scalars.argtypes = [ctypes.c_void_p, _u8p, ctypes.c_ulong, _u8p]
_lib.fd_ed25519_hip_private_diag_dsm.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_ulong] + [_u8p] * 8
_lib.fd_ed25519_hip_private_diag_dsm_nmax.argtypes = [ctypes.c_void_p, ctypes.c_int]
_lib.fd_ed25519_hip_private_diag_dsm_nmax.restype = ctypes.c_ulong
_lib.fd_ed25519_hip_private_diag_dsm_check.argtypes = [ctypes.c_int, ctypes.c_ulong, ctypes.c_ulong, ctypes.c_int] + [_u8p] * 7
_lib.fd_ed25519_hip_private_diag_prep.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_ulong, ctypes.c_ulong] + [_u8p] * 15
_lib.fd_ed25519_hip_private_diag_prep_nmax.argtypes = [ctypes.c_void_p, ctypes.c_int]
_lib.fd_ed25519_hip_private_diag_prep_nmax.restype = ctypes.c_ulong
_lib.fd_ed25519_hip_private_diag_prep_check.argtypes = [ctypes.c_int, ctypes.c_ulong, ctypes.c_ulong, ctypes.c_ulong] + [_u8p] * 6
_lib.fd_ed25519_hip_private_sign_table.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
_lib.fd_ed25519_hip_verify_digests_dev.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 5
_lib.fd_ed25519_hip_strerror.argtypes = [ctypes.c_int]
_lib.fd_ed25519_hip_strerror.restype = ctypes.c_char_p

# Ed25519 precompile instructions of raw transactions (include/fd_ed25519_hip.h Part 2b)
PRECOMPILE_ERR_SIGNATURE = -3        # FD_EXECUTOR_PRECOMPILE_ERR_SIGNATURE
PRECOMPILE_ERR_DATA_OFFSET = -4      # FD_EXECUTOR_PRECOMPILE_ERR_DATA_OFFSET
PRECOMPILE_ERR_INSTR_DATA_SIZE = -5  # FD_EXECUTOR_PRECOMPILE_ERR_INSTR_DATA_SIZE
PRECOMPILE_PARSE_FAILED = -16
PRECOMPILE_BAD_RESERVATION = -17
PRECOMPILE_ENT_MAX = 87
# fd_ed25519_hip_precompile_ent_t
PRECOMPILE_ENT_DTYPE = np.dtype([("instr", np.uint8), ("pre", np.int8), ("sig_off", np.uint16), ("pub_off", np.uint16),
                                 ("msg_off", np.uint16), ("msg_sz", np.uint16)])
_lib.fd_ed25519_hip_precompile_count.argtypes = [ctypes.c_char_p, ctypes.c_ulong]
_lib.fd_ed25519_hip_precompile_count.restype = ctypes.c_uint
_lib.fd_ed25519_hip_precompile_plan.argtypes = [ctypes.c_char_p, ctypes.c_ulong, ctypes.c_void_p, ctypes.c_ulong,
                                                ctypes.POINTER(ctypes.c_byte), ctypes.POINTER(ctypes.c_ubyte)]
_lib.fd_ed25519_hip_precompile_dev.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 4 + [ctypes.c_ulong] + [_u8p] * 5
_lib.fd_ed25519_hip_precompile_host.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 5


def precompile_work_bytes(ntxn, n_ent):
    """FD_ED25519_HIP_PRECOMPILE_WORK_BYTES"""
    return 111 * int(n_ent) + 3 * int(ntxn) + 16


def precompile_count(payload):
    """fd_ed25519_hip_precompile_count: the entries to reserve for one raw
    transaction (host only)."""
    payload = bytes(payload)
    return _lib.fd_ed25519_hip_precompile_count(payload, len(payload))


def precompile_plan(payload):
    """fd_ed25519_hip_precompile_plan: (entries as PRECOMPILE_ENT_DTYPE
    records, parse-or-header code, index of the first instruction whose
    header fails or 0xFF) of one raw transaction (host only)."""
    payload = bytes(payload)
    ents = np.zeros(PRECOMPILE_ENT_MAX, PRECOMPILE_ENT_DTYPE)
    code, instr = ctypes.c_byte(0), ctypes.c_ubyte(0)
    n = _lib.fd_ed25519_hip_precompile_plan(payload, len(payload), ents.ctypes.data, len(ents), ctypes.byref(code),
                                            ctypes.byref(instr))
    return ents[:n], code.value, instr.value


# leader signatures of Merkle shreds (include/fd_ed25519_hip.h Part 2c)
SHRED_OK = 0
SHRED_ERR_PARSE = -16
SHRED_UNSUPPORTED = -18
SHRED_ERR_HEADER = -19
SHRED_ERR_SIGNATURE = -20
_lib.fd_ed25519_hip_shred_root.argtypes = [ctypes.c_char_p, ctypes.c_ulong, ctypes.c_char_p]
_lib.fd_ed25519_hip_shreds_dev.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 9
_lib.fd_ed25519_hip_shreds_host.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 6


def shred_work_bytes(n):
    """FD_ED25519_HIP_SHRED_WORK_BYTES"""
    return 110 * int(n) + 16


def shred_root(shred):
    """fd_ed25519_hip_shred_root: (code, the 32-byte Merkle root the leader
    signed or None) of one raw shred (host only)."""
    shred = bytes(shred)
    root = ctypes.create_string_buffer(32)
    code = _lib.fd_ed25519_hip_shred_root(shred, len(shred), root)
    return code, (root.raw if code == 0 else None)


# sealing a leader's FEC sets (include/fd_ed25519_hip.h Part 2f)
FEC_OK = 0
FEC_ERR_PARSE = -16
FEC_UNSUPPORTED = -18
FEC_ERR_SET = -19
FEC_SET_MAX = 134
_lib.fd_ed25519_hip_fec_root.argtypes = [_u8p, _u8p, _u8p, ctypes.c_ulong, ctypes.c_char_p, _u8p]
_lib.fd_ed25519_hip_fec_seal_dev.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 3 + [ctypes.c_ulong] + [_u8p] * 7
_lib.fd_ed25519_hip_fec_seal_host.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 3 + [ctypes.c_ulong] + [_u8p] * 5


def fec_work_bytes(n, n_set):
    """FD_ED25519_HIP_FEC_WORK_BYTES"""
    return 140 * int(n_set) + 4 * int(n) + 16


def fec_depth(cnt):
    """proof nodes of a leaf in a set of cnt shreds (fd_bmtree_depth( cnt ) - 1)"""
    return (int(cnt) - 1).bit_length()


def fec_root(shreds):
    """fd_ed25519_hip_fec_root: (code, 32-byte root, the 20 depth proof bytes
    of every shred) of one FEC set given as its raw shreds in tree order, or
    (code, None, None) for a set with a code (host only; nothing is written
    into the shreds)."""
    from .tile import pack_payloads
    cnt = len(shreds)
    root = ctypes.create_string_buffer(32)
    if not cnt:
        return _lib.fd_ed25519_hip_fec_root(None, None, None, 0, root, None), None, None
    buf, off, sz = pack_payloads([bytes(s) for s in shreds])
    width = 20 * fec_depth(cnt) if cnt <= FEC_SET_MAX else 0
    proofs = np.zeros(max(1, cnt * width), np.uint8)
    code = _lib.fd_ed25519_hip_fec_root(_ptr(buf), _ptr(off), _ptr(sz), cnt, root, _ptr(proofs))
    if code:
        return code, None, None
    return code, root.raw, [proofs[width * j:width * (j + 1)].tobytes() for j in range(cnt)]


# the Reed-Solomon parity of a leader's FEC sets (include/fd_ed25519_hip.h Part 2g)
_lib.fd_ed25519_hip_fec_parity.argtypes = [_u8p, _u8p, _u8p, ctypes.c_ulong]
_lib.fd_ed25519_hip_fec_parity_dev.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 3 + [ctypes.c_ulong] + [_u8p] * 3
_lib.fd_ed25519_hip_fec_parity_host.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 3 + [ctypes.c_ulong] + [_u8p] * 2


def fec_parity_region(cnt):
    """bytes of a shred the code protects in a set of cnt shreds: [0x40, +P)
    of a data shred, [0x59, +P) of a code shred"""
    return 1139 - 20 * fec_depth(cnt)


def fec_parity(shreds):
    """fd_ed25519_hip_fec_parity: (code, the shreds after the call) of one
    FEC set given as its raw shreds in tree order -- the parity regions of
    its code shreds filled when the code is 0, nothing changed otherwise
    (host only)."""
    from .tile import pack_payloads
    cnt = len(shreds)
    if not cnt:
        return _lib.fd_ed25519_hip_fec_parity(None, None, None, 0), []
    buf, off, sz = pack_payloads([bytes(s) for s in shreds])
    code = _lib.fd_ed25519_hip_fec_parity(_ptr(buf), _ptr(off), _ptr(sz), cnt)
    return code, [buf[int(off[i]):int(off[i]) + int(sz[i])].tobytes() for i in range(cnt)]


# recovering received FEC sets (include/fd_ed25519_hip.h Part 2h)
FEC_ERR_PARTIAL = -23
FEC_ERR_CORRUPT = -24
_lib.fd_ed25519_hip_fec_recover.argtypes = [_u8p] * 4 + [ctypes.c_ulong]
_lib.fd_ed25519_hip_fec_recover_dev.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 4 + [ctypes.c_ulong] + [_u8p] * 3
_lib.fd_ed25519_hip_fec_recover_host.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 4 + [ctypes.c_ulong] + [_u8p] * 2


def fec_recover(shreds, erased):
    """fd_ed25519_hip_fec_recover: (code, the slots after the call) of one
    FEC set given as its slots in tree order, erased[j] nonzero where slot j
    is erased (its bytes are not read, its length is its size) -- the erased
    slots' signatures, code headers and protected regions filled when the
    code is 0, nothing changed otherwise (host only)."""
    from .tile import pack_payloads
    cnt = len(shreds)
    if not cnt:
        return _lib.fd_ed25519_hip_fec_recover(None, None, None, None, 0), []
    buf, off, sz = pack_payloads([bytes(s) for s in shreds])
    er = _c([1 if x else 0 for x in erased], np.uint8)
    assert len(er) == cnt
    code = _lib.fd_ed25519_hip_fec_recover(_ptr(buf), _ptr(off), _ptr(sz), _ptr(er), cnt)
    return code, [buf[int(off[i]):int(off[i]) + int(sz[i])].tobytes() for i in range(cnt)]


# shredding entry batches (include/fd_ed25519_hip.h Part 2j)
SHREDDER_OK = 0
SHREDDER_ERR_BATCH = -19
SHREDDER_BAD_RESERVATION = -17
SHREDDER_DESC = np.dtype([("slot", "<u8"), ("data_idx", "<u4"), ("parity_idx", "<u4"), ("version", "<u2"), ("parent_off", "<u2"),
                          ("reference_tick", "u1"), ("block_complete", "u1"), ("pad", "u1", (2,))])
assert SHREDDER_DESC.itemsize == 24
_lib.fd_ed25519_hip_shredder_count.argtypes = [ctypes.c_ulong] + [ctypes.POINTER(ctypes.c_ulong)] * 3
_lib.fd_ed25519_hip_shredder.argtypes = [_u8p, ctypes.c_ulong] + [_u8p] * 5
_SHREDDER_FRONT = ([ctypes.c_void_p, ctypes.c_ulong, _u8p, ctypes.c_ulong] + [_u8p] * 5 + [ctypes.c_ulong, ctypes.c_ulong, _u8p,
                   ctypes.c_ulong, ctypes.c_ulong] + [_u8p] * 4)
_lib.fd_ed25519_hip_shredder_front_dev.argtypes = _SHREDDER_FRONT + [ctypes.c_void_p]
_lib.fd_ed25519_hip_shredder_dev.argtypes = _SHREDDER_FRONT + [_u8p] * 5 + [ctypes.c_void_p]
_lib.fd_ed25519_hip_shredder_host.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 6 + [ctypes.c_ulong] + [_u8p] * 5


def shredder_work_bytes(n, n_set):
    """FD_ED25519_HIP_SHREDDER_WORK_BYTES"""
    return fec_work_bytes(n, n_set) + 33 * int(n_set) + 16


def shredder_desc(slot=0, data_idx=0, parity_idx=0, version=0, parent_off=0, reference_tick=0, block_complete=0):
    """one fd_ed25519_hip_shredder_batch_t; the integer fields narrow as the
    reference's casts do (idx mod 2^32, version and parent_off mod 2^16)"""
    d = np.zeros(1, SHREDDER_DESC)
    d["slot"], d["data_idx"], d["parity_idx"] = slot & (2**64 - 1), data_idx & 0xFFFFFFFF, parity_idx & 0xFFFFFFFF
    d["version"], d["parent_off"] = version & 0xFFFF, parent_off & 0xFFFF
    d["reference_tick"], d["block_complete"] = reference_tick & 0xFF, block_complete & 0xFF
    return d


def shredder_count(sz):
    """fd_ed25519_hip_shredder_count: (sets, data shreds, parity shreds) of a batch of sz bytes"""
    out = [ctypes.c_ulong() for _ in range(3)]
    _check(_lib.fd_ed25519_hip_shredder_count(int(sz), *[ctypes.byref(x) for x in out]))
    return tuple(int(x.value) for x in out)


def shredder(batch, desc):
    """fd_ed25519_hip_shredder: (code, the sets of one batch, each the list of
    its shreds in tree order -- data shreds whole, parity shreds with header
    and zero proof and a zero parity region) (host only); desc from
    shredder_desc."""
    batch = bytes(batch)
    n_set, nd, npar = shredder_count(len(batch))
    n = nd + npar
    buf = np.zeros(max(1, 1228 * n), np.uint8)
    off = np.arange(max(1, n), dtype=np.uint64) * 1228
    sz, first = np.zeros(max(1, n), np.uint32), np.zeros(n_set + 1, np.uint32)
    src = np.frombuffer(batch or b"\0", np.uint8)
    code = _lib.fd_ed25519_hip_shredder(_ptr(src), len(batch), _ptr(_c(desc, SHREDDER_DESC)), _ptr(buf), _ptr(off), _ptr(sz),
                                        _ptr(first))
    if code:
        return code, []
    flat = [buf[1228 * i:1228 * i + int(sz[i])].tobytes() for i in range(n)]
    return code, [flat[int(first[k]):int(first[k + 1])] for k in range(n_set)]


# a block's proof-of-history hash chain (include/fd_ed25519_hip.h Part 2i)
POH_ERR_PARSE = -16
POH_UNSUPPORTED = -18
POH_ERR_HASH = -25
POH_HASH_CNT_CEIL = 1 << 17
_lib.fd_ed25519_hip_poh_prepare_count.argtypes = [_u8p, ctypes.c_ulong, _u8p, _u8p]
_lib.fd_ed25519_hip_poh_prepare.argtypes = [_u8p] + [ctypes.c_ulong] * 4 + [_u8p] * 4
_lib.fd_ed25519_hip_poh.argtypes = [_u8p, ctypes.c_ulong, ctypes.c_ulong] + [_u8p] * 3 + [ctypes.c_ulong, _u8p, ctypes.c_ulong,
                                                                                        _u8p, _u8p]
_lib.fd_ed25519_hip_poh_dev.argtypes = ([ctypes.c_void_p, ctypes.c_ulong, _u8p, ctypes.c_ulong] + [_u8p] * 3 +
                                        [ctypes.c_ulong, _u8p, ctypes.c_ulong] + [_u8p] * 4)
_lib.fd_ed25519_hip_poh_host.argtypes = ([ctypes.c_void_p, ctypes.c_ulong, _u8p, ctypes.c_ulong] + [_u8p] * 3 +
                                         [ctypes.c_ulong, _u8p, ctypes.c_ulong] + [_u8p] * 2)
_lib.fd_ed25519_hip_poh_blocks_host.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 4 + [ctypes.c_ulong] + [_u8p] * 3


def poh_work_bytes(n, n_sig):
    """FD_ED25519_HIP_POH_WORK_BYTES"""
    return 32 * int(n_sig) + 33 * int(n) + 16


def poh_prepare(block, first_in_off=0):
    """fd_ed25519_hip_poh_prepare_count + _prepare: the walk of one raw block
    -> (code, hdr_off u64[n], in_off u64[n], sig_first u32[n+1], sig_off
    u64[n_sig]), offsets relative to the block's first byte and in_off[0] =
    first_in_off; the arrays are None when the code is not 0 (host only)."""
    block = np.frombuffer(bytes(block), np.uint8) if len(block) else np.zeros(0, np.uint8)
    n, n_sig = ctypes.c_ulong(0), ctypes.c_ulong(0)
    ptr = _ptr(block) if len(block) else None
    code = _lib.fd_ed25519_hip_poh_prepare_count(ptr, len(block), ctypes.byref(n), ctypes.byref(n_sig))
    if code:
        return code, None, None, None, None
    n, n_sig = n.value, n_sig.value
    hdr, inn = np.zeros(max(1, n), np.uint64), np.zeros(max(1, n), np.uint64)
    first, sig = np.zeros(n + 1, np.uint32), np.zeros(max(1, n_sig), np.uint64)
    code = _lib.fd_ed25519_hip_poh_prepare(ptr, len(block), int(first_in_off), n, n_sig, _ptr(hdr), _ptr(inn), _ptr(first),
                                           _ptr(sig))
    assert code == 0, code
    return 0, hdr[:n], inn[:n], first, sig[:n_sig]


def _poh_args(buf, hdr_off, in_off, sig_first, sig_off):
    buf = np.frombuffer(bytes(buf), np.uint8) if not isinstance(buf, np.ndarray) else _c(buf, np.uint8)
    hdr, inn = _c(hdr_off, np.uint64), _c(in_off, np.uint64)
    first, sig = _c(sig_first, np.uint32), _c(sig_off, np.uint64)
    n = len(hdr)
    assert len(inn) == n and len(first) == n + 1
    return buf, hdr, inn, first, sig, n


def poh_verify(buf, hdr_off, in_off, sig_first, sig_off, hash_cnt_max=POH_HASH_CNT_CEIL):
    """fd_ed25519_hip_poh: (int8 code per microblock, the computed states
    uint8[n][32]) of the microblocks described by offsets into buf (host
    only)."""
    buf, hdr, inn, first, sig, n = _poh_args(buf, hdr_off, in_off, sig_first, sig_off)
    out, states = np.zeros(max(1, n), np.int8), np.zeros((max(1, n), 32), np.uint8)
    _check(_lib.fd_ed25519_hip_poh(_ptr(buf) if len(buf) else None, len(buf), n, _ptr(hdr), _ptr(inn), _ptr(first), len(sig),
                                   _ptr(sig) if len(sig) else None, int(hash_cnt_max), _ptr(out), _ptr(states)))
    return out[:n], states[:n]


# signed gossip and repair control packets (include/fd_ed25519_hip.h Part 2d)
PROTO_GOSSIP = 0
PROTO_REPAIR_SERV = 1
PACKET_OK = 0
PACKET_ERR_PARSE = -16
PACKET_UNSUPPORTED = -18
PACKET_ERR_SIGNATURE = -20
PACKET_NOT_FOR_SELF = -21
PACKET_MAX = 1232
# fd_ed25519_hip_packet_plan_t
PACKET_PLAN_DTYPE = np.dtype([("key_off", np.uint16), ("sig_off", np.uint16), ("msg0_off", np.uint16), ("msg0_sz", np.uint16),
                              ("msg1_off", np.uint16), ("msg1_sz", np.uint16), ("disc", np.uint32)])
_lib.fd_ed25519_hip_packet_plan.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_ulong, ctypes.c_char_p, ctypes.c_void_p]
_lib.fd_ed25519_hip_packets_dev.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_ulong] + [_u8p] * 3 + \
    [ctypes.c_ulong, ctypes.c_char_p] + [_u8p] * 4
_lib.fd_ed25519_hip_packets_host.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_ulong] + [_u8p] * 3 + \
    [ctypes.c_char_p, _u8p]


def packet_work_bytes(n, pkt_bytes):
    """FD_ED25519_HIP_PACKET_WORK_BYTES"""
    return 110 * int(n) + ((int(pkt_bytes) + 31) & ~15)


def _self_key(self_key):
    self_key = bytes(self_key)
    if len(self_key) != 32:
        raise ValueError("self_key must be 32 bytes")
    return self_key


def packet_plan(proto, pkt, self_key):
    """fd_ed25519_hip_packet_plan: (code, plan as one PACKET_PLAN_DTYPE record)
    of one raw packet (host only): where its key, signature and the two runs
    of its signed message lie when the code is 0."""
    pkt = bytes(pkt)
    plan = np.zeros(1, PACKET_PLAN_DTYPE)
    code = _lib.fd_ed25519_hip_packet_plan(int(proto), pkt, len(pkt), _self_key(self_key), plan.ctypes.data)
    if code == -22:   # FD_ED25519_HIP_ERR_INVAL: an unknown protocol
        raise ValueError("packet_plan: unknown protocol")
    return code, plan[0]


# the CRDS values of gossip pull responses and push messages (include/fd_ed25519_hip.h Part 2e)
CRDS_OK = 0
CRDS_ERR_PARSE = -16
CRDS_BAD_RESERVATION = -17
CRDS_UNSUPPORTED = -18
CRDS_ERR_SIGNATURE = -20
CRDS_OWN = -21
CRDS_VAL_MAX = 10
# fd_ed25519_hip_crds_val_t
CRDS_VAL_DTYPE = np.dtype([("disc", np.uint32), ("sig_off", np.uint16), ("key_off", np.uint16), ("msg_off", np.uint16),
                           ("msg_sz", np.uint16), ("pre", np.int8)], align=True)
_lib.fd_ed25519_hip_crds_count.argtypes = [ctypes.c_char_p, ctypes.c_ulong]
_lib.fd_ed25519_hip_crds_count.restype = ctypes.c_uint
_lib.fd_ed25519_hip_crds_plan.argtypes = [ctypes.c_char_p, ctypes.c_ulong, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_ulong,
                                          ctypes.POINTER(ctypes.c_byte)]
_lib.fd_ed25519_hip_crds_dev.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 3 + [ctypes.c_ulong, ctypes.c_char_p, _u8p,
                                                                                         ctypes.c_ulong] + [_u8p] * 6
_lib.fd_ed25519_hip_crds_host.argtypes = [ctypes.c_void_p, ctypes.c_ulong] + [_u8p] * 3 + [ctypes.c_char_p] + [_u8p] * 4


def crds_work_bytes(n, n_val):
    """FD_ED25519_HIP_CRDS_WORK_BYTES"""
    return 114 * int(n_val) + int(n) + 16


def crds_count(pkt):
    """fd_ed25519_hip_crds_count: the values to reserve for one raw gossip
    packet (host only)."""
    pkt = bytes(pkt)
    return _lib.fd_ed25519_hip_crds_count(pkt, len(pkt))


def crds_plan(pkt, self_key):
    """fd_ed25519_hip_crds_plan: (packet code, values as CRDS_VAL_DTYPE
    records) of one raw gossip packet (host only): where each value's
    signature, key and signed message lie, and pre = CRDS_OWN for a value
    under self_key."""
    pkt = bytes(pkt)
    vals = np.zeros(CRDS_VAL_MAX, CRDS_VAL_DTYPE)
    code = ctypes.c_byte(0)
    n = _lib.fd_ed25519_hip_crds_plan(pkt, len(pkt), _self_key(self_key), vals.ctypes.data, len(vals), ctypes.byref(code))
    return code.value, vals[:n]


_lib.fd_ed25519_hip_last_error.restype = ctypes.c_char_p


class _Info(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("cu_cnt", ctypes.c_int), ("dsm_blocks_per_cu", ctypes.c_int),
                ("dsm_grid", ctypes.c_uint), ("max_chunk", ctypes.c_ulong), ("device_bytes", ctypes.c_ulong),
                ("flags", ctypes.c_int), ("arch", ctypes.c_char * 64), ("pci_domain", ctypes.c_int),
                ("pci_bus", ctypes.c_int), ("pci_device", ctypes.c_int)]


_lib.fd_ed25519_hip_engine_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Info)]


class HipError(RuntimeError):
    pass


def _check(rc):
    if rc:
        raise HipError(f"{_lib.fd_ed25519_hip_strerror(rc).decode()} ({_lib.fd_ed25519_hip_last_error().decode()})")


def library():
    """The loaded ctypes library (for callers that need raw entry points)."""
    return _lib


def strerror(err):
    return _lib.fd_ed25519_strerror(int(err)).decode()


def verify(msg, sig, public_key):
    """fd_ed25519_verify drop-in (synchronous, default engine)."""
    assert len(sig) == 64 and len(public_key) == 32
    msg = bytes(msg)
    return _lib.fd_ed25519_verify(msg, len(msg), bytes(sig), bytes(public_key), None)


def verify_batch_single_msg(msg, signatures, pubkeys, batch_sz=None):
    """fd_ed25519_verify_batch_single_msg drop-in: signatures is 64*n bytes,
    pubkeys 32*n bytes."""
    signatures, pubkeys, msg = bytes(signatures), bytes(pubkeys), bytes(msg)
    n = len(signatures) // 64 if batch_sz is None else batch_sz
    return _lib.fd_ed25519_verify_batch_single_msg(msg, len(msg), signatures or b"\0" * 64, pubkeys or b"\0" * 32,
                                                   None, n & 0xFF)


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


class Engine:
    """A libfd_ed25519_hip engine bound to one GPU."""

    def __init__(self, device=0, max_chunk=0, codes="avx512", half="extended", dsm="auto", one_stream=False,
                 overlap=True, pipeline=True, forms=None, compact=False, r16_max=None):
        flags = FLAG_CODES_PORTABLE if codes == "portable" else 0
        flags |= FLAG_ONE_STREAM if one_stream else 0
        flags |= 0 if overlap else FLAG_NO_OVERLAP
        flags |= 0 if pipeline else FLAG_NO_PIPELINE
        flags |= FLAG_COMPACT_TABLES if compact else 0
        flags |= FLAG_HALF_STRICT if half == "strict" else 0
        flags |= {"auto": 0, "quad": FLAG_DSM_QUAD, "wide": FLAG_DSM_WIDE, "oct": FLAG_DSM_OCT, "r16": FLAG_DSM_R16}[dsm]
        self._h = _lib.fd_ed25519_hip_engine_new(int(device), int(max_chunk), flags)
        if not self._h:
            raise HipError(f"engine_new failed: {_lib.fd_ed25519_hip_last_error().decode()}")
        self.codes = codes
        if forms is not None:   # (quad_max, oct_max): fd_ed25519_hip_engine_set_forms
            _check(_lib.fd_ed25519_hip_engine_set_forms(self._h, int(forms[0]), int(forms[1])))
        if r16_max is not None:   # dsm16 up to this chunk size: fd_ed25519_hip_engine_set_r16_max
            _check(_lib.fd_ed25519_hip_engine_set_r16_max(self._h, int(r16_max)))

    def close(self):
        if self._h:
            _lib.fd_ed25519_hip_engine_delete(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        i = _Info()
        _check(_lib.fd_ed25519_hip_engine_info(self._h, ctypes.byref(i)))
        return {f: (getattr(i, f).decode() if f == "arch" else getattr(i, f)) for f, _ in _Info._fields_}

    @property
    def stream(self):
        return _lib.fd_ed25519_hip_engine_stream(self._h)

    def sync(self):
        _check(_lib.fd_ed25519_hip_engine_sync(self._h))

    def verify_host(self, msgs, msg_off, msg_sz, sigs, pubs):
        """SoA host batch -> int8 codes (synchronous)."""
        n = len(msg_sz)
        out = np.zeros(n, dtype=np.int8)
        if n == 0:
            return out
        msgs = _c(msgs, np.uint8) if len(msgs) else np.zeros(1, np.uint8)
        off, sz = _c(msg_off, np.uint64), _c(msg_sz, np.uint32)
        sigs, pubs = _c(sigs, np.uint8).reshape(-1), _c(pubs, np.uint8).reshape(-1)
        assert len(sigs) >= 64 * n and len(pubs) >= 32 * n
        _check(_lib.fd_ed25519_hip_verify_host(self._h, n, _ptr(msgs), _ptr(off), _ptr(sz), _ptr(sigs), _ptr(pubs),
                                               _ptr(out)))
        return out

    def verify_txns_host(self, msgs, txn_msg_off, txn_msg_sz, txn_first, txn_cnt, sigs, pubs, want_sig_codes=False):
        """batch_single_msg semantics per transaction -> (txn codes, sig codes|None)."""
        ntxn = len(txn_cnt)
        out = np.zeros(ntxn, dtype=np.int8)
        nsig = len(sigs) if np.ndim(sigs) == 2 else len(sigs) // 64
        osig = np.zeros(max(nsig, 1), dtype=np.int8) if want_sig_codes else None
        if ntxn == 0:
            return out, osig
        msgs = _c(msgs, np.uint8) if len(msgs) else np.zeros(1, np.uint8)
        sigs = _c(sigs, np.uint8).reshape(-1) if nsig else np.zeros(64, np.uint8)
        pubs = _c(pubs, np.uint8).reshape(-1) if nsig else np.zeros(32, np.uint8)
        _check(_lib.fd_ed25519_hip_verify_txns_host(
            self._h, ntxn, _ptr(msgs), _ptr(_c(txn_msg_off, np.uint64)), _ptr(_c(txn_msg_sz, np.uint32)),
            _ptr(_c(txn_first, np.uint32)), _ptr(_c(txn_cnt, np.uint32)), _ptr(sigs), _ptr(pubs), _ptr(out),
            _ptr(osig)))
        return out, osig

    def verify_dev(self, n, d_msgs, d_off, d_sz, d_sigs, d_pubs, d_out, stream=None):
        """Device-resident batch: arguments are device addresses (ints); async."""
        _check(_lib.fd_ed25519_hip_verify_dev(self._h, int(n), d_msgs, d_off, d_sz, d_sigs, d_pubs, d_out, stream))

    def txn_combine_dev(self, ntxn, d_sig_codes, d_first, d_cnt, d_out, stream=None):
        _check(_lib.fd_ed25519_hip_txn_combine_dev(self._h, int(ntxn), d_sig_codes, d_first, d_cnt, d_out, stream))

    def precompile_host(self, payloads):
        """The Ed25519 precompile instructions of raw transactions
        (fd_ed25519_hip_precompile_host) -> (int8 code per transaction,
        uint8 index of the failing instruction or 0xFF); synchronous."""
        from .tile import pack_payloads
        n = len(payloads)
        codes, instr = np.zeros(n, np.int8), np.full(n, 0xFF, np.uint8)
        if n:
            buf, off, sz = pack_payloads(payloads)
            _check(_lib.fd_ed25519_hip_precompile_host(self._h, n, _ptr(buf), _ptr(off), _ptr(sz), _ptr(codes),
                                                       _ptr(instr)))
        return codes, instr

    def shreds_host(self, shreds, leaders):
        """The leader signatures of raw Merkle shreds
        (fd_ed25519_hip_shreds_host): leaders is one 32-byte key per shred,
        or one key for all -> (int8 code per shred, uint8 [n, 32] derived
        roots, zero where none was derived); synchronous."""
        from .tile import pack_payloads
        n = len(shreds)
        codes, roots = np.zeros(n, np.int8), np.zeros((n, 32), np.uint8)
        if n:
            if isinstance(leaders, (bytes, bytearray)):
                leaders = [bytes(leaders)] * n
            keys = np.frombuffer(b"".join(bytes(k) for k in leaders), np.uint8)
            assert keys.size == 32 * n
            buf, off, sz = pack_payloads(shreds)
            _check(_lib.fd_ed25519_hip_shreds_host(self._h, n, _ptr(buf), _ptr(off), _ptr(sz), _ptr(keys), _ptr(codes),
                                                   _ptr(roots)))
        return codes, roots

    def shreds_dev(self, n, d_shreds, d_off, d_sz, d_leaders, d_work, d_out, d_roots=None, d_sig_out=None, stream=None):
        """Device-resident fd_ed25519_hip_shreds_dev: device addresses (ints); async."""
        _check(_lib.fd_ed25519_hip_shreds_dev(self._h, int(n), d_shreds, d_off, d_sz, d_leaders, d_work, d_out, d_roots,
                                              d_sig_out, stream))

    def packets_host(self, proto, pkts, self_key):
        """Signed gossip (PROTO_GOSSIP) or repair (PROTO_REPAIR_SERV) control
        packets (fd_ed25519_hip_packets_host) under the validator's own
        identity self_key -> int8 code per packet (PACKET_*); synchronous."""
        from .tile import pack_payloads
        n = len(pkts)
        codes = np.zeros(n, np.int8)
        self_key = _self_key(self_key)
        if n:
            buf, off, sz = pack_payloads(pkts)
            _check(_lib.fd_ed25519_hip_packets_host(self._h, int(proto), n, _ptr(buf), _ptr(off), _ptr(sz), self_key,
                                                    _ptr(codes)))
        return codes

    def packets_dev(self, proto, n, d_pkts, d_off, d_sz, pkt_bytes, self_key, d_work, d_out, d_sig_out=None, stream=None):
        """Device-resident fd_ed25519_hip_packets_dev: device addresses (ints),
        self_key 32 host bytes; async."""
        _check(_lib.fd_ed25519_hip_packets_dev(self._h, int(proto), int(n), d_pkts, d_off, d_sz, int(pkt_bytes),
                                               _self_key(self_key), d_work, d_out, d_sig_out, stream))

    def precompile_dev(self, ntxn, d_payloads, d_off, d_sz, d_ent_first, n_ent, d_work, d_txn_out, d_instr_out,
                       d_ent_out=None, stream=None):
        """Device-resident fd_ed25519_hip_precompile_dev: device addresses (ints); async."""
        _check(_lib.fd_ed25519_hip_precompile_dev(self._h, int(ntxn), d_payloads, d_off, d_sz, d_ent_first, int(n_ent),
                                                  d_work, d_txn_out, d_instr_out, d_ent_out, stream))

    def crds_host(self, pkts, self_key, want_hashes=False):
        """The CRDS values of raw gossip pull responses and push messages
        (fd_ed25519_hip_crds_host) under the validator's own identity
        self_key -> (int8 code per packet, uint32 val_first [n + 1], int8 code
        per value, the values of packet i at val_first[i]..val_first[i + 1])
        and, with want_hashes, uint8 [n_val, 32] value hashes; synchronous."""
        from .tile import pack_payloads
        n = len(pkts)
        self_key = _self_key(self_key)
        pkt_codes, first = np.zeros(n, np.int8), np.zeros(n + 1, np.uint32)
        vals = np.zeros(max(1, sum(crds_count(p) for p in pkts)), np.int8)
        hashes = np.zeros((len(vals), 32), np.uint8) if want_hashes else None
        if n:
            buf, off, sz = pack_payloads(pkts)
            _check(_lib.fd_ed25519_hip_crds_host(self._h, n, _ptr(buf), _ptr(off), _ptr(sz), self_key, _ptr(first),
                                                 _ptr(pkt_codes), _ptr(vals), _ptr(hashes)))
        n_val = int(first[n])
        out = (pkt_codes, first, vals[:n_val])
        return out + (hashes[:n_val],) if want_hashes else out

    def crds_dev(self, n, d_pkts, d_off, d_sz, pkt_bytes, self_key, d_val_first, n_val, d_work, d_pkt_out, d_val_out,
                 d_sig_out=None, d_hash_out=None, stream=None):
        """Device-resident fd_ed25519_hip_crds_dev: device addresses (ints),
        self_key 32 host bytes; async."""
        _check(_lib.fd_ed25519_hip_crds_dev(self._h, int(n), d_pkts, d_off, d_sz, int(pkt_bytes), _self_key(self_key),
                                            d_val_first, int(n_val), d_work, d_pkt_out, d_val_out, d_sig_out, d_hash_out,
                                            stream))

    def _fec_flat(self, shreds, set_first, call):
        """What the three fec_*_flat share: packs shreds, runs call(n, shreds,
        off, sz, n_set, set_first, codes) -- a *_host of the library over those
        pointers -- and unpacks -> (int8 code per set, the shreds after)."""
        from .tile import pack_payloads
        n, n_set = len(shreds), len(set_first) - 1
        first = _c(set_first, np.uint32)
        codes = np.zeros(max(1, n_set), np.int8)
        buf, off, sz = pack_payloads([bytes(s) for s in shreds]) if n else (np.zeros(1, np.uint8),) * 3
        _check(call(n, _ptr(buf), _ptr(off), _ptr(sz), n_set, _ptr(first), _ptr(codes)))
        return codes[:n_set], [buf[int(off[i]):int(off[i]) + int(sz[i])].tobytes() for i in range(n)]

    @staticmethod
    def _fec_by_sets(sets, flat_call):
        """What the three fec_*_host share: flattens sets, runs flat_call(the
        shreds, their set_first) -- a fec_*_flat -- and splits the shreds it
        returns (its second result) into sets again."""
        first = [0]
        for s in sets:
            first.append(first[-1] + len(s))
        codes, flat, *rest = flat_call([x for s in sets for x in s], first)
        return (codes, [flat[first[k]:first[k + 1]] for k in range(len(sets))], *rest)

    def fec_seal_flat(self, shreds, set_first, privs):
        """fd_ed25519_hip_fec_seal_host on shreds (a list of raw shreds) whose
        set k is shreds[set_first[k]:set_first[k + 1]] in tree order; privs is
        one 32-byte private key per set, one for all, or None (proofs and
        roots only) -> (int8 code per set, the shreds after the call, uint8
        [n_set, 32] roots, uint8 [n_set, 64] signatures or None);
        synchronous."""
        n_set = len(set_first) - 1
        roots = np.zeros((max(1, n_set), 32), np.uint8)
        keys = sigs = None
        if privs is not None:
            if isinstance(privs, (bytes, bytearray)):
                privs = [bytes(privs)] * n_set
            keys = np.frombuffer(b"".join(bytes(k) for k in privs) or bytes(32), np.uint8)
            assert keys.size == 32 * max(1, n_set)
            sigs = np.zeros((max(1, n_set), 64), np.uint8)
        codes, out = self._fec_flat(shreds, set_first, lambda n, buf, off, sz, ns, first, codes: _lib.fd_ed25519_hip_fec_seal_host(
            self._h, n, buf, off, sz, ns, first, _ptr(keys), codes, _ptr(roots), _ptr(sigs)))
        return codes, out, roots[:n_set], (sigs[:n_set] if sigs is not None else None)

    def fec_seal_host(self, sets, privs):
        """Seals FEC sets (fd_ed25519_hip_fec_seal_host): sets is a list of
        sets, each the list of its raw shreds in tree order (data, then
        parity), privs as for fec_seal_flat -> (int8 code per set, the sets
        with signature and proofs written where the code is 0, roots,
        signatures or None); synchronous."""
        return self._fec_by_sets(sets, lambda flat, first: self.fec_seal_flat(flat, first, privs))

    def fec_seal_dev(self, n, d_shreds, d_off, d_sz, n_set, d_set_first, d_privs, d_work, d_set_out, d_roots=None,
                     d_sigs=None, stream=None):
        """Device-resident fd_ed25519_hip_fec_seal_dev: device addresses (ints); async."""
        _check(_lib.fd_ed25519_hip_fec_seal_dev(self._h, int(n), d_shreds, d_off, d_sz, int(n_set), d_set_first, d_privs,
                                                d_work, d_set_out, d_roots, d_sigs, stream))

    def fec_parity_flat(self, shreds, set_first):
        """fd_ed25519_hip_fec_parity_host on shreds (a list of raw shreds)
        whose set k is shreds[set_first[k]:set_first[k + 1]] in tree order ->
        (int8 code per set, the shreds after the call); synchronous."""
        return self._fec_flat(shreds, set_first, lambda n, buf, off, sz, ns, first, codes: _lib.fd_ed25519_hip_fec_parity_host(
            self._h, n, buf, off, sz, ns, first, codes))

    def fec_parity_host(self, sets):
        """Fills the parity shreds of FEC sets (fd_ed25519_hip_fec_parity_host):
        sets is a list of sets, each the list of its raw shreds in tree order
        (data, then parity, of which the first 0x59 bytes are read) -> (int8
        code per set, the sets with the parity regions written where the code
        is 0); synchronous."""
        return self._fec_by_sets(sets, self.fec_parity_flat)

    def fec_parity_dev(self, n, d_shreds, d_off, d_sz, n_set, d_set_first, d_set_out, stream=None):
        """Device-resident fd_ed25519_hip_fec_parity_dev: device addresses (ints); async."""
        _check(_lib.fd_ed25519_hip_fec_parity_dev(self._h, int(n), d_shreds, d_off, d_sz, int(n_set), d_set_first, d_set_out,
                                                  stream))

    def fec_recover_flat(self, shreds, erased, set_first):
        """fd_ed25519_hip_fec_recover_host on shreds (a list of slots) whose
        set k is shreds[set_first[k]:set_first[k + 1]] in tree order, erased
        one flag per slot -> (int8 code per set, the slots after the call);
        synchronous."""
        er = _c([1 if x else 0 for x in erased] + [0], np.uint8)
        assert len(er) == len(shreds) + 1
        return self._fec_flat(shreds, set_first, lambda n, buf, off, sz, ns, first, codes: _lib.fd_ed25519_hip_fec_recover_host(
            self._h, n, buf, off, sz, _ptr(er), ns, first, codes))

    def fec_recover_host(self, sets, erased):
        """Recovers received FEC sets (fd_ed25519_hip_fec_recover_host): sets
        is a list of sets, each the list of its slots in tree order, erased
        the list of each set's flags (nonzero: the slot is erased and only
        its length counts) -> (int8 code per set, the sets with the erased
        slots filled where the code is 0); synchronous."""
        flags = [x for e in erased for x in e]
        return self._fec_by_sets(sets, lambda flat, first: self.fec_recover_flat(flat, flags, first))

    def fec_recover_dev(self, n, d_shreds, d_off, d_sz, d_erased, n_set, d_set_first, d_set_out, stream=None):
        """Device-resident fd_ed25519_hip_fec_recover_dev: device addresses (ints); async."""
        _check(_lib.fd_ed25519_hip_fec_recover_dev(self._h, int(n), d_shreds, d_off, d_sz, d_erased, int(n_set), d_set_first,
                                                   d_set_out, stream))

    def shredder_host(self, batches, descs, privs=None, stride=1228):
        """fd_ed25519_hip_shredder_host: batches a list of entry batches,
        descs their shredder_desc()s, privs one 32-byte key per batch, one for
        all, or None -> (int8 code per batch, the call's sets, each the list of
        its finished shreds, uint8 [n_set, 32] roots, uint8 [n_set, 64]
        signatures or None); synchronous."""
        from .tile import pack_payloads
        nb = len(batches)
        counts = [shredder_count(len(b)) for b in batches]
        n_set, n = sum(c[0] for c in counts), sum(c[1] + c[2] for c in counts)
        buf, off, sz = pack_payloads([bytes(b) for b in batches]) if nb else (np.zeros(1, np.uint8),) * 3
        desc = np.concatenate([_c(d, SHREDDER_DESC) for d in descs]) if nb else np.zeros(1, SHREDDER_DESC)
        keys = sigs = None
        if privs is not None:
            if isinstance(privs, (bytes, bytearray)):
                privs = [bytes(privs)] * nb
            keys = np.frombuffer(b"".join(bytes(k) for k in privs) or bytes(32), np.uint8)
            sigs = np.zeros((max(1, n_set), 64), np.uint8)
        out = np.zeros(max(1, stride * n), np.uint8)
        ssz, first = np.zeros(max(1, n), np.uint32), np.zeros(n_set + 1, np.uint32)
        codes, roots = np.zeros(max(1, nb), np.int8), np.zeros((max(1, n_set), 32), np.uint8)
        _check(_lib.fd_ed25519_hip_shredder_host(self._h, nb, _ptr(buf), _ptr(off), _ptr(_c(sz, np.uint32)), _ptr(desc), _ptr(keys),
                                                 _ptr(out), stride, _ptr(ssz), _ptr(first), _ptr(codes), _ptr(roots), _ptr(sigs)))
        flat = [out[stride * i:stride * i + int(ssz[i])].tobytes() for i in range(n)]
        sets = [flat[int(first[k]):int(first[k + 1])] for k in range(n_set)]
        return codes[:nb], sets, roots[:n_set], (sigs[:n_set] if sigs is not None else None)

    def shredder_front_dev(self, nb, d_buf, buf_sz, d_batch_off, d_batch_sz, d_desc, d_set_first_b, d_shred_first_b, n_set, n,
                           d_shreds, base_off, stride, d_shred_off, d_shred_sz, d_set_first, d_batch_out, stream=None):
        """Device-resident fd_ed25519_hip_shredder_front_dev: device addresses (ints); async."""
        _check(_lib.fd_ed25519_hip_shredder_front_dev(self._h, int(nb), d_buf, int(buf_sz), d_batch_off, d_batch_sz, d_desc,
                                                      d_set_first_b, d_shred_first_b, int(n_set), int(n), d_shreds, int(base_off),
                                                      int(stride), d_shred_off, d_shred_sz, d_set_first, d_batch_out, stream))

    def shredder_dev(self, nb, d_buf, buf_sz, d_batch_off, d_batch_sz, d_desc, d_set_first_b, d_shred_first_b, n_set, n,
                     d_shreds, base_off, stride, d_shred_off, d_shred_sz, d_set_first, d_batch_out, d_privs, d_work, d_set_out,
                     d_roots=None, d_sigs=None, stream=None):
        """Device-resident fd_ed25519_hip_shredder_dev (front, parity and seal): device addresses (ints); async."""
        _check(_lib.fd_ed25519_hip_shredder_dev(self._h, int(nb), d_buf, int(buf_sz), d_batch_off, d_batch_sz, d_desc,
                                                d_set_first_b, d_shred_first_b, int(n_set), int(n), d_shreds, int(base_off),
                                                int(stride), d_shred_off, d_shred_sz, d_set_first, d_batch_out, d_privs, d_work,
                                                d_set_out, d_roots, d_sigs, stream))

    def poh_host(self, buf, hdr_off, in_off, sig_first, sig_off, hash_cnt_max=POH_HASH_CNT_CEIL):
        """fd_ed25519_hip_poh_host: (int8 code per microblock, the computed
        states uint8[n][32]) of the microblocks described by offsets into
        buf; synchronous."""
        buf, hdr, inn, first, sig, n = _poh_args(buf, hdr_off, in_off, sig_first, sig_off)
        out, states = np.zeros(max(1, n), np.int8), np.zeros((max(1, n), 32), np.uint8)
        _check(_lib.fd_ed25519_hip_poh_host(self._h, n, _ptr(buf) if len(buf) else None, len(buf), _ptr(hdr), _ptr(inn),
                                            _ptr(first), len(sig), _ptr(sig) if len(sig) else None, int(hash_cnt_max),
                                            _ptr(out), _ptr(states)))
        return out[:n], states[:n]

    def poh_blocks_host(self, blocks, in_hashes, hash_cnt_max=POH_HASH_CNT_CEIL):
        """fd_ed25519_hip_poh_blocks_host: blocks is a list of raw blocks,
        in_hashes the 32-byte hash each one's first microblock starts from ->
        (int8 code per block, uint32 first_bad per block, the last
        microblock's header hash uint8[nb][32]); synchronous."""
        from .tile import pack_payloads
        nb = len(blocks)
        assert len(in_hashes) == nb
        codes, bad, last = np.zeros(max(1, nb), np.int8), np.zeros(max(1, nb), np.uint32), np.zeros((max(1, nb), 32), np.uint8)
        if nb:
            buf, off, sz = pack_payloads([bytes(b) for b in blocks])
            inh = np.frombuffer(b"".join(bytes(h) for h in in_hashes), np.uint8)
            assert len(inh) == 32 * nb
            off, sz = _c(off, np.uint64), _c(sz, np.uint64)
            _check(_lib.fd_ed25519_hip_poh_blocks_host(self._h, nb, _ptr(buf), _ptr(off), _ptr(sz), _ptr(inh), int(hash_cnt_max),
                                                       _ptr(codes), _ptr(bad), _ptr(last)))
        return codes[:nb], bad[:nb], last[:nb]

    def poh_dev(self, n, d_buf, buf_sz, d_hdr_off, d_in_off, d_sig_first, n_sig, d_sig_off, hash_cnt_max, d_out, d_out_hash,
                d_work, stream=None):
        """Device-resident fd_ed25519_hip_poh_dev: device addresses (ints); async."""
        _check(_lib.fd_ed25519_hip_poh_dev(self._h, int(n), d_buf, int(buf_sz), d_hdr_off, d_in_off, d_sig_first, int(n_sig),
                                           d_sig_off, int(hash_cnt_max), d_out, d_out_hash, d_work, stream))

    # ---- batched signing / synthetic workloads -------------------------
    def sign_dev(self, n, d_msgs, d_off, d_sz, d_privs, d_sigs, d_pubs, stream=None):
        _check(_lib.fd_ed25519_hip_sign_dev(self._h, int(n), d_msgs, d_off, d_sz, d_privs, d_sigs, d_pubs, stream))

    def gen_dev(self, n, seed, index_base, d_msgs, msg_bytes, d_off, d_sz, d_sigs, d_pubs, stream=None):
        _check(_lib.fd_ed25519_hip_gen_dev(self._h, int(n), int(seed), int(index_base), d_msgs, int(msg_bytes), d_off,
                                           d_sz, d_sigs, d_pubs, stream))

    def corrupt_dev(self, n, seed, index_base, ppm, d_msgs, d_off, d_sz, d_sigs, d_pubs, d_expect=None, d_cls=None,
                    stream=None):
        _check(_lib.fd_ed25519_hip_corrupt_dev(self._h, int(n), int(seed), int(index_base), int(ppm), d_msgs, d_off,
                                               d_sz, d_sigs, d_pubs, d_expect, d_cls, stream))

    # ---- measurement ------------------------------------------------------
    def timing(self, enable=True):
        _check(_lib.fd_ed25519_hip_engine_timing(self._h, 1 if enable else 0))

    def timing_read(self):
        ms = (ctypes.c_double * len(PHASES))()
        cnt = ctypes.c_ulong(0)
        _check(_lib.fd_ed25519_hip_engine_timing_read(self._h, ms, ctypes.byref(cnt)))
        return {name: ms[i] for i, name in enumerate(PHASES)}, cnt.value

    def check_base_tables(self):
        """per base table ([e]B, [e][2^144]B, and the full-length form's
        [0..2^15]B), the count of entries e with entry e+1 != entry e +
        entry 1 ((0, 0, 0) for correct tables)"""
        bad = (ctypes.c_ulong * 3)()
        _check(_lib.fd_ed25519_hip_engine_check_base_tables(self._h, bad))
        return bad[0], bad[1], bad[2]

    def base_entry(self, which, index):
        """entry `index` of wide base table `which` (0: [e]B, 1: [e][2^144]B):
        int32 [30] = (y+x, y-x, 2dxy) in radix-2^25.5 limbs"""
        out = (ctypes.c_int * 30)()
        _check(_lib.fd_ed25519_hip_engine_base_entry(self._h, which, index, out))
        return np.array(out[:], dtype=np.int64)

    def sign_table(self):
        """Diagnostic: the signer's own table [0..128]B, int32 [129][36] =
        (y+x, y-x, 2dxy) in radix-2^25.5 limbs and six zero words an entry
        (fd_ed25519_hip_private_sign_table; sign_dev and gen_dev alone read it)"""
        out = np.zeros((129, 36), dtype=np.int32)
        _check(_lib.fd_ed25519_hip_private_sign_table(self._h, out.ctypes.data))
        return out

    def diag_half_scalars(self, k_words):
        """Diagnostic: the device's half-size scalar search for k given as
        uint32 [n][8]; returns uint32 [n][12] (ok, d<0, c[5], |d|[5])."""
        k = np.ascontiguousarray(k_words, dtype=np.uint32).reshape(-1, 8)
        out = np.zeros((len(k), 12), dtype=np.uint32)
        if len(k):
            _check(_lib.fd_ed25519_hip_diag_half_scalars(self._h, k.ctypes.data_as(_u8p), len(k),
                                                         out.ctypes.data_as(_u8p)))
        return out

    def diag_dsm(self, form, sflag, hflag, pflag, pts, hs, k=None, S=None):
        """Diagnostic: the dsm phase alone on the caller's work arrays
        (fd_ed25519_hip_private_diag_dsm, csrc/fd_ed25519_hip_internal.h):
        form 0 wide, 1 quad, 2 oct, 3 r16, 4 / 8 the split forms; every
        array [rows][n]; returns the int8 codes [n].  Arrays outside the
        kernels' contracts raise HipError before anything is launched."""
        sflag, hflag = _c(sflag, np.uint8).reshape(-1), _c(hflag, np.uint8).reshape(-1)
        n = len(sflag)
        rows_p, rows_h = (int(form) * 40, 24) if form in (4, 8) else (40, 19)
        pflag, pts, hs = _c(pflag, np.uint8).reshape(-1), _c(pts, np.int32).reshape(-1), _c(hs, np.uint32).reshape(-1)
        assert len(hflag) == n and len(pflag) == 2 * n and len(pts) == rows_p * n and len(hs) == rows_h * n
        k = None if k is None else _c(k, np.uint32).reshape(-1)
        S = None if S is None else _c(S, np.uint8).reshape(-1)
        assert (k is None or len(k) == 8 * n) and (S is None or len(S) == 64 * n)
        out = np.zeros(max(n, 1), dtype=np.int8)
        _check(_lib.fd_ed25519_hip_private_diag_dsm(self._h, int(form), n, _ptr(sflag), _ptr(hflag), _ptr(pflag),
                                                    _ptr(pts), _ptr(hs), _ptr(k), _ptr(S), _ptr(out)))
        return out[:n]

    def diag_dsm_nmax(self, form):
        """the most signatures diag_dsm takes in that form on this engine"""
        return _lib.fd_ed25519_hip_private_diag_dsm_nmax(self._h, int(form))

    def diag_prep(self, form, sigs, pubs, msgs=None, msg_off=None, msg_sz=None, digests=None, cap=None):
        """Diagnostic: the hash, scalar and decode phases alone on host
        inputs (fd_ed25519_hip_private_diag_prep,
        csrc/fd_ed25519_hip_internal.h): form 0 wide, 1 / 2 the fused prep
        kernel, 3 prep16, 4 its decode blocks only, 5 prep16 running the
        full-length items; messages (msgs, msg_off, msg_sz) or digests
        [n][64].  Returns the work arrays as the kernels left them, stride
        cap (default n), as a dict: k [8][cap], sflag, hflag, pflag [2][cap],
        pts [40][cap], hs [19][cap], perm, out, fix_cnt, work_ctr, fix_list
        -- FD_ED25519_DIAG_DSM_UNWRITTEN (0x55) bytes wherever nothing was
        written.  Inputs outside the contracts raise HipError before
        anything is launched."""
        sigs, pubs = _c(sigs, np.uint8).reshape(-1), _c(pubs, np.uint8).reshape(-1)
        n = len(sigs) // 64
        cap = n if cap is None else int(cap)
        assert len(sigs) == 64 * n and len(pubs) == 32 * n
        if digests is not None:
            digests = _c(digests, np.uint8).reshape(-1)
            assert len(digests) == 64 * n
            msgs = msg_off = msg_sz = None
        else:
            msgs = _c(msgs, np.uint8).reshape(-1) if msgs is not None and len(msgs) else np.zeros(1, np.uint8)
            msg_off, msg_sz = _c(msg_off, np.uint64), _c(msg_sz, np.uint32)
            assert len(msg_off) == n and len(msg_sz) == n
        c = max(cap, 1)
        a = dict(k=np.zeros((8, c), np.uint32), sflag=np.zeros(c, np.uint8), hflag=np.zeros(c, np.uint8),
                 pflag=np.zeros((2, c), np.uint8), pts=np.zeros((40, c), np.int32), hs=np.zeros((19, c), np.uint32),
                 perm=np.zeros(c, np.uint32), out=np.zeros(c, np.int8))
        fix = np.zeros(2 + c, np.uint32)
        _check(_lib.fd_ed25519_hip_private_diag_prep(self._h, int(form), n, cap, _ptr(sigs), _ptr(pubs), _ptr(msgs),
                                                     _ptr(msg_off), _ptr(msg_sz), _ptr(digests),
                                                     *[_ptr(a[f]) for f in ("k", "sflag", "hflag", "pflag", "pts", "hs",
                                                                            "perm", "out")], _ptr(fix)))
        a.update(fix_cnt=int(fix[0]), work_ctr=int(fix[1]), fix_list=fix[2:])
        return a

    def diag_prep_nmax(self, form):
        """the most signatures diag_prep takes in that form on this engine"""
        return _lib.fd_ed25519_hip_private_diag_prep_nmax(self._h, int(form))

    def verify_digests_host(self, digests, sigs, pubs):
        """SoA host batch with the caller's SHA-512(R||A||M) per signature
        (digests [n][64]) -> int8 codes (synchronous): staged like
        verify_host, verified by fd_ed25519_hip_verify_digests_dev."""
        digests, sigs, pubs = (_c(x, np.uint8).reshape(-1) for x in (digests, sigs, pubs))
        n = len(digests) // 64
        assert len(digests) == 64 * n and len(sigs) == 64 * n and len(pubs) == 32 * n
        if n == 0:
            return np.zeros(0, dtype=np.int8)
        bufs = [self.alloc(x.nbytes).upload(x) for x in (digests, sigs, pubs)] + [self.alloc(n)]
        try:
            _check(_lib.fd_ed25519_hip_verify_digests_dev(self._h, n, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr,
                                                          None))
            self.sync()
            return bufs[3].download(np.int8, n)
        finally:
            for b in bufs:
                b.free()

    def clock_mhz(self):
        return _lib.fd_ed25519_hip_device_clock_mhz(self._h)

    # ---- device memory ----------------------------------------------------
    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)


class DeviceBuffer:
    """Device memory owned by an engine's HIP runtime."""

    def __init__(self, engine, nbytes):
        self.engine, self.nbytes = engine, int(nbytes)
        self.ptr = _lib.fd_ed25519_hip_dev_alloc(engine._h, max(self.nbytes, 1))
        if not self.ptr:
            raise HipError(f"dev_alloc({nbytes}) failed: {_lib.fd_ed25519_hip_last_error().decode()}")

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        _check(_lib.fd_ed25519_hip_memcpy(self.engine._h, self.ptr, arr.ctypes.data, arr.nbytes, 0))
        return self

    def download(self, dtype, count, offset_bytes=0):
        out = np.empty(count, dtype=dtype)
        assert offset_bytes + out.nbytes <= self.nbytes
        _check(_lib.fd_ed25519_hip_memcpy(self.engine._h, out.ctypes.data, self.ptr + offset_bytes, out.nbytes, 1))
        return out

    def download_into(self, out, offset_bytes=0):
        """D2H straight into a caller's contiguous array (e.g. a slice of a
        page-locked host window), no intermediate copy."""
        assert out.flags["C_CONTIGUOUS"] and offset_bytes + out.nbytes <= self.nbytes
        if out.nbytes:
            _check(_lib.fd_ed25519_hip_memcpy(self.engine._h, out.ctypes.data, self.ptr + offset_bytes, out.nbytes, 1))
        return out

    def free(self):
        if self.ptr:
            _lib.fd_ed25519_hip_dev_free(self.engine._h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceWorkload:
    """A signature batch resident in HBM (SoA), generated on the device."""

    def __init__(self, engine, n, lo, hi, ppm, seed, index_base=0):
        from . import workload
        self.n = n
        sizes = workload.msg_sizes(seed, index_base, n, lo, hi)
        off = workload.msg_offsets(sizes)
        self.msg_bytes = int(sizes.astype(np.uint64).sum())
        self.sizes = sizes
        self.msgs = engine.alloc(self.msg_bytes + 16)
        self.off = engine.alloc(8 * n).upload(off)
        self.sz = engine.alloc(4 * n).upload(sizes)
        self.sigs = engine.alloc(64 * n)
        self.pubs = engine.alloc(32 * n)
        self.out = engine.alloc(n)
        self.expect = engine.alloc(n)
        self.cls = engine.alloc(n)
        engine.gen_dev(n, seed, index_base, self.msgs.ptr, self.msg_bytes, self.off.ptr, self.sz.ptr, self.sigs.ptr,
                       self.pubs.ptr)
        engine.corrupt_dev(n, seed, index_base, ppm, self.msgs.ptr, self.off.ptr, self.sz.ptr, self.sigs.ptr,
                           self.pubs.ptr, self.expect.ptr, self.cls.ptr)
        engine.sync()
        self.engine = engine

    def verify(self, stream=None):
        self.engine.verify_dev(self.n, self.msgs.ptr, self.off.ptr, self.sz.ptr, self.sigs.ptr, self.pubs.ptr,
                               self.out.ptr, stream)

    def free(self):
        for b in (self.msgs, self.off, self.sz, self.sigs, self.pubs, self.out, self.expect, self.cls):
            b.free()


_lib.fd_ed25519_hip_device_count.restype = ctypes.c_int


_lib.fd_ed25519_hip_dropin_stats.argtypes = [ctypes.POINTER(ctypes.c_ulong), ctypes.POINTER(ctypes.c_ulong)]
_lib.fd_ed25519_hip_dropin_device_bytes.restype = ctypes.c_ulong
_lib.fd_ed25519_hip_shared_device_bytes.argtypes = [ctypes.c_int]
_lib.fd_ed25519_hip_shared_device_bytes.restype = ctypes.c_ulong


def dropin_stats():
    """(launches, calls): the drop-ins' combined launches and the calls they carried."""
    a, b = ctypes.c_ulong(), ctypes.c_ulong()
    _lib.fd_ed25519_hip_dropin_stats(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


DROPIN_ON_LOST_ABORT, DROPIN_ON_LOST_REJECT = 0, 1
_lib.fd_ed25519_hip_dropin_set_on_lost.argtypes = [ctypes.c_int]
_lib.fd_ed25519_hip_dropin_status.argtypes = [ctypes.POINTER(ctypes.c_ulong)]


def dropin_set_on_lost(policy):
    """The drop-ins' lost-device policy (fd_ed25519_hip_dropin_set_on_lost):
    DROPIN_ON_LOST_ABORT (default) or DROPIN_ON_LOST_REJECT; returns the previous."""
    return _lib.fd_ed25519_hip_dropin_set_on_lost(int(policy))


def dropin_status():
    """(lost, recoveries): 0 or the code that lost the device, and the launches
    that succeeded on a re-created engine (fd_ed25519_hip_dropin_status)."""
    r = ctypes.c_ulong()
    lost = _lib.fd_ed25519_hip_dropin_status(ctypes.byref(r))
    return lost, r.value


def dropin_reset():
    """Re-creates the drop-in engines (fd_ed25519_hip_dropin_reset): 0 or an error code."""
    return _lib.fd_ed25519_hip_dropin_reset()


def dropin_device_bytes():
    """Device memory the drop-ins hold: their engines plus the process's shared base tables."""
    return _lib.fd_ed25519_hip_dropin_device_bytes()


def shared_device_bytes(device=0):
    return _lib.fd_ed25519_hip_shared_device_bytes(int(device))


def device_count():
    """Visible HIP devices, from the library's own runtime."""
    return _lib.fd_ed25519_hip_device_count()
