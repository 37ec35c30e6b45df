/* fd_ed25519_txn.hip -- raw transaction payloads straight to the verify
   phases (GPU-side fd_txn_parse).

   The host copies frags as they come (payload bytes + offset/size per
   transaction) and reads one byte per transaction: the signature count
   (byte 0; a payload fd_txn_parse accepts has 1..127 signatures there), to
   reserve its signature slots.  On the device, one lane per transaction:

     stage   fd_txn_parse (fd_txn_parse_core.h, the same source the host
             library compiles), with the first 64 bytes of its fd_txn_t
             (the trailer the tile publishes) and, if accepted, the gather of its
             signatures and signer keys into the aligned SoA the verify
             phases read, with every signature's message pointing at the
             payload's message bytes in place (message_off .. end,
             fd_verify.h:57-60)
     finish fd_ed25519_verify_batch_single_msg's combine per transaction,
             with FD_ED25519_TXN_PARSE_FAILED for payloads the parser
             rejected (after_frag's filter, fd_verify.c:117-121)

   The Ed25519 precompile instructions of the same payloads
   (fd_precompile_ed25519_verify, fd_precompile_core.h) take the same
   three passes, one lane per transaction again: precompile_stage parses,
   walks the offsets tables and gathers every entry's signature and key
   (its message stays in place in the payload), the verify phases run over
   the entries, precompile_finish applies the sequential priority. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/fd_ed25519_hip_tile.h"
#include "fd_ed25519_hip_internal.h"
#include "fd_front_dev.h"

#define FD_TXN_FN __device__ static inline
#include "fd_txn_parse_core.h"
#include "fd_precompile_core.h"

/* FD_ED25519_SUCCESS / ERR_* come from fd_ed25519_hip.h (via the tile header) */
static_assert(FD_ED25519_TXN_PARSE_FAILED_CODE == FD_ED25519_HIP_TXN_CODE_PARSE_FAILED, "parse-failure code");

__global__ void __launch_bounds__(256)
fd_ed25519_txn_stage_kernel(fd_ed25519_txn_stage_params_t p) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.ntxn) return;
  const uint8_t* pay = p.payloads + p.pay_off[t];
  const uint32_t sz = p.pay_sz[t];
  fd_ed25519_hip_txn_t tx;
  const uint32_t cnt = p.txn_cnt[t];
  /* the host reserved cnt signature slots from its own read of the
     signature count; the copy parsed here may differ from that read when
     the payload sat in a room the tile can still write (zero-copy).  The
     slots are filled from this parse's offsets, so a count that disagrees
     with the host's -- or an account list shorter than it -- is a parse
     failure: nothing is read past what this parse validated */
  const int good = fd_txn_core_parse(pay, sz, &tx, p.trailer ? p.trailer + 64 * t : nullptr, 64) != 0 &&
                   (uint32_t)tx.signature_cnt == cnt && (uint32_t)tx.acct_addr_cnt >= cnt;
  p.parse_ok[t] = (uint8_t)good;
  const uint32_t slots = (cnt >= 1u && cnt <= 16u) ? cnt : 0u;  /* the host reserved these */
  const uint32_t first = p.txn_first[t];
  for (uint32_t j = 0; j < slots; j++) {
    const uint64_t k = first + j;
    uint4* sg = reinterpret_cast<uint4*>(p.sigs + 64 * k);
    uint4* pk = reinterpret_cast<uint4*>(p.pubs + 32 * k);
    if (good) {
      const uint8_t* s = pay + tx.signature_off + 64u * j;
      const uint8_t* a = pay + tx.acct_addr_off + 32u * j;
      FRONT_SLOT_GATHER(sg, pk, s, a);
      p.msg_off[k] = p.pay_off[t] + tx.message_off;
      p.msg_sz[k] = sz - tx.message_off;
    } else {
      FRONT_SLOT_ZERO(sg, pk);
      p.msg_off[k] = p.pay_off[t];
      p.msg_sz[k] = 0u;
    }
  }
}

/* per-transaction code: parse failure, else the batch_single_msg priority
   (the first phase-1 error in signature order, then ERR_MSG) */
__global__ void __launch_bounds__(256)
fd_ed25519_txn_finish_kernel(const int8_t* sig_codes, const uint32_t* txn_first, const uint32_t* txn_cnt,
                             const uint8_t* parse_ok, int8_t* out, uint64_t ntxn) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntxn) return;
  int code = FD_ED25519_SUCCESS;
  const uint32_t f = txn_first[t], n = txn_cnt[t];
  if (parse_ok && !parse_ok[t]) {
    code = FD_ED25519_TXN_PARSE_FAILED_CODE;
  } else if (n == 0u || n > 16u) {
    code = FD_ED25519_ERR_SIG;
  } else {
    bool msg_fail = false;
    for (uint32_t j = 0; j < n; j++) {
      const int c = sig_codes[f + j];
      if (c == FD_ED25519_ERR_MSG) msg_fail = true;
      else if (c != FD_ED25519_SUCCESS) { code = c; break; }
    }
    if (code == FD_ED25519_SUCCESS && msg_fail) code = FD_ED25519_ERR_MSG;
  }
  out[t] = (int8_t)code;
}

extern "C" int fd_ed25519_hip_launch_txn_stage(const fd_ed25519_txn_stage_params_t* p, void* stream) {
  return front_launch_1d(fd_ed25519_txn_stage_kernel, 256, p->ntxn, stream, *p);
}

extern "C" int fd_ed25519_hip_launch_txn_finish(const int8_t* d_sig_codes, const uint32_t* d_txn_first,
                                                const uint32_t* d_txn_cnt, const uint8_t* d_parse_ok,
                                                int8_t* d_txn_out, uint64_t ntxn, void* stream) {
  return front_launch_1d(fd_ed25519_txn_finish_kernel, 256, ntxn, stream, d_sig_codes, d_txn_first, d_txn_cnt, d_parse_ok,
                         d_txn_out, ntxn);
}

/* ---- Ed25519 precompile instructions --------------------------------- */

/* hdr_pos and a transaction's entry count travel in a byte */
static_assert(FD_PRECOMPILE_CORE_ENT_MAX <= 255UL, "entry counts fit a byte");
/* the instruction table's words hold two offsets below 2^16, its mask one bit per instruction */
static_assert(FD_TXN_CORE_MTU < 65536UL && FD_TXN_CORE_INSTR_MAX <= 64UL, "instruction table layout");

/* one wave per block: a lane's instruction table is a column of LDS, word
   j at tab[j * BLOCK + lane] (lanes reading one j hit 64 distinct banks):
   64 instructions x 64 lanes x 4 B = 16 KiB a block */
#define FD_PRECOMPILE_STAGE_BLOCK 64
static_assert(FD_TXN_CORE_INSTR_MAX * FD_PRECOMPILE_STAGE_BLOCK * 4UL <= 16384UL, "stage LDS");

/* the slots ent_first reserves for transaction t: [*first, *first + n), n
   at most ENT_MAX and inside [0, n_ent) -- or -1 when ent_first does not
   describe such a range (then no slot of t is touched) */
__device__ static inline int precompile_slots(const uint32_t* ent_first, uint64_t t, uint64_t n_ent, uint32_t* first) {
  const uint32_t f = ent_first[t], l = ent_first[t + 1];
  *first = f;
  if (l < f || (uint64_t)l > n_ent || l - f > (uint32_t)FD_PRECOMPILE_CORE_ENT_MAX) return -1;
  return (int)(l - f);
}

__global__ void __launch_bounds__(FD_PRECOMPILE_STAGE_BLOCK)
fd_ed25519_precompile_stage_kernel(fd_ed25519_precompile_stage_params_t p) {
  __shared__ unsigned tab_all[FD_TXN_CORE_INSTR_MAX * FD_PRECOMPILE_STAGE_BLOCK];
  const uint64_t t = (uint64_t)blockIdx.x * FD_PRECOMPILE_STAGE_BLOCK + threadIdx.x;
  if (t >= p.ntxn) return;
  unsigned* tab = tab_all + threadIdx.x;
  const uint64_t base = p.pay_off[t];
  const uint8_t* pay = p.payloads + base;
  const uint32_t sz = p.pay_sz[t];
  uint32_t first;
  const int reserved = precompile_slots(p.ent_first, t, p.n_ent, &first);
  const uint32_t slots = reserved < 0 ? 0u : (uint32_t)reserved;
  fd_ed25519_hip_txn_t tx;
  fd_precompile_core_sum_t sum;
  sum.ent_cnt = 0u; sum.hdr_instr = 0xFF; sum.hdr_pos = 0;
  unsigned long mask = 0UL;
  int status = 0;
  if (!fd_txn_core_parse(pay, sz, &tx, nullptr, 0)) {
    status = FD_ED25519_HIP_PRECOMPILE_PARSE_FAILED;
  } else {
    mask = fd_precompile_core_table(pay, &tx, tab, FD_PRECOMPILE_STAGE_BLOCK);
    fd_precompile_core_summary(pay, tab, FD_PRECOMPILE_STAGE_BLOCK, tx.instr_cnt, mask, &sum);
    /* the slots are filled from this walk, so a reservation made from
       another count (a payload changed since the host counted it) fills
       none of them */
    if (reserved < 0 || sum.ent_cnt != slots) status = FD_ED25519_HIP_PRECOMPILE_BAD_RESERVATION;
  }
  p.status[t] = (int8_t)status;
  p.hdr_instr[t] = sum.hdr_instr;
  p.hdr_pos[t] = sum.hdr_pos;
  if (status) {
    for (uint32_t j = 0; j < slots; j++) {
      const uint64_t k = (uint64_t)first + j;
      uint4* sg = reinterpret_cast<uint4*>(p.sigs + 64 * k);
      uint4* pk = reinterpret_cast<uint4*>(p.pubs + 32 * k);
      FRONT_SLOT_ZERO(sg, pk);
      p.msg_off[k] = base;
      p.msg_sz[k] = 0u;
      p.pre[k] = (int8_t)status;
      p.ent_instr[k] = 0xFF;
    }
    return;
  }
  /* k ends at first + slots, the summary having counted the same headers;
     the bound holds even if the payload's bytes change under the kernel */
  uint64_t k = first;
  const uint64_t k_end = (uint64_t)first + slots;
  for (unsigned j = 0; j < (unsigned)tx.instr_cnt; j++) {
    if (!((mask >> j) & 1UL)) continue;
    const unsigned w = tab[j * FD_PRECOMPILE_STAGE_BLOCK];
    const int h = fd_precompile_core_header(pay + FD_PRECOMPILE_CORE_TAB_OFF(w), FD_PRECOMPILE_CORE_TAB_SZ(w));
    for (int i = 0; i < h && k < k_end; i++, k++) {
      fd_precompile_core_ent_t ent;
      fd_precompile_core_entry(pay, tab, FD_PRECOMPILE_STAGE_BLOCK, tx.instr_cnt, j, (unsigned)i, &ent);
      uint4* sg = reinterpret_cast<uint4*>(p.sigs + 64 * k);
      uint4* pk = reinterpret_cast<uint4*>(p.pubs + 32 * k);
      if (!ent.pre) {
        const uint8_t* s = pay + ent.sig_off;
        const uint8_t* a = pay + ent.pub_off;
        FRONT_SLOT_GATHER(sg, pk, s, a);
      } else {
        FRONT_SLOT_ZERO(sg, pk);
      }
      p.msg_off[k] = base + ent.msg_off;
      p.msg_sz[k] = ent.msg_sz;
      p.pre[k] = ent.pre;
      p.ent_instr[k] = ent.instr;
    }
  }
}

/* per-transaction code: the first failure in instruction order, and within
   an instruction in entry order (an entry's equation failure ahead of the
   next entry's bad offset: not batch_single_msg's two phases); a header
   failure sits between the entries of the instructions around it */
__global__ void __launch_bounds__(256)
fd_ed25519_precompile_finish_kernel(fd_ed25519_precompile_finish_params_t p) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.ntxn) return;
  uint32_t first;
  const int reserved = precompile_slots(p.ent_first, t, p.n_ent, &first);
  const uint32_t slots = reserved < 0 ? 0u : (uint32_t)reserved;
  int code = p.status[t];
  unsigned instr = 0xFF;
  if (code) {
    if (p.ent_out)
      for (uint32_t j = 0; j < slots; j++) p.ent_out[(uint64_t)first + j] = (int8_t)code;
  } else {
    const unsigned hdr_instr = p.hdr_instr[t], hdr_pos = p.hdr_pos[t];
    for (uint32_t j = 0; j <= slots; j++) {
      if (!code && hdr_instr != 0xFF && j == hdr_pos) {
        code = FD_ED25519_HIP_PRECOMPILE_ERR_INSTR_DATA_SIZE;
        instr = hdr_instr;
      }
      if (j == slots) break;
      const uint64_t k = (uint64_t)first + j;
      const int c = p.pre[k] ? FD_ED25519_HIP_PRECOMPILE_ERR_DATA_OFFSET
                  : p.codes[k] != FD_ED25519_SUCCESS ? FD_ED25519_HIP_PRECOMPILE_ERR_SIGNATURE : 0;
      if (p.ent_out) p.ent_out[k] = (int8_t)c;
      if (!code && c) {
        code = c;
        instr = p.ent_instr[k];
      }
    }
  }
  p.txn_out[t] = (int8_t)code;
  p.instr_out[t] = (uint8_t)instr;
}

extern "C" int fd_ed25519_hip_launch_precompile_stage(const fd_ed25519_precompile_stage_params_t* p, void* stream) {
  return front_launch_1d(fd_ed25519_precompile_stage_kernel, FD_PRECOMPILE_STAGE_BLOCK, p->ntxn, stream, *p);
}

extern "C" int fd_ed25519_hip_launch_precompile_finish(const fd_ed25519_precompile_finish_params_t* p, void* stream) {
  return front_launch_1d(fd_ed25519_precompile_finish_kernel, 256, p->ntxn, stream, *p);
}

/* fd_ed25519_hip_launch_pull (fd_ed25519_hip_internal.h): blockIdx.y picks
   the span, the x blocks stride over its 16-byte words; the last n % 16
   bytes are copied one by one (never a byte past the span: a span can end
   at the last byte of a registered mapping). */
__global__ void __launch_bounds__(256)
fd_ed25519_pull_kernel(fd_ed25519_pull_params_t p) {
  const uint32_t k = blockIdx.y;
  if (k >= p.cnt) return;
  const uint8_t* src = p.src[k];
  uint8_t* dst = p.dst[k];
  const uint64_t n = p.n[k], n16 = n / 16u;
  const uint4* s4 = reinterpret_cast<const uint4*>(src);
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * blockDim.x)
    d4[i] = s4[i];
  if (blockIdx.x == 0 && threadIdx.x < (n & 15u)) dst[16u * n16 + threadIdx.x] = src[16u * n16 + threadIdx.x];
}

extern "C" int fd_ed25519_hip_launch_pull(const fd_ed25519_pull_params_t* p, void* stream) {
  if (!p->cnt) return 0;
  uint64_t most = 0;
  for (uint32_t k = 0; k < p->cnt; k++) most = p->n[k] > most ? p->n[k] : most;
  /* ~8 words per thread, at most 256 blocks per span */
  uint64_t blocks = (most / 16u + 2047u) / 2048u;
  blocks = blocks < 1u ? 1u : blocks > 256u ? 256u : blocks;
  hipLaunchKernelGGL(fd_ed25519_pull_kernel, dim3((uint32_t)blocks, p->cnt), dim3(256), 0, (hipStream_t)stream, *p);
  return (int)hipGetLastError();
}
