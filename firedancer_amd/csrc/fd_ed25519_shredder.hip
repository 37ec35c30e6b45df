/* fd_ed25519_shredder.hip -- the front of the leader's shred path
   (include/fd_ed25519_hip.h Part 2j): what fd_shredder_next_fec_set
   (src/disco/shred/fd_shredder.c:145-221) does to an entry batch before the
   parity of fd_ed25519_reedsol.hip and the tree of fd_ed25519_fec.hip.  One
   launch, one workgroup per set and, behind them, a lane per batch:

     find     the batch that reserved the set, by a search in set_first_b
     judge    fd_shredder_core.h's rule 5 on the batch; a batch with a code
              gets no shred, its first set the whole shred reservation as its
              range and its other sets an empty one
     plan     the set's bytes, d, p, depth and indices (rules 1-4); lane j
              writes shred j's shred_off and shred_sz and its header bytes
              [0x40, 0x58) or [0x40, 0x59) into LDS
     copy     a lane per dword of a shred: the value of the four bytes -- zero,
              header bytes from LDS, batch bytes from aligned dword loads and
              v_alignbyte (load4_any), zero fill -- and one store by the rule
              of fd_reedsol_dev.h: the dword where it lies inside the field,
              bytes at a field's ends.  Dwords are counted from the dword that
              holds the field's first byte, so every store inside a field is
              dword-aligned whatever the shred's address, and no store covers a
              byte outside [0, 1203) of a data shred, [0, 0x59) and the proof
              field of a parity shred. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/fd_ed25519_hip.h"
#include "fd_ed25519_hip_internal.h"
#include "fd_front_dev.h"

#define FD_SHRED_FN __device__ static inline
#include "fd_shredder_core.h"

#define FD_SHREDDER_BLOCK    256
#define FD_SHREDDER_DATA_W   302   /* dwords that hold 1203 bytes from any byte of a dword on: ( 1203 + 3 + 3 ) / 4 */
#define FD_SHREDDER_CODE_W    64   /* a parity shred's: 23 for [0, 0x59), ( 0x59 + 6 ) / 4, and up to 41 for a proof of 160 bytes */
#define FD_SHREDDER_CODE_HDR_W 23
#define FD_SHREDDER_HDR_ROW   32   /* a shred's header bytes in LDS */

static_assert(sizeof(fd_shredder_core_desc_t) == 24 && sizeof(fd_ed25519_hip_shredder_batch_t) == 24, "descriptor");

/* bytes [pos, pos + 4) of shred s, s + pos dword-aligned, from v: those inside [lo, hi) */
__device__ static inline void shredder_put4(uint8_t* s, const int pos, const int lo, const int hi, const uint32_t v) {
  uint8_t* to = s + pos;
  if (pos >= lo && pos + 4 <= hi) {
    *reinterpret_cast<uint32_t*>(to) = v;
  } else {
    for (int b = 0; b < 4; b++)
      if (pos + b >= lo && pos + b < hi) to[b] = (uint8_t)(v >> (8 * b));
  }
}

/* the header bytes of [pos, pos + 4) that lie in [0x40, end) */
__device__ static inline uint32_t shredder_hdr4(const uint8_t* row, const int pos, const int end) {
  uint32_t v = 0u;
  for (int b = 0; b < 4; b++) {
    const int at = pos + b;
    if (at >= 0x40 && at < end) v |= (uint32_t)row[at - 0x40] << (8 * b);
  }
  return v;
}

__device__ static inline int shredder_judge(const fd_ed25519_shredder_params_t& p, const uint64_t b) {
  return fd_shredder_core_judge(p.batch_off[b], p.batch_sz[b], p.buf_sz, p.set_first_b[b], p.set_first_b[b + 1], p.n_set,
                                p.shred_first_b[b], p.shred_first_b[b + 1], p.n);
}

__global__ void __launch_bounds__(FD_SHREDDER_BLOCK)
fd_ed25519_shredder_kernel(fd_ed25519_shredder_params_t p) {
  __shared__ uint8_t s_hdr[FD_FEC_CORE_CNT_MAX][FD_SHREDDER_HDR_ROW];
  const uint32_t t = threadIdx.x;
  if (blockIdx.x >= p.set_cnt) {   /* the batches' codes, and the end of set_first */
    const uint64_t b = (uint64_t)(blockIdx.x - p.set_cnt) * FD_SHREDDER_BLOCK + t;
    if (b < p.nb && p.batch_out) p.batch_out[b] = (int8_t)shredder_judge(p, b);
    if (b == 0) p.set_first[p.set_cnt] = (uint32_t)p.m;
    return;
  }
  const uint64_t kk = blockIdx.x, k = p.set0 + kk;
  /* the last batch whose reservation starts at or before set k */
  uint64_t lo = 0, hi = p.nb;
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (p.set_first_b[mid] <= k) lo = mid; else hi = mid;
  }
  const uint64_t b = lo;
  const uint64_t s0 = p.set_first_b[b], s1 = p.set_first_b[b + 1], h0 = p.shred_first_b[b], h1 = p.shred_first_b[b + 1];
  if (!(s0 <= k && k < s1)) {   /* no batch owns the set */
    if (t == 0) p.set_first[kk] = (uint32_t)(p.n - p.shred0);
    return;
  }
  if (p.privs && t < 8) reinterpret_cast<uint32_t*>(p.keys)[8 * kk + t] = reinterpret_cast<const uint32_t*>(p.privs)[8 * b + t];
  if (shredder_judge(p, b)) {
    const uint64_t h = k == s0 ? h0 : h1;
    if (t == 0) p.set_first[kk] = (uint32_t)((h < p.n ? h : p.n) - p.shred0);
    return;
  }

  const fd_shredder_core_desc_t desc = reinterpret_cast<const fd_shredder_core_desc_t*>(p.desc)[b];
  fd_shredder_core_plan_t pl;
  fd_shredder_core_plan(p.batch_sz[b], k - s0, desc.data_idx, desc.parity_idx, &pl);
  /* the batch's shreds are [h0, h1) = rule 2's counts, so the set's lie in them and in the launch's [shred0, shred0 + m) */
  const uint64_t first = h0 + pl.shred0 - p.shred0;
  const uint32_t d = pl.d, np = pl.p, cnt = d + np;
  if (t == 0) p.set_first[kk] = (uint32_t)first;
  for (uint32_t j = t; j < cnt; j += FD_SHREDDER_BLOCK) {
    p.shred_off[first + j] = p.base_off + p.stride * (first + j);
    p.shred_sz[first + j] = j < d ? FD_SHRED_CORE_MIN_SZ : FD_SHRED_CORE_MAX_SZ;
    if (j < d) fd_shredder_core_data_hdr(s_hdr[j], &desc, &pl, j);
    else       fd_shredder_core_code_hdr(s_hdr[j], &desc, &pl, j - d);
  }
  __syncthreads();

  /* the data shreds: dword w of shred i covers its bytes [4 w - a, 4 w - a + 4), a the shred's address mod 4 */
  const uint8_t* src = p.buf + p.batch_off[b] + pl.off - (b == p.skip_b ? p.skip : 0);
  for (uint32_t it = t; it < d * FD_SHREDDER_DATA_W; it += FD_SHREDDER_BLOCK) {
    const uint32_t i = it / FD_SHREDDER_DATA_W, w = it - i * FD_SHREDDER_DATA_W;
    uint8_t* s = p.shreds + p.base_off + p.stride * (first + i);
    const int pos = 4 * (int)w - (int)(reinterpret_cast<uintptr_t>(s) & 3);
    if (pos >= (int)FD_SHRED_CORE_MIN_SZ) continue;
    const int n = (int)fd_shredder_core_payload(&pl, i);
    uint32_t v = 0u;
    if (pos + 4 > 0x40 && pos < (int)FD_SHRED_CORE_DATA_HDR_SZ) v = shredder_hdr4(s_hdr[i], pos, (int)FD_SHRED_CORE_DATA_HDR_SZ);
    const int rel = pos - (int)FD_SHRED_CORE_DATA_HDR_SZ;
    if (rel > -4 && rel < n) {   /* batch bytes [from, min( rel + 4, n )) of the shred's n */
      const int from = rel < 0 ? 0 : rel, keep = n - from;
      uint32_t x = load4_any(src + (uint64_t)i * pl.payload + from);
      if (keep < 4) x &= (1u << (8 * keep)) - 1u;
      v |= rel < 0 ? x << (8 * -rel) : x;
    }
    shredder_put4(s, pos, 0, (int)FD_SHRED_CORE_MIN_SZ, v);
  }

  /* the parity shreds: [0, 0x59), then the proof field from the dword that holds its first byte */
  const int proof = (int)(FD_SHRED_CORE_MAX_SZ - 20u * pl.depth);
  for (uint32_t it = t; it < np * FD_SHREDDER_CODE_W; it += FD_SHREDDER_BLOCK) {
    const uint32_t j = it / FD_SHREDDER_CODE_W, w = it % FD_SHREDDER_CODE_W;
    uint8_t* s = p.shreds + p.base_off + p.stride * (first + d + j);
    if (w < FD_SHREDDER_CODE_HDR_W) {
      const int pos = 4 * (int)w - (int)(reinterpret_cast<uintptr_t>(s) & 3);
      if (pos >= (int)FD_SHRED_CORE_CODE_HDR_SZ) continue;
      shredder_put4(s, pos, 0, (int)FD_SHRED_CORE_CODE_HDR_SZ, shredder_hdr4(s_hdr[d + j], pos, (int)FD_SHRED_CORE_CODE_HDR_SZ));
    } else {
      const int pos = proof + 4 * (int)(w - FD_SHREDDER_CODE_HDR_W) - (int)(reinterpret_cast<uintptr_t>(s + proof) & 3);
      if (pos >= (int)FD_SHRED_CORE_MAX_SZ) continue;
      shredder_put4(s, pos, proof, (int)FD_SHRED_CORE_MAX_SZ, 0u);
    }
  }
}

extern "C" int fd_ed25519_hip_launch_shredder(const fd_ed25519_shredder_params_t* p, void* stream) {
  if (!p->nb) return 0;
  const uint64_t blocks = p->set_cnt + (p->nb + FD_SHREDDER_BLOCK - 1) / FD_SHREDDER_BLOCK;
  hipLaunchKernelGGL(fd_ed25519_shredder_kernel, dim3((uint32_t)blocks), dim3(FD_SHREDDER_BLOCK), 0, (hipStream_t)stream, *p);
  return (int)hipGetLastError();
}
