/* fd_ed25519_fec.hip -- sealing a leader's FEC sets (include/fd_ed25519_hip.h
   Part 2f): what fd_shredder_next_fec_set (src/disco/shred/fd_shredder.c:
   225-260) does to a set whose data and parity shreds are filled -- the
   Merkle tree over the shreds, the signature of its root, the signature and
   each shred's inclusion proof copied into the shreds -- the inverse of
   fd_ed25519_shred.hip.  Three launches:

     tree     one workgroup per set: fd_fec_core.h's rules reduced to one
              code per set, the leaf hashes (fd_sha256_dev.h) into LDS, the
              layers of the tree in LDS with a barrier between layers, then
              every lane copies its leaf's sibling nodes out of LDS into its
              shred's proof; the root goes into the workspace as the 32-byte
              message of the set's signature
     sign     fd_ed25519_sign_kernel (fd_ed25519_gen.hip) over the n_set
              roots (host/fd_ed25519_hip_fronts.c launches it)
     scatter  one lane per shred copies its set's signature into s[0..64)

   The write hazard.  Shreds may start at any byte and 1203 is odd, so shreds
   packed back to back take every alignment: the last byte of one shred's
   proof and the first byte of the next shred's signature can share a dword
   and belong to different lanes, workgroups or launches, and so can two
   leaves' proofs.  No field is therefore written by a read-modify-write of a
   dword, and no dword store covers a byte outside the lane's own 20- or
   64-byte field: fec_store_field writes the bytes up to the first dword
   boundary inside the field and those behind the last one with byte stores
   and only what lies between with dword stores. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/fd_ed25519_hip.h"
#include "fd_ed25519_hip_internal.h"
#include "fd_front_dev.h"

#define FD_SHRED_FN __device__ static inline
#include "fd_fec_core.h"

#define FD_DEV __device__ __forceinline__
#include "fd_sha256_dev.h"

/* One wave per set, looping over the leaves in rounds of 64 (a set of the
   common 32+32 shape is one round): a lane's leaf is a chain of about 18
   compressions and a layer two more for however many lanes it has, so a
   second wave would only add to the latency of a set of more than 64 leaves
   and idle for any other, and single-wave blocks spread a small batch over
   the most SIMDs.  The kernel itself is written for any
   block size. */
#ifndef FD_FEC_TREE_BLOCK
#define FD_FEC_TREE_BLOCK 64
#endif

/* a node's eight big-endian hash words in a row of nine: the pair (2t, 2t+1)
   a lane merges is 18 dwords from its neighbour's, 2-way on the 32 banks
   where rows of eight would be 16-way */
#define FD_FEC_ROW 9

/* N dwords d[0..N) (memory order, d[N] == 0) as the 4N bytes at dst, any
   byte address, touching no byte outside [dst, dst+4N): see the write
   hazard above */
template <int N>
FD_DEV void fec_store_field(uint8_t* dst, const uint32_t (&d)[N + 1]) {
  const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3);
  const uint32_t head = (4u - sh) & 3u;   /* bytes up to the first dword boundary */
  for (uint32_t b = 0; b < head; b++) dst[b] = (uint8_t)(d[0] >> (8u * b));
  uint32_t* w = reinterpret_cast<uint32_t*>(dst + head);
  const int full = sh ? N - 1 : N;
#pragma unroll
  for (int q = 0; q < N; q++)
    if (q < full) w[q] = __builtin_amdgcn_alignbyte(d[q + 1], d[q], head);
  const uint32_t tail = __builtin_amdgcn_alignbyte(d[N], d[N - 1], head);   /* its low sh bytes: the field's last */
  for (uint32_t b = 0; b < sh; b++) dst[head + 4u * (N - 1) + b] = (uint8_t)(tail >> (8u * b));
}

__global__ void __launch_bounds__(FD_FEC_TREE_BLOCK)
fd_ed25519_fec_tree_kernel(fd_ed25519_fec_tree_params_t p) {
  __shared__ uint32_t s_node[FD_FEC_CORE_NODE_MAX * FD_FEC_ROW];
  __shared__ uint32_t s_first_bad;   /* (j << 8 | code) of the first failing shred */
  const uint32_t k = blockIdx.x, t = threadIdx.x;
  const uint64_t first = p.set_first[k], last = p.set_first[k + 1];
  /* a set_first that is no prefix sum: a range that runs backwards or leaves [0, n) is rule 1's */
  const bool range_ok = first <= last && last <= p.n && last - first >= 1 && last - first <= FD_FEC_CORE_CNT_MAX;
  const uint32_t cnt = range_ok ? (uint32_t)(last - first) : 0u;
  if (t == 0) s_first_bad = 0xffffffffu;
  __syncthreads();
  for (uint32_t j = t; j < cnt; j += FD_FEC_TREE_BLOCK) {
    fd_shred_core_t c;
    const int code = fd_fec_core_judge(p.shreds + p.shred_off[first + j], p.shred_sz[first + j], cnt, j, &c);
    if (code) atomicMin(&s_first_bad, (j << 8) | ((uint32_t)code & 0xffu));
  }
  __syncthreads();
  const uint32_t bad = s_first_bad;
  const int set_code = !range_ok ? FD_FEC_CORE_ERR_SET : bad != 0xffffffffu ? (int)(int8_t)(bad & 0xffu) : FD_FEC_CORE_OK;
  uint4* rt = reinterpret_cast<uint4*>(p.roots + 32 * (uint64_t)k);
  uint4* ro = p.roots_out ? reinterpret_cast<uint4*>(p.roots_out + 32 * (uint64_t)k) : nullptr;
  if (t == 0) {
    p.msg_off[k] = 32 * (uint64_t)k;
    p.msg_sz[k] = set_code ? 0u : 32u;
    p.set_out[k] = (int8_t)set_code;
  }
  if (set_code) {   /* rule 6: nothing of the set's shreds is written; an empty message to sign, a zero root */
    if (t == 0) {
      const uint4 z = make_uint4(0u, 0u, 0u, 0u);
      rt[0] = z; rt[1] = z;
      if (ro) { ro[0] = z; ro[1] = z; }
    }
    return;
  }
  const uint32_t depth = fd_fec_core_depth(cnt);

  /* the leaves: every shred passed rule 2, so its type is 0x80 or 0x40 and its depth nibble is depth */
  for (uint32_t j = t; j < cnt; j += FD_FEC_TREE_BLOCK) {
    const uint8_t* s = p.shreds + p.shred_off[first + j];
    const bool is_data = (s[0x40] & 0xf0u) == 0x80u;
    uint32_t h[8];
    sha256_leaf(h, s, 1115u - 20u * depth + 0x18u + (is_data ? 0u : 0x19u));
#pragma unroll
    for (int i = 0; i < 8; i++) s_node[j * FD_FEC_ROW + i] = h[i];
    p.set_of[first + j] = k;
  }
  __syncthreads();

  /* the layers: node u of the next from nodes 2u and min(2u+1, m-1) */
  uint32_t at = 0u, m = cnt;
  for (uint32_t l = 0; l < depth; l++) {
    const uint32_t up = at + m, pm = (m + 1u) >> 1;
    for (uint32_t u = t; u < pm; u += FD_FEC_TREE_BLOCK) {
      const uint32_t* lp = s_node + (at + 2u * u) * FD_FEC_ROW;
      const uint32_t* rp = s_node + (at + min(2u * u + 1u, m - 1u)) * FD_FEC_ROW;
      uint32_t left[5], right[5], h[8];
#pragma unroll
      for (int i = 0; i < 5; i++) { left[i] = lp[i]; right[i] = rp[i]; }
      sha256_node_pair(h, left, right);
#pragma unroll
      for (int i = 0; i < 8; i++) s_node[(up + u) * FD_FEC_ROW + i] = h[i];
    }
    __syncthreads();
    at = up; m = pm;
  }

  if (t == 0) {   /* at: the top node */
    const uint32_t* r = s_node + at * FD_FEC_ROW;
    const uint4 lo = make_uint4(__builtin_bswap32(r[0]), __builtin_bswap32(r[1]), __builtin_bswap32(r[2]), __builtin_bswap32(r[3]));
    const uint4 hi = make_uint4(__builtin_bswap32(r[4]), __builtin_bswap32(r[5]), __builtin_bswap32(r[6]), __builtin_bswap32(r[7]));
    rt[0] = lo; rt[1] = hi;
    if (ro) { ro[0] = lo; ro[1] = hi; }
  }

  /* the proofs: node l of leaf j is layer l's node min((j>>l)^1, m_l-1) */
  for (uint32_t j = t; j < cnt; j += FD_FEC_TREE_BLOCK) {
    uint8_t* s = p.shreds + p.shred_off[first + j];
    const bool is_data = (s[0x40] & 0xf0u) == 0x80u;
    uint8_t* proof = s + (is_data ? FD_SHRED_CORE_MIN_SZ : FD_SHRED_CORE_MAX_SZ) - FD_SHRED_CORE_NODE_SZ * depth;
    uint32_t base = 0u, ml = cnt;
    for (uint32_t l = 0; l < depth; l++) {
      const uint32_t* np = s_node + (base + min((j >> l) ^ 1u, ml - 1u)) * FD_FEC_ROW;
      uint32_t d[6];
#pragma unroll
      for (int i = 0; i < 5; i++) d[i] = __builtin_bswap32(np[i]);
      d[5] = 0u;
      fec_store_field<5>(proof + FD_SHRED_CORE_NODE_SZ * l, d);
      base += ml; ml = (ml + 1u) >> 1;
    }
  }
}

/* lane i < n: shred i's signature field from its set's signature, when a set
   sealed it (set_of: the tree kernel's, ~0 for a shred of no sealed set);
   lane k < n_set: the caller's copy of set k's signature, zero for a set
   with a code */
__global__ void __launch_bounds__(256)
fd_ed25519_fec_scatter_kernel(fd_ed25519_fec_scatter_params_t p) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < p.n) {
    const uint32_t k = p.set_of[i];
    if (k < p.n_set) {
      const uint4* src = reinterpret_cast<const uint4*>(p.sigs + 64 * (uint64_t)k);
      uint32_t d[17];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint4 v = src[q];
        d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w;
      }
      d[16] = 0u;
      fec_store_field<16>(p.shreds + p.shred_off[i], d);
    }
  }
  if (p.sigs_out && i < p.n_set) {
    const uint4* src = reinterpret_cast<const uint4*>(p.sigs + 64 * i);
    uint4* dst = reinterpret_cast<uint4*>(p.sigs_out + 64 * i);   /* 16-byte aligned: fec_seal_dev checks */
    const bool ok = p.set_out[i] == 0;
#pragma unroll
    for (int q = 0; q < 4; q++) dst[q] = ok ? src[q] : make_uint4(0u, 0u, 0u, 0u);
  }
}

extern "C" int fd_ed25519_hip_launch_fec_tree(const fd_ed25519_fec_tree_params_t* p, void* stream) {
  if (!p->n_set) return 0;
  hipLaunchKernelGGL(fd_ed25519_fec_tree_kernel, dim3((uint32_t)p->n_set), dim3(FD_FEC_TREE_BLOCK), 0, (hipStream_t)stream, *p);
  return (int)hipGetLastError();
}

extern "C" int fd_ed25519_hip_launch_fec_scatter(const fd_ed25519_fec_scatter_params_t* p, void* stream) {
  return front_launch_1d(fd_ed25519_fec_scatter_kernel, 256, p->n > p->n_set ? p->n : p->n_set, stream, *p);
}

extern "C" unsigned fd_ed25519_hip_private_fec_tree_block(void) { return FD_FEC_TREE_BLOCK; }
