/* fd_ed25519_poh.hip -- a block's proof-of-history hash chain
   (include/fd_ed25519_hip.h Part 2i): what fd_runtime_poh_verify_wide_task
   (src/flamenco/runtime/fd_runtime.c:2007-2063) does to every microblock of a
   block, by fd_poh_core.h's rules.  Three launches on one stream:

     leaf   one lane per signature, so the launch is balanced whatever the
            microblocks look like: SHA-256( 0x00 || sig ) (two blocks) into
            the workspace as eight big-endian words
     tree   one wave per microblock: its slice of leaves reduced layer by
            layer to the fd_wbmtree32 root.  A slice of up to 128 leaves is
            reduced in LDS rows of nine dwords (fd_ed25519_fec.hip's layout);
            a larger one first in place in the workspace, a layer at a time,
            until 128 nodes are left: no cap on signatures
     chain  one lane per microblock: the k dependent compressions from the in
            state, the mixin with the tree's root, the comparison with the
            header's hash

   Every workgroup is one wave: the tree's barriers are then a wave's own,
   and a small batch spreads over the most SIMDs.  A wave serves one
   microblock however few signatures it has: on microblocks of 20 the tree
   launch uses 7 % of its lane slots and is most of the call; a
   sub-wave form is not built here.  A lane of the chain runs as long as its
   wave's longest k; the host wrapper orders microblocks by descending k
   before upload. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/fd_ed25519_hip.h"
#include "fd_ed25519_hip_internal.h"
#include "fd_front_dev.h"

#define FD_SHRED_FN __device__ static inline
#include "fd_shred_core.h"

#define FD_POH_FN __device__ static inline
#define FD_POH_CORE_NO_HOST 1
#include "fd_poh_core.h"

#define FD_DEV __device__ __forceinline__
#include "fd_sha256_dev.h"

#define FD_POH_ROW        9     /* a node's eight words in a row of nine: see FD_FEC_ROW */
#define FD_POH_LDS_LEAVES 128u  /* two per lane of the wave */

FD_DEV void poh_row_load(uint32_t (&x)[8], const uint32_t* row) {
  const uint4 lo = reinterpret_cast<const uint4*>(row)[0], hi = reinterpret_cast<const uint4*>(row)[1];
  x[0] = lo.x; x[1] = lo.y; x[2] = lo.z; x[3] = lo.w; x[4] = hi.x; x[5] = hi.y; x[6] = hi.z; x[7] = hi.w;
}

FD_DEV void poh_row_store(uint32_t* row, const uint32_t (&x)[8]) {
  reinterpret_cast<uint4*>(row)[0] = make_uint4(x[0], x[1], x[2], x[3]);
  reinterpret_cast<uint4*>(row)[1] = make_uint4(x[4], x[5], x[6], x[7]);
}

__global__ void __launch_bounds__(256)
fd_ed25519_poh_leaf_kernel(fd_ed25519_poh_params_t p) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= p.n_sig) return;
  const uint64_t off = p.sig_off[j];
  uint32_t h[8];
  if (fd_poh_core_inside(off, 64UL, p.buf_sz)) {
    sha256_leaf65(h, p.buf + off);
  } else {
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = 0u;
  }
  poh_row_store(p.leaves + 8 * j, h);
}

__global__ void __launch_bounds__(64)
fd_ed25519_poh_tree_kernel(fd_ed25519_poh_params_t p) {
  __shared__ uint32_t s_node[FD_POH_LDS_LEAVES * FD_POH_ROW];
  __shared__ uint32_t s_bad;
  const uint32_t i = blockIdx.x, t = threadIdx.x;
  const uint64_t first = p.sig_first[i], last = p.sig_first[i + 1];
  if (!(first < last && last <= p.n_sig)) {   /* no tree: the chain judges the range */
    if (t == 0) p.pre[i] = 0;
    return;
  }
  const uint64_t cnt = last - first;
  if (t == 0) s_bad = 0u;
  __syncthreads();
  for (uint64_t j = t; j < cnt; j += 64)
    if (!fd_poh_core_inside(p.sig_off[first + j], 64UL, p.buf_sz)) s_bad = 1u;
  __syncthreads();
  const uint32_t bad = s_bad;
  if (t == 0) p.pre[i] = (int8_t)bad;
  if (bad) return;

  /* layers of more than 128 nodes, in place: node u from nodes 2u and min(2u+1, m-1).  A round of 64 nodes reads
     places [2*base, 2*base+128) and writes [base, base+64): all its reads stand before the barrier, its writes
     behind it, and no later round reads a place an earlier one wrote */
  uint32_t* g = p.leaves + 8 * first;
  uint64_t m = cnt;
  while (m > FD_POH_LDS_LEAVES) {
    const uint64_t pm = (m + 1) >> 1;
    for (uint64_t base = 0; base < pm; base += 64) {
      const uint64_t u = base + t;
      const bool live = u < pm;
      uint32_t l[8], r[8], h[8];
      if (live) {
        const uint64_t ri = 2 * u + 1 < m ? 2 * u + 1 : m - 1;
        poh_row_load(l, g + 8 * (2 * u));
        poh_row_load(r, g + 8 * ri);
      }
      __syncthreads();
      if (live) {
        sha256_node65(h, l, r);
        poh_row_store(g + 8 * u, h);
      }
      __syncthreads();
    }
    m = pm;
  }

  /* the rest in LDS: a layer has at most one pair per lane */
  uint32_t mm = (uint32_t)m;
  for (uint32_t j = t; j < mm; j += 64) {
    uint32_t x[8];
    poh_row_load(x, g + 8 * (uint64_t)j);
#pragma unroll
    for (int q = 0; q < 8; q++) s_node[j * FD_POH_ROW + q] = x[q];
  }
  __syncthreads();
  while (mm > 1u) {
    const uint32_t pm = (mm + 1u) >> 1;
    const bool live = t < pm;
    uint32_t l[8], r[8], h[8];
    if (live) {
      const uint32_t* lp = s_node + (2u * t) * FD_POH_ROW;
      const uint32_t* rp = s_node + min(2u * t + 1u, mm - 1u) * FD_POH_ROW;
#pragma unroll
      for (int q = 0; q < 8; q++) { l[q] = lp[q]; r[q] = rp[q]; }
    }
    __syncthreads();
    if (live) {
      sha256_node65(h, l, r);
#pragma unroll
      for (int q = 0; q < 8; q++) s_node[t * FD_POH_ROW + q] = h[q];
    }
    __syncthreads();
    mm = pm;
  }
  if (t == 0) {
    uint32_t x[8];
#pragma unroll
    for (int q = 0; q < 8; q++) x[q] = s_node[q];
    poh_row_store(p.roots + 8 * (uint64_t)i, x);
  }
}

__global__ void __launch_bounds__(64)
fd_ed25519_poh_chain_kernel(fd_ed25519_poh_params_t p) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const uint64_t hdr_off = p.hdr_off[i], in_off = p.in_off[i];
  unsigned long k;
  int mixin;
  int code = fd_poh_core_judge(p.buf, p.buf_sz, hdr_off, in_off, p.sig_first[i], p.sig_first[i + 1], p.n_sig,
                               p.hash_cnt_max, &k, &mixin);
  /* parse before unsupported: the places of the signatures are the tree's to judge */
  if (code != FD_POH_CORE_ERR_PARSE && mixin && p.pre[i]) code = FD_POH_CORE_ERR_PARSE;
  uint32_t s[8];
#pragma unroll
  for (int q = 0; q < 8; q++) s[q] = 0u;
  if (!code) {
    uint32_t want[8];
    sha256_load32(s, p.buf + in_off);
    sha256_load32(want, p.buf + hdr_off + 8);
    /* no descriptor makes a launch longer than the bound allows, whatever the judge said */
    const uint32_t kk = (uint32_t)(k < p.hash_cnt_max ? k : p.hash_cnt_max);
#pragma clang loop unroll(disable)
    for (uint32_t t = 0; t < kk; t++) sha256_chain32(s);
    if (mixin) {
      uint32_t root[8];
      poh_row_load(root, p.roots + 8 * i);
      sha256_mix64(s, root);
    }
    uint32_t diff = 0u;
#pragma unroll
    for (int q = 0; q < 8; q++) diff |= s[q] ^ want[q];
    if (diff) code = FD_POH_CORE_ERR_HASH;
  }
  p.out[i] = (int8_t)code;
  if (p.out_hash) {
    uint4* o = reinterpret_cast<uint4*>(p.out_hash + 32 * i);
    o[0] = make_uint4(__builtin_bswap32(s[0]), __builtin_bswap32(s[1]), __builtin_bswap32(s[2]), __builtin_bswap32(s[3]));
    o[1] = make_uint4(__builtin_bswap32(s[4]), __builtin_bswap32(s[5]), __builtin_bswap32(s[6]), __builtin_bswap32(s[7]));
  }
}

/* tools/poh_bench.py mirrors the parameter block to time the launches one by one, and holds its copy to this */
extern "C" unsigned fd_ed25519_hip_private_poh_params_bytes(void) { return (unsigned)sizeof(fd_ed25519_poh_params_t); }

extern "C" int fd_ed25519_hip_launch_poh_leaf(const fd_ed25519_poh_params_t* p, void* stream) {
  return front_launch_1d(fd_ed25519_poh_leaf_kernel, 256, p->n_sig, stream, *p);
}

extern "C" int fd_ed25519_hip_launch_poh_tree(const fd_ed25519_poh_params_t* p, void* stream) {
  if (!p->n) return 0;
  hipLaunchKernelGGL(fd_ed25519_poh_tree_kernel, dim3((uint32_t)p->n), dim3(64), 0, (hipStream_t)stream, *p);
  return (int)hipGetLastError();
}

extern "C" int fd_ed25519_hip_launch_poh_chain(const fd_ed25519_poh_params_t* p, void* stream) {
  return front_launch_1d(fd_ed25519_poh_chain_kernel, 64, p->n, stream, *p);
}
