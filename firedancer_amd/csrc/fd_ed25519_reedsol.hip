/* fd_ed25519_reedsol.hip -- the Reed-Solomon parity of a leader's FEC sets
   (include/fd_ed25519_hip.h Part 2g): what fd_shredder_next_fec_set
   (src/disco/shred/fd_shredder.c:167-223) does to a set whose data shreds
   and parity headers are filled, before the Merkle tree of
   fd_ed25519_fec.hip.  One launch, one workgroup per set:

     judge    fd_fec_core.h's rules 1-2 and fd_reedsol_core.h's rule 7 reduced
              to one code per set, as the tree kernel reduces its rules
     tables   the 8 KB of product tables and the set's rows of M_d (the
              engine's, built on the host from fd_reedsol_core.h) into LDS
     encode   the column loop of fd_reedsol_dev.h (fd_reedsol_rows) over the
              parity rows [0, p): source i is data shred i's region, at 0x40,
              target row r code shred r's, at 0x59.  The loop carries the one
              rule of its stores: no store covers a byte outside
              [0x59, 0x59 + P). */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/fd_ed25519_hip.h"
#include "fd_ed25519_hip_internal.h"
#include "fd_front_dev.h"

#define FD_SHRED_FN __device__ static inline
#include "fd_reedsol_core.h"
#include "fd_reedsol_dev.h"

/* at most 67 parity rows, in passes that start at row 0 */
#define FD_RS_ROW_MAX ( ( ( FD_REEDSOL_CORE_MAX + FD_REEDSOL_ROWS - 1 ) / FD_REEDSOL_ROWS ) * FD_REEDSOL_ROWS )

__global__ void __launch_bounds__(FD_REEDSOL_BLOCK)
fd_ed25519_fec_parity_kernel(fd_ed25519_fec_parity_params_t p) {
  __shared__ uint4 s_mul[FD_REEDSOL_CORE_MUL_BYTES / 16];        /* [256][2]: T0 T1 | T2 pad */
  __shared__ uint32_t s_coef[FD_RS_ROW_MAX * FD_REEDSOL_STRIDE / 4];   /* [row][68], zero beyond the set's d and p */
  __shared__ uint32_t s_first_bad;    /* (j << 8 | code) of the first failing shred */
  __shared__ uint32_t s_first_code;   /* the first shred that is no data shred the rules pass */
  const uint32_t k = blockIdx.x, t = threadIdx.x;
  const uint64_t first = p.set_first[k], last = p.set_first[k + 1];
  /* a set_first that is no prefix sum: a range that runs backwards or leaves [0, n) is rule 1's */
  const bool range_ok = first <= last && last <= p.n && last - first >= 1 && last - first <= FD_FEC_CORE_CNT_MAX;
  const uint32_t cnt = range_ok ? (uint32_t)(last - first) : 0u;
  if (t == 0) { s_first_bad = 0xffffffffu; s_first_code = cnt; }
  __syncthreads();
  int own = FD_FEC_CORE_OK;
  for (uint32_t j = t; j < cnt; j += FD_REEDSOL_BLOCK) {   /* cnt <= 134: one round */
    fd_shred_core_t c;
    const uint8_t* s = p.shreds + p.shred_off[first + j];
    own = fd_fec_core_judge(s, p.shred_sz[first + j], cnt, j, &c);
    if (own) atomicMin(&s_first_bad, (j << 8) | ((uint32_t)own & 0xffu));
    if (own || (s[0x40] & 0xf0u) != 0x80u) atomicMin(&s_first_code, j);
  }
  __syncthreads();
  const uint32_t d = s_first_code;
  for (uint32_t j = t; j < cnt; j += FD_REEDSOL_BLOCK) {
    if (own) continue;
    const int code = fd_reedsol_core_judge(p.shreds + p.shred_off[first + j], cnt, j, d);
    if (code) atomicMin(&s_first_bad, (j << 8) | ((uint32_t)code & 0xffu));
  }
  __syncthreads();
  const uint32_t bad = s_first_bad;
  const int set_code = !range_ok ? FD_FEC_CORE_ERR_SET : bad != 0xffffffffu ? (int)(int8_t)(bad & 0xffu) : FD_FEC_CORE_OK;
  if (t == 0) p.set_out[k] = (int8_t)set_code;
  if (set_code) return;   /* rule 8: nothing of the set's shreds is written */

  /* 1 <= d <= 67 data shreds, 1 <= np <= 67 parity shreds, every header agreeing */
  const uint32_t np = cnt - d;
  const uint32_t region = FD_REEDSOL_CORE_REGION(fd_fec_core_depth(cnt));
  const uint4* gmul = reinterpret_cast<const uint4*>(p.tab);
  for (uint32_t q = t; q < FD_REEDSOL_CORE_MUL_BYTES / 16; q += FD_REEDSOL_BLOCK) s_mul[q] = gmul[q];
  for (uint32_t q = t; q < FD_RS_ROW_MAX * FD_REEDSOL_STRIDE / 4; q += FD_REEDSOL_BLOCK) s_coef[q] = 0u;
  __syncthreads();
  const uint8_t* mat = p.tab + FD_REEDSOL_CORE_MAT_AT(d);
  uint8_t* coef8 = reinterpret_cast<uint8_t*>(s_coef);
  for (uint32_t q = t; q < np * d; q += FD_REEDSOL_BLOCK) coef8[(q / d) * FD_REEDSOL_STRIDE + q % d] = mat[q];
  __syncthreads();

  fd_reedsol_rows<true>(
      s_mul, s_coef, d, region, 0u, np,
      [&](const uint32_t i) { return p.shreds + p.shred_off[first + i] + FD_REEDSOL_CORE_DATA_AT; },
      [&](const uint32_t r) { return p.shreds + p.shred_off[first + d + r] + FD_REEDSOL_CORE_CODE_AT; });
}

extern "C" int fd_ed25519_hip_launch_fec_parity(const fd_ed25519_fec_parity_params_t* p, void* stream) {
  if (!p->n_set) return 0;
  hipLaunchKernelGGL(fd_ed25519_fec_parity_kernel, dim3((uint32_t)p->n_set), dim3(FD_REEDSOL_BLOCK), 0, (hipStream_t)stream, *p);
  return (int)hipGetLastError();
}
