/* fd_ed25519_reedsol.hip -- the Reed-Solomon parity of a leader's FEC sets
   (include/fd_ed25519_hip.h Part 2g): what fd_shredder_next_fec_set
   (src/disco/shred/fd_shredder.c:167-223) does to a set whose data shreds
   and parity headers are filled, before the Merkle tree of
   fd_ed25519_fec.hip.  One launch, one workgroup per set:

     judge    fd_fec_core.h's rules 1-2 and fd_reedsol_core.h's rule 7 reduced
              to one code per set, as the tree kernel reduces its rules
     tables   the 8 KB of product tables and the set's rows of M_d (the
              engine's, built on the host from fd_reedsol_core.h) into LDS
     encode   one lane per 4-byte column of the protected region; a lane
              loads its column of four data shreds at a time, forms each
              dword's three byte selectors once, and for every parity row
              reads the row's four coefficients and each coefficient's
              product table from LDS at wave-uniform addresses (a broadcast)
              and looks the four bytes' products up with three v_perm_b32:
              c x = T0[ x&7 ] ^ T1[ (x>>3)&7 ] ^ T2[ x>>6 ].  FD_RS_ROWS
              accumulators a pass; a set of more parity shreds takes more
              passes over its data.

   The write hazard is the seal's (fd_ed25519_fec.hip): shreds start at any
   byte, so the last byte of a region and the first byte of the proof behind
   it, or of the header in front, can share a dword that belongs to another
   lane or another launch.  A lane stores its column as one dword when the
   column is dword-aligned and as bytes when it is not, and the last column,
   which has three bytes (P = 3 mod 4), always as bytes: no store covers a
   byte outside [0x59, 0x59 + P). */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/fd_ed25519_hip.h"
#include "fd_ed25519_hip_internal.h"
#include "fd_front_dev.h"

#define FD_SHRED_FN __device__ static inline
#include "fd_reedsol_core.h"
#include "fd_reedsol_dev.h"

#define FD_RS_BLOCK  256   /* 255 columns at depth 6 (32+32), 250 at depth 7 */
#define FD_RS_ROWS   32    /* parity rows a pass: their accumulators live in registers */
#define FD_RS_STRIDE 68    /* a row of coefficients in LDS: 67 padded to whole dwords */
#define FD_RS_ROW_MAX ( ( ( FD_REEDSOL_CORE_MAX + FD_RS_ROWS - 1 ) / FD_RS_ROWS ) * FD_RS_ROWS )

__global__ void __launch_bounds__(FD_RS_BLOCK)
fd_ed25519_fec_parity_kernel(fd_ed25519_fec_parity_params_t p) {
  __shared__ uint4 s_mul[FD_REEDSOL_CORE_MUL_BYTES / 16];        /* [256][2]: T0 T1 | T2 pad */
  __shared__ uint32_t s_coef[FD_RS_ROW_MAX * FD_RS_STRIDE / 4];   /* [row][68], zero beyond the set's d and p */
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
  for (uint32_t j = t; j < cnt; j += FD_RS_BLOCK) {   /* cnt <= 134: one round */
    fd_shred_core_t c;
    const uint8_t* s = p.shreds + p.shred_off[first + j];
    own = fd_fec_core_judge(s, p.shred_sz[first + j], cnt, j, &c);
    if (own) atomicMin(&s_first_bad, (j << 8) | ((uint32_t)own & 0xffu));
    if (own || (s[0x40] & 0xf0u) != 0x80u) atomicMin(&s_first_code, j);
  }
  __syncthreads();
  const uint32_t d = s_first_code;
  for (uint32_t j = t; j < cnt; j += FD_RS_BLOCK) {
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
  const uint32_t ncol = (region + 3u) >> 2;
  const uint4* gmul = reinterpret_cast<const uint4*>(p.tab);
  for (uint32_t q = t; q < FD_REEDSOL_CORE_MUL_BYTES / 16; q += FD_RS_BLOCK) s_mul[q] = gmul[q];
  for (uint32_t q = t; q < FD_RS_ROW_MAX * FD_RS_STRIDE / 4; q += FD_RS_BLOCK) s_coef[q] = 0u;
  __syncthreads();
  const uint8_t* mat = p.tab + FD_REEDSOL_CORE_MAT_AT(d);
  uint8_t* coef8 = reinterpret_cast<uint8_t*>(s_coef);
  for (uint32_t q = t; q < np * d; q += FD_RS_BLOCK) coef8[(q / d) * FD_RS_STRIDE + q % d] = mat[q];
  __syncthreads();

  for (uint32_t col = t; col < ncol; col += FD_RS_BLOCK) {
    for (uint32_t r0 = 0; r0 < np; r0 += FD_RS_ROWS) {
      uint32_t acc[FD_RS_ROWS];
#pragma unroll
      for (int r = 0; r < FD_RS_ROWS; r++) acc[r] = 0u;
      for (uint32_t i0 = 0; i0 < d; i0 += 4) {
        uint32_t s0[4], s1[4], s2[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          /* a column of the last data shred may reach one byte into its proof: inside the shred */
          const uint32_t x = i0 + u < d ? load4_any(p.shreds + p.shred_off[first + i0 + u] + FD_REEDSOL_CORE_DATA_AT + 4u * col) : 0u;
          fd_reedsol_sel(x, s0[u], s1[u], s2[u]);
        }
#pragma unroll
        for (int g = 0; g < FD_RS_ROWS; g += 8) {
          if (r0 + g < np) {   /* block-uniform: the rows past np have zero coefficients all the same */
#pragma unroll
            for (int r = g; r < g + 8; r++) {
              const uint32_t c4 = s_coef[(r0 + r) * (FD_RS_STRIDE / 4) + (i0 >> 2)];
#pragma unroll
              for (int u = 0; u < 4; u++) {
                const uint32_t c = (c4 >> (8 * u)) & 0xffu;
                acc[r] ^= fd_reedsol_mul(s_mul[2 * c], s_mul[2 * c + 1].x, s0[u], s1[u], s2[u]);
              }
            }
          }
        }
      }
#pragma unroll
      for (int r = 0; r < FD_RS_ROWS; r++) {
        if (r0 + r < np) {
          uint8_t* dst = p.shreds + p.shred_off[first + d + r0 + r] + FD_REEDSOL_CORE_CODE_AT + 4u * col;
          const uint32_t v = acc[r];
          if (col + 1u < ncol && !(reinterpret_cast<uintptr_t>(dst) & 3)) {
            *reinterpret_cast<uint32_t*>(dst) = v;
          } else {
            const uint32_t nb = col + 1u < ncol ? 4u : region - 4u * col;
            for (uint32_t b = 0; b < nb; b++) dst[b] = (uint8_t)(v >> (8u * b));
          }
        }
      }
    }
  }
}

extern "C" int fd_ed25519_hip_launch_fec_parity(const fd_ed25519_fec_parity_params_t* p, void* stream) {
  if (!p->n_set) return 0;
  hipLaunchKernelGGL(fd_ed25519_fec_parity_kernel, dim3((uint32_t)p->n_set), dim3(FD_RS_BLOCK), 0, (hipStream_t)stream, *p);
  return (int)hipGetLastError();
}
