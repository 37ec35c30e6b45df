/* fd_reedsol_dev.h -- the GF(2^8) product of the Reed-Solomon kernels on the
   device: four bytes of a dword times one coefficient c, from c's 20 bytes of
   fd_reedsol_core.h's product tables,

     c x = T0[ x&7 ] ^ T1[ (x>>3)&7 ] ^ T2[ x>>6 ]

   with one v_perm_b32 per table, and the column loop both kernels run over
   it (fd_reedsol_rows) with the one rule of its stores.  Included by the
   parity kernel (fd_ed25519_reedsol.hip), the recover kernel
   (fd_ed25519_recover.hip) and the test-only diag library
   (diag/fd_ed25519_diag_reedsol.hip), which runs the selector and the
   product on caller-chosen operands. */
#ifndef FD_REEDSOL_DEV_H
#define FD_REEDSOL_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fd_front_dev.h"

/* the three byte selectors of a dword x: per byte, bits 0-2, bits 3-5 and bits 6-7 */
__device__ __forceinline__ void fd_reedsol_sel(const uint32_t x, uint32_t& s0, uint32_t& s1, uint32_t& s2) {
  s0 = x & 0x07070707u; s1 = (x >> 3) & 0x07070707u; s2 = (x >> 6) & 0x03030303u;
}

/* the four products c x of x's bytes from c's 20 table bytes: t = T0 | T1, t2 = T2 */
__device__ __forceinline__ uint32_t fd_reedsol_mul(const uint4 t, const uint32_t t2, const uint32_t s0, const uint32_t s1, const uint32_t s2) {
  return __builtin_amdgcn_perm(t.y, t.x, s0) ^ __builtin_amdgcn_perm(t.w, t.z, s1) ^ __builtin_amdgcn_perm(0u, t2, s2);
}

#define FD_REEDSOL_BLOCK  256   /* lanes of a set's workgroup: 255 columns at depth 6 (32+32), 250 at depth 7 */
#define FD_REEDSOL_ROWS   32    /* target rows a pass: their accumulators live in registers */
#define FD_REEDSOL_STRIDE 68    /* a row of coefficients in LDS: 67 padded to whole dwords */

/* The column loop: target row r in [row0, row1) = sum over the sources i < d
   of coef[r][i] times source i, over the region bytes of a set's shreds.
   One lane per 4-byte column; a lane loads its column of four sources at a
   time (load4_any: the last column may reach one byte past the region, into
   the proof, inside the shred), forms each dword's three selectors once, and
   for every row of a pass reads the row's four coefficients (coef: [row]
   [FD_REEDSOL_STRIDE] bytes, zero beyond d and beyond the caller's rows up to
   the next multiple of 8 behind any pass's start) and each coefficient's
   product table (mul: fd_reedsol_core.h's, [256][2] uint4) from LDS at
   wave-uniform addresses.  FD_REEDSOL_ROWS accumulators a pass; more rows
   take more passes over the sources.  src(i) is where source i's region
   starts and dst(r) where target row r's does.  STORE writes the rows; else
   they are compared with what stands there and the differences returned.

   The write hazard is the seal's (fd_ed25519_fec.hip): shreds start at any
   byte, so the last byte of a region and the first byte of the proof behind
   it, or of the header in front, can share a dword that belongs to another
   lane or another launch.  A lane stores its column as one dword when the
   column is dword-aligned and as bytes when it is not, and the last column,
   which has three bytes (region = 3 mod 4), always as bytes: no store covers
   a byte outside the region. */
template <bool STORE, typename SRC, typename DST>
__device__ __forceinline__ uint32_t fd_reedsol_rows(const uint4* mul, const uint32_t* coef, const uint32_t d, const uint32_t region,
                                                    const uint32_t row0, const uint32_t row1, const SRC src, const DST dst) {
  const uint32_t ncol = (region + 3u) >> 2;
  uint32_t diff = 0u;
  for (uint32_t col = threadIdx.x; col < ncol; col += FD_REEDSOL_BLOCK) {
    for (uint32_t r0 = row0; r0 < row1; r0 += FD_REEDSOL_ROWS) {
      uint32_t acc[FD_REEDSOL_ROWS];
#pragma unroll
      for (int r = 0; r < FD_REEDSOL_ROWS; r++) acc[r] = 0u;
      for (uint32_t i0 = 0; i0 < d; i0 += 4) {
        uint32_t s0[4], s1[4], s2[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const uint32_t x = i0 + u < d ? load4_any(src(i0 + u) + 4u * col) : 0u;
          fd_reedsol_sel(x, s0[u], s1[u], s2[u]);
        }
#pragma unroll
        for (int g = 0; g < FD_REEDSOL_ROWS; g += 8) {
          if (r0 + g < row1) {   /* block-uniform; rows behind row1 are computed and dropped */
#pragma unroll
            for (int r = g; r < g + 8; r++) {
              const uint32_t c4 = coef[(r0 + r) * (FD_REEDSOL_STRIDE / 4) + (i0 >> 2)];
#pragma unroll
              for (int u = 0; u < 4; u++) {
                const uint32_t c = (c4 >> (8 * u)) & 0xffu;
                acc[r] ^= fd_reedsol_mul(mul[2 * c], mul[2 * c + 1].x, s0[u], s1[u], s2[u]);
              }
            }
          }
        }
      }
#pragma unroll
      for (int r = 0; r < FD_REEDSOL_ROWS; r++) {
        if (r0 + r < row1) {
          uint8_t* to = dst(r0 + r) + 4u * col;
          const uint32_t v = acc[r];
          if (!STORE) {
            diff |= (v ^ load4_any(to)) & (col + 1u < ncol ? 0xffffffffu : 0x00ffffffu);   /* region = 3 mod 4 */
          } else if (col + 1u < ncol && !(reinterpret_cast<uintptr_t>(to) & 3)) {
            *reinterpret_cast<uint32_t*>(to) = v;
          } else {
            const uint32_t nb = col + 1u < ncol ? 4u : region - 4u * col;
            for (uint32_t b = 0; b < nb; b++) to[b] = (uint8_t)(v >> (8u * b));
          }
        }
      }
    }
  }
  return diff;
}

#endif
