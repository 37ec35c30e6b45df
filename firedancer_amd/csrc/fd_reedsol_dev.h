/* fd_reedsol_dev.h -- the GF(2^8) product of the Reed-Solomon kernels on the
   device: four bytes of a dword times one coefficient c, from c's 20 bytes of
   fd_reedsol_core.h's product tables,

     c x = T0[ x&7 ] ^ T1[ (x>>3)&7 ] ^ T2[ x>>6 ]

   with one v_perm_b32 per table.  Included by the parity kernel
   (fd_ed25519_reedsol.hip), the recover kernel (fd_ed25519_recover.hip) and
   the test-only diag library (diag/fd_ed25519_diag_reedsol.hip), which runs
   these two functions on caller-chosen operands. */
#ifndef FD_REEDSOL_DEV_H
#define FD_REEDSOL_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* the three byte selectors of a dword x: per byte, bits 0-2, bits 3-5 and bits 6-7 */
__device__ __forceinline__ void fd_reedsol_sel(const uint32_t x, uint32_t& s0, uint32_t& s1, uint32_t& s2) {
  s0 = x & 0x07070707u; s1 = (x >> 3) & 0x07070707u; s2 = (x >> 6) & 0x03030303u;
}

/* the four products c x of x's bytes from c's 20 table bytes: t = T0 | T1, t2 = T2 */
__device__ __forceinline__ uint32_t fd_reedsol_mul(const uint4 t, const uint32_t t2, const uint32_t s0, const uint32_t s1, const uint32_t s2) {
  return __builtin_amdgcn_perm(t.y, t.x, s0) ^ __builtin_amdgcn_perm(t.w, t.z, s1) ^ __builtin_amdgcn_perm(0u, t2, s2);
}

#endif
