/* fd_ed25519_diag_reedsol.hip -- test-only: the GF(2^8) product of the
   Reed-Solomon kernels (fd_reedsol_dev.h) and the recover kernel's
   coefficient build (fd_reedsol_core.h's log_d, log_n and coef from tables in
   LDS) on caller-chosen operands.

   A whole set only ever multiplies by the coefficients its d and its masks
   happen to give; neither every product c x nor a chosen basis is reachable
   that way.  This unit includes the product's fd_reedsol_dev.h and
   fd_reedsol_core.h unchanged, compiles them with the product's flags and
   fills its LDS tables as the two kernels do, from the engine's table block;
   tests/test_gpu_gf256_diag.py compares what comes back with reedsol_model
   and recover_model.  A third object of libfd_ed25519_diag.so; not linked
   into the product library and no part of its ABI.

       int fd_ed25519_diag_reedsol( int op, const uint8_t* tab, const uint32_t* in,
                                    uint32_t* out, unsigned long n )

   with host pointers: tab is the FD_REEDSOL_CORE_TAB_BYTES of
   fd_ed25519_hip_private_reedsol_tables (the block an engine uploads; the
   diag library does not link the host runtime, so the caller fetches it), in
   is n cases, out is n rows.  The entry point copies tab, in and out's n rows
   up (so a byte no lane stores keeps the caller's value), launches,
   synchronises, copies n rows back and frees, and returns the HIP error code.
   hipErrorInvalidValue, before any launch, for an unknown op, a missing
   pointer, n above 2^20 and any case outside the bounds below.  The device
   out array has 64 more rows of 0xc5 behind it; one that changed is
   hipErrorUnknown.

     op 0 PRODUCT  a case is two words (c, x), c < 256; a row is one word: the
                   four byte products c x[b], through fd_reedsol_sel and
                   fd_reedsol_mul on the 32 table bytes of c in LDS.  Blocks
                   of 256 lanes, case i on lane i % 256 of block i / 256.
     op 1 COEF     a case is 20 words: cnt, d, then basis[0 .. d) as bytes (68
                   bytes, the rest zero); 1 <= d <= 67, d < cnt <= 134, the
                   basis strictly increasing and below cnt, as the kernel's
                   prefix count makes it.  A row is 134 x 68 bytes: row r
                   holds L[ e_r ][ basis[ i ] ] at byte i < d for e_r the r-th
                   slot of [0, cnt) that is no basis slot; every other byte is
                   not written.  One block of 256 lanes per case, in the
                   recover kernel's order: log_d a lane per basis slot and
                   log_n a lane per target, a barrier, then one coefficient a
                   lane. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#define FD_SHRED_FN __device__ static inline
#include "../fd_reedsol_core.h"
#include "../fd_reedsol_dev.h"

#define RS_DIAG_MAX_N   (1ul << 20)
#define RS_DIAG_BLOCK   256
#define RS_DIAG_STRIDE  68     /* the recover kernel's FD_RC_STRIDE */
#define RS_DIAG_COEF_IN 20     /* words a COEF case */
#define RS_DIAG_COEF_OUT (FD_FEC_CORE_CNT_MAX * RS_DIAG_STRIDE / 4)   /* words a COEF row */
#define RS_DIAG_PAD_ROWS 64
#define RS_DIAG_CANARY  0xc5

enum { RS_OP_PRODUCT, RS_OP_COEF, RS_OP_N };

__global__ void __launch_bounds__(RS_DIAG_BLOCK)
diag_rs_product_kernel(const uint8_t* tab, const uint32_t* in, uint32_t* out, uint32_t n) {
  __shared__ uint4 s_mul[FD_REEDSOL_CORE_MUL_BYTES / 16];        /* [256][2]: T0 T1 | T2 pad */
  const uint32_t t = threadIdx.x;
  const uint4* gmul = reinterpret_cast<const uint4*>(tab);
  for (uint32_t q = t; q < FD_REEDSOL_CORE_MUL_BYTES / 16; q += RS_DIAG_BLOCK) s_mul[q] = gmul[q];
  __syncthreads();
  const uint32_t i = blockIdx.x * RS_DIAG_BLOCK + t;
  if (i >= n) return;
  const uint32_t c = in[2u * i] & 0xffu, x = in[2u * i + 1u];
  uint32_t s0, s1, s2;
  fd_reedsol_sel(x, s0, s1, s2);
  out[i] = fd_reedsol_mul(s_mul[2 * c], s_mul[2 * c + 1].x, s0, s1, s2);
}

__global__ void __launch_bounds__(RS_DIAG_BLOCK)
diag_rs_coef_kernel(const uint8_t* tab, const uint32_t* in, uint32_t* out) {
  __shared__ fd_reedsol_core_gf_t s_gf;
  __shared__ uint8_t s_basis[RS_DIAG_STRIDE];
  __shared__ uint8_t s_log_d[RS_DIAG_STRIDE];
  __shared__ uint8_t s_tgt[FD_FEC_CORE_CNT_MAX];
  __shared__ uint8_t s_log_n[FD_FEC_CORE_CNT_MAX];
  const uint32_t t = threadIdx.x;
  const uint32_t* src = in + (uint64_t)blockIdx.x * RS_DIAG_COEF_IN;
  const uint32_t cnt = src[0], d = src[1], ntgt = cnt - d;   /* the entry point checked them */
  {
    const uint32_t* ggf = reinterpret_cast<const uint32_t*>(tab + FD_REEDSOL_CORE_GF_AT);
    uint32_t* lgf = reinterpret_cast<uint32_t*>(&s_gf);
    for (uint32_t q = t; q < sizeof(fd_reedsol_core_gf_t) / 4; q += RS_DIAG_BLOCK) lgf[q] = ggf[q];
  }
  if (t < RS_DIAG_STRIDE) s_basis[t] = (uint8_t)(src[2u + (t >> 2)] >> (8u * (t & 3u)));
  __syncthreads();
  if (t == 0) {   /* the targets: every slot that is no basis slot, in set order */
    uint32_t i = 0u, r = 0u;
    for (uint32_t e = 0; e < cnt; e++) {
      if (i < d && s_basis[i] == e) i++;
      else s_tgt[r++] = (uint8_t)e;
    }
  }
  __syncthreads();
  if (t < d) s_log_d[t] = (uint8_t)fd_reedsol_core_log_d(&s_gf, s_basis, d, s_basis[t]);
  if (t < ntgt) s_log_n[t] = (uint8_t)fd_reedsol_core_log_n(&s_gf, s_basis, d, s_tgt[t]);
  __syncthreads();
  uint8_t* coef8 = reinterpret_cast<uint8_t*>(out + (uint64_t)blockIdx.x * RS_DIAG_COEF_OUT);
  for (uint32_t q = t; q < ntgt * d; q += RS_DIAG_BLOCK) {
    const uint32_t r = q / d, i = q % d;   /* r < ntgt <= 133, i < d <= 67: inside the row */
    coef8[r * RS_DIAG_STRIDE + i] = (uint8_t)fd_reedsol_core_coef(&s_gf, s_log_n[r], s_log_d[i], s_tgt[r], s_basis[i]);
  }
}

/* ---- host side ------------------------------------------------------------ */

static bool rs_case_ok(int op, const uint32_t* c) {
  if (op == RS_OP_PRODUCT) return c[0] < 256u;
  const uint32_t cnt = c[0], d = c[1];
  if (d < 1u || d > FD_REEDSOL_CORE_MAX || cnt <= d || cnt > FD_FEC_CORE_CNT_MAX) return false;
  const uint8_t* b = reinterpret_cast<const uint8_t*>(c + 2);
  for (uint32_t i = 0; i < d; i++)
    if (b[i] >= cnt || (i && b[i] <= b[i - 1u])) return false;
  for (uint32_t i = d; i < 4u * (RS_DIAG_COEF_IN - 2u); i++)
    if (b[i]) return false;
  return true;
}

extern "C" int fd_ed25519_diag_reedsol(int op, const uint8_t* tab, const uint32_t* in, uint32_t* out, unsigned long n) {
  if (op < 0 || op >= RS_OP_N || !tab || !in || !out || n > RS_DIAG_MAX_N) return (int)hipErrorInvalidValue;
  const size_t in_w = op == RS_OP_PRODUCT ? 2u : RS_DIAG_COEF_IN, out_w = op == RS_OP_PRODUCT ? 1u : RS_DIAG_COEF_OUT;
  for (unsigned long i = 0; i < n; i++)
    if (!rs_case_ok(op, in + i * in_w)) return (int)hipErrorInvalidValue;
  if (!n) return (int)hipSuccess;
  const size_t in_sz = (size_t)n * in_w * 4u, out_sz = (size_t)n * out_w * 4u, pad_sz = RS_DIAG_PAD_ROWS * out_w * 4u;
  uint8_t* d_tab = nullptr;
  uint32_t *d_in = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc((void**)&d_tab, FD_REEDSOL_CORE_TAB_BYTES);
  if (e == hipSuccess) e = hipMalloc((void**)&d_in, in_sz);
  if (e == hipSuccess) e = hipMalloc((void**)&d_out, out_sz + pad_sz);
  if (e == hipSuccess) e = hipMemcpy(d_tab, tab, FD_REEDSOL_CORE_TAB_BYTES, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, in_sz, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_out, out, out_sz, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(reinterpret_cast<uint8_t*>(d_out) + out_sz, RS_DIAG_CANARY, pad_sz);
  if (e == hipSuccess) {
    if (op == RS_OP_PRODUCT)
      hipLaunchKernelGGL(diag_rs_product_kernel, dim3((uint32_t)((n + RS_DIAG_BLOCK - 1u) / RS_DIAG_BLOCK)), dim3(RS_DIAG_BLOCK), 0, 0,
                         (const uint8_t*)d_tab, (const uint32_t*)d_in, d_out, (uint32_t)n);
    else
      hipLaunchKernelGGL(diag_rs_coef_kernel, dim3((uint32_t)n), dim3(RS_DIAG_BLOCK), 0, 0, (const uint8_t*)d_tab,
                         (const uint32_t*)d_in, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, out_sz, hipMemcpyDeviceToHost);
  if (e == hipSuccess) {
    uint8_t* pad = static_cast<uint8_t*>(malloc(pad_sz));
    if (!pad) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipMemcpy(pad, reinterpret_cast<uint8_t*>(d_out) + out_sz, pad_sz, hipMemcpyDeviceToHost);
    for (size_t b = 0; e == hipSuccess && b < pad_sz; b++)
      if (pad[b] != RS_DIAG_CANARY) e = hipErrorUnknown;   /* a lane stored past the n rows */
    free(pad);
  }
  if (d_tab) (void)hipFree(d_tab);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  return (int)e;
}
