/* fd_ed25519_diag_sign.hip -- test-only: the arithmetic of the device signer
   (fd_ed25519_sign_kernel, fd_ed25519_gen.hip) on caller-chosen operands:
   ge_scalarmult_base and ge_encode (fd25519_dsm.h) and mul256_add
   (fd25519_sc.h), which the sign kernel alone calls.

   A signature only ever feeds these SHA-512 outputs: a scalar whose recoded
   digits are -128 or zero where it matters, a 32-bit pattern that a carry
   chain needs, a point with x = 0 or y next to p are not reachable that
   way.  This unit includes the product's headers unchanged, compiles them
   with the product's flags and has the sign kernel's own shape: 256 lanes a
   block, the [0..128]B table copied to LDS by the same strided int4 loop and
   barrier, one case per lane.  tests/test_gpu_sign_diag.py compares what
   comes back with tests/sign_model.py.  A fourth object of
   libfd_ed25519_diag.so; not linked into the product library and no part of
   its ABI.

       int fd_ed25519_diag_sign( int op, const uint32_t* in, uint32_t* out,
                                 unsigned long n, const int32_t* btab )

   with host pointers: in is n cases of 32 words, out n rows of 40 words,
   btab the FD_ED25519_BTAB_INTS of the signer's table (the diag library does
   not link the host runtime, so the caller fetches it:
   fd_ed25519_hip_private_sign_table), needed by ops 0 and 1.  The entry
   point allocates, copies, launches, synchronises, copies back and frees,
   and returns the HIP error code; hipErrorInvalidValue, before any launch,
   for an unknown op, a missing pointer (the table: ops 0 and 1 only) and n
   above 2^20.  Every load and store is guarded by the case index.

     op 0 BASE       in[0..8) a scalar s < L (the caller's promise, as the
                     kernel's sc_reduce512 makes it): ge_scalarmult_base,
                     ge_encode.  out[0..8) the encoding, out[8..38) the
                     limbs of Q.X, Q.Y, Q.Z.
     op 1 BASE_WIDE  in[0..8) any 256-bit s, by the kernel's public-key path:
                     zero-extended to 512 bits, sc_reduce512, then as op 0.
     op 2 MULADD     in[0..8) k, in[8..16) a, in[16..24) r, any values:
                     mul256_add( prod, k, a, r ), sc_reduce512( S, prod ).
                     out[0..16) prod, out[16..24) S.
     op 3 ENCODE     in[0..30) the limbs of X, Y, Z: ge_encode.  out[0..8). */
#include <hip/hip_runtime.h>
#include "../fd25519_dsm.h"
#include "../fd25519_sc.h"

#define SIGN_DIAG_MAX_N (1ul << 20)
#define SIGN_DIAG_BLOCK 256
#define SIGN_DIAG_IN    32
#define SIGN_DIAG_OUT   40

enum { SIGN_OP_BASE, SIGN_OP_BASE_WIDE, SIGN_OP_MULADD, SIGN_OP_ENCODE, SIGN_OP_N };

template <int OP>
__global__ void __launch_bounds__(SIGN_DIAG_BLOCK)
diag_sign_kernel(const int32_t* btab, const uint32_t* in, uint32_t* out, uint32_t n) {
  __shared__ int4 s_btab[FD_ED25519_BTAB_INTS / 4];
  const int4* g_btab = reinterpret_cast<const int4*>(btab);   /* ops 2 and 3: a table of zeros, never read back */
  for (int t = threadIdx.x; t < FD_ED25519_BTAB_INTS / 4; t += blockDim.x) s_btab[t] = g_btab[t];
  __syncthreads();
  const uint32_t i = blockIdx.x * SIGN_DIAG_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t* src = in + (uint64_t)i * SIGN_DIAG_IN;
  uint32_t* o = out + (uint64_t)i * SIGN_DIAG_OUT;

  if (OP == SIGN_OP_BASE || OP == SIGN_OP_BASE_WIDE) {
    uint32_t s[8];
#pragma unroll
    for (int w = 0; w < 8; w++) s[w] = src[w];
    if (OP == SIGN_OP_BASE_WIDE) {
      uint32_t wide[16], smod[8];
#pragma unroll
      for (int w = 0; w < 16; w++) wide[w] = w < 8 ? s[w] : 0u;
      sc_reduce512(smod, wide);
#pragma unroll
      for (int w = 0; w < 8; w++) s[w] = smod[w];
    }
    ge_p2 Q;
    ge_scalarmult_base(Q, s, s_btab);
    uint32_t enc[8];
    ge_encode(enc, Q);
#pragma unroll
    for (int w = 0; w < 8; w++) o[w] = enc[w];
#pragma unroll
    for (int k = 0; k < 10; k++) {
      o[8 + k] = (uint32_t)Q.X.v[k];
      o[18 + k] = (uint32_t)Q.Y.v[k];
      o[28 + k] = (uint32_t)Q.Z.v[k];
    }
  }
  if (OP == SIGN_OP_MULADD) {
    uint32_t k[8], a[8], r[8], prod[16], S[8];
#pragma unroll
    for (int w = 0; w < 8; w++) {
      k[w] = src[w];
      a[w] = src[8 + w];
      r[w] = src[16 + w];
    }
    mul256_add(prod, k, a, r);
    sc_reduce512(S, prod);
#pragma unroll
    for (int w = 0; w < 16; w++) o[w] = prod[w];
#pragma unroll
    for (int w = 0; w < 8; w++) o[16 + w] = S[w];
  }
  if (OP == SIGN_OP_ENCODE) {
    ge_p2 Q;
#pragma unroll
    for (int k = 0; k < 10; k++) {
      Q.X.v[k] = (int32_t)src[k];
      Q.Y.v[k] = (int32_t)src[10 + k];
      Q.Z.v[k] = (int32_t)src[20 + k];
    }
    uint32_t enc[8];
    ge_encode(enc, Q);
#pragma unroll
    for (int w = 0; w < 8; w++) o[w] = enc[w];
  }
}

/* ---- host side ------------------------------------------------------------ */

typedef void (*sign_kernel_t)(const int32_t*, const uint32_t*, uint32_t*, uint32_t);

static sign_kernel_t sign_kernel(int op) {
  switch (op) {
  case SIGN_OP_BASE: return diag_sign_kernel<SIGN_OP_BASE>;
  case SIGN_OP_BASE_WIDE: return diag_sign_kernel<SIGN_OP_BASE_WIDE>;
  case SIGN_OP_MULADD: return diag_sign_kernel<SIGN_OP_MULADD>;
  case SIGN_OP_ENCODE: return diag_sign_kernel<SIGN_OP_ENCODE>;
  default: return nullptr;
  }
}

extern "C" int fd_ed25519_diag_sign(int op, const uint32_t* in, uint32_t* out, unsigned long n, const int32_t* btab) {
  const sign_kernel_t kern = sign_kernel(op);
  const bool tab = op == SIGN_OP_BASE || op == SIGN_OP_BASE_WIDE;
  if (!kern || !in || !out || n > SIGN_DIAG_MAX_N || (tab && !btab)) return (int)hipErrorInvalidValue;
  if (!n) return (int)hipSuccess;
  const size_t in_sz = (size_t)n * SIGN_DIAG_IN * 4u, out_sz = (size_t)n * SIGN_DIAG_OUT * 4u;
  const size_t tab_sz = (size_t)FD_ED25519_BTAB_INTS * sizeof(int32_t);
  int32_t* d_tab = nullptr;
  uint32_t *d_in = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc((void**)&d_tab, tab_sz);
  if (e == hipSuccess) e = hipMalloc((void**)&d_in, in_sz);
  if (e == hipSuccess) e = hipMalloc((void**)&d_out, out_sz);
  if (e == hipSuccess) e = tab ? hipMemcpy(d_tab, btab, tab_sz, hipMemcpyHostToDevice) : hipMemset(d_tab, 0, tab_sz);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, in_sz, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_out, 0, out_sz);
  if (e == hipSuccess) {
    const uint32_t grid = (uint32_t)((n + SIGN_DIAG_BLOCK - 1) / SIGN_DIAG_BLOCK);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(SIGN_DIAG_BLOCK), 0, 0, (const int32_t*)d_tab, (const uint32_t*)d_in, d_out,
                       (uint32_t)n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, out_sz, hipMemcpyDeviceToHost);
  if (d_tab) (void)hipFree(d_tab);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  return (int)e;
}
