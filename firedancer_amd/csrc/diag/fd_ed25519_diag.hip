/* fd_ed25519_diag.hip -- test-only: single device functions of the field,
   scalar and group headers on caller-chosen operands.

   Every GPU parity test enters through a whole verify, whose arithmetic
   only ever sees operands derived from a hash or a decompressed point; the
   edges of the limb bounds, of the carry chains and of the scalar folds
   are not reachable that way.  This unit includes the product's device
   headers unchanged, compiles them with the product's flags, and wraps one
   function per kernel (the pattern of fd_ed25519_diag_half_kernel, without
   an engine): tests/test_gpu_field_diag.py, test_gpu_scalar_diag.py and
   test_gpu_group_diag.py compare what comes back with Python integers.

   Built as libfd_ed25519_diag.so; not linked into the product library and
   no part of its ABI.  The library's other objects, each with an entry
   point and argument list of its own: fd_ed25519_diag_hash.hip (the SHA-512
   and SHA-256 headers), fd_ed25519_diag_reedsol.hip (the GF(2^8) product
   and the recover kernel's coefficients) and fd_ed25519_diag_sign.hip (the
   signer's family: ge_scalarmult_base, ge_encode and mul256_add over the
   signer's own [0..128]B table, tests/test_gpu_sign_diag.py).

   One C entry point per family,

       int fd_ed25519_diag_<family>( int op, const uint32_t* in, uint32_t* out, unsigned long n )

   with host pointers: n cases of IN words each in, n cases of OUT words
   each out (the strides below); it allocates, copies, launches,
   synchronises, copies back and frees, and returns the HIP error code
   (hipErrorInvalidValue for an unknown op, n above 2^20 or, digits160, a
   window count outside [33, 38]).

   Every load and store is guarded by the case index.  In the quad and
   16-lane kernels every lane runs to the end (rows past n compute on
   zeros and skip their stores): a lane that returned early would be
   missing from the DPP / permlane / bpermute exchanges of its neighbours.
   No loop depends on data. */
#include <hip/hip_runtime.h>
#include "../fd25519_dsm.h"
#include "../fd25519_ge4.h"
#include "../fd25519_sc.h"
#include "../fd25519_half.h"
#include "../fd25519_r16.h"

#define DIAG_MAX_N (1ul << 20)

/* ---- fe: one lane per case -----------------------------------------------
   in  20 words: f[10], g[10]   (FROMBYTES: f[0..7] are the 8 words;
                                 SQ_SH: g[0] & 1 is the lane's sh)
   out 20 words: h[10], fe_tobytes(h)[8], fe_iszero(h), fe_isodd(h)
   IDENT returns h = f untouched, so the last ten words are fe_tobytes /
   fe_iszero / fe_isodd of the caller's raw limbs. */
enum {
  FE_OP_MUL, FE_OP_MUL19, FE_OP_SQ, FE_OP_SQ2, FE_OP_MUL_U, FE_OP_SQ_U, FE_OP_SQ2_U, FE_OP_CARRY, FE_OP_IDENT,
  FE_OP_FROMBYTES, FE_OP_POW22523, FE_OP_INVERT, FE_OP_SQ_SH, FE_OP_N
};
#define FE_IN 20
#define FE_OUT 20

FD_DEV void ld_fe(fe& x, const uint32_t* src) {
#pragma unroll
  for (int i = 0; i < 10; i++) x.v[i] = (int32_t)src[i];
}

FD_DEV void st_fe(uint32_t* dst, const fe& x) {
#pragma unroll
  for (int i = 0; i < 10; i++) dst[i] = (uint32_t)x.v[i];
}

template <int OP>
__global__ void __launch_bounds__(64) diag_fe_kernel(const uint32_t* in, uint32_t* out, uint32_t n) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  fe f, g, h;
  ld_fe(f, in + (uint64_t)i * FE_IN);
  ld_fe(g, in + (uint64_t)i * FE_IN + 10);
  if (OP == FE_OP_MUL) fe_mul(h, f, g);
  if (OP == FE_OP_MUL19) { fe g19; fe_19(g19, g); fe_mul19(h, f, g, g19); }
  if (OP == FE_OP_SQ) fe_sq(h, f);
  if (OP == FE_OP_SQ2) fe_sq2(h, f);
  if (OP == FE_OP_MUL_U) fe_mul_u(h, f, g);
  if (OP == FE_OP_SQ_U) fe_sq_u(h, f);
  if (OP == FE_OP_SQ2_U) fe_sq2_u(h, f);
  if (OP == FE_OP_CARRY) fe_carry(h, f);
  if (OP == FE_OP_IDENT) h = f;
  if (OP == FE_OP_FROMBYTES) {
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = (uint32_t)f.v[k];
    fe_frombytes(h, w);
  }
  if (OP == FE_OP_POW22523) fe_pow22523(h, f);
  if (OP == FE_OP_INVERT) fe_invert(h, f);
  if (OP == FE_OP_SQ_SH) fe_sq_sh(h, f, g.v[0] & 1);
  uint32_t* o = out + (uint64_t)i * FE_OUT;
  st_fe(o, h);
  uint32_t s[8];
  fe_tobytes(s, h);
#pragma unroll
  for (int k = 0; k < 8; k++) o[10 + k] = s[k];
  o[18] = fe_iszero(h) ? 1u : 0u;
  o[19] = (uint32_t)fe_isodd(h);
}

/* ---- r16: one 16-lane row per case, four cases per wave -------------------
   in  32 words: f[16], g[16]   (FROM_FE: f[0..9] are the ten fe limbs)
   out 32 words: x[16] (lane c's result), r16_words(r16_digits(x))[8],
                 r16_iszero(x), 7 unused
   IDENT returns x = f, so the digits and the zero test are of the caller's
   raw limbs. */
enum { R16_OP_MUL, R16_OP_SQ, R16_OP_IDENT, R16_OP_FROM_FE, R16_OP_POW22523, R16_OP_N };
#define R16_IN 32
#define R16_OUT 32

template <int OP>
__global__ void __launch_bounds__(64) diag_r16_kernel(const uint32_t* in, uint32_t* out, uint32_t n) {
  r16ctx k;
  r16_init(k);
  const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 4);
  const bool valid = row < n;
  const uint32_t* src = in + (uint64_t)(valid ? row : 0u) * R16_IN;
  const uint32_t f = valid ? src[k.c] : 0u, g = valid ? src[16 + k.c] : 0u;
  uint32_t x = f;
  if (OP == R16_OP_MUL) x = r16_mul(f, g, k);
  if (OP == R16_OP_SQ) x = r16_sq(f, k);
  if (OP == R16_OP_FROM_FE) {
    fe t;
#pragma unroll
    for (int i = 0; i < 10; i++) t.v[i] = valid ? (int32_t)src[i] : 0;
    x = r16_from_fe(t, k);
  }
  if (OP == R16_OP_POW22523) x = r16_pow22523(f, k);
  uint32_t l[16], w[8];
  r16_digits(l, x);
  r16_words(w, l);
  const bool z = r16_iszero(x);
  /* the last cross-lane operation is behind us */
  if (valid) {
    uint32_t* o = out + (uint64_t)row * R16_OUT;
    o[k.c] = x;
    if (k.c < 8u) {
      uint32_t wv = 0u;
#pragma unroll
      for (int i = 0; i < 8; i++) wv = k.c == (uint32_t)i ? w[i] : wv;
      o[16 + k.c] = wv;
    }
    if (k.c == 8u) o[24] = z ? 1u : 0u;
  }
}

/* ---- sc: one lane per case ------------------------------------------------
   in  16 words (REDUCE512: all; the others: the scalar's 8 words)
   out 64 words: REDUCE512 8 words; IS_CANONICAL 1; RECODE16 64 / RECODE256
   32 / RECODE65536 16 signed digits, digit i at out[i], each as the loop
   would pop it (the most significant first). */
enum { SC_OP_REDUCE512, SC_OP_IS_CANONICAL, SC_OP_RECODE16, SC_OP_RECODE256, SC_OP_RECODE65536, SC_OP_N };
#define SC_IN 16
#define SC_OUT 64

template <int BITS>
FD_DEV void pop_all(uint32_t* o, uint32_t (&d)[8]) {
#pragma unroll
  for (int t = 256 / BITS - 1; t >= 0; t--) o[t] = (uint32_t)pop_digit<BITS>(d);
}

template <int OP>
__global__ void __launch_bounds__(64) diag_sc_kernel(const uint32_t* in, uint32_t* out, uint32_t n) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const uint32_t* src = in + (uint64_t)i * SC_IN;
  uint32_t* o = out + (uint64_t)i * SC_OUT;
  uint32_t x[16], s[8], d[8];
#pragma unroll
  for (int w = 0; w < 16; w++) x[w] = src[w];
#pragma unroll
  for (int w = 0; w < 8; w++) s[w] = x[w];
  if (OP == SC_OP_REDUCE512) {
    sc_reduce512(d, x);
#pragma unroll
    for (int w = 0; w < 8; w++) o[w] = d[w];
  }
  if (OP == SC_OP_IS_CANONICAL) o[0] = sc_is_canonical(s) ? 1u : 0u;
  if (OP == SC_OP_RECODE16) { recode_radix16(d, s); pop_all<4>(o, d); }
  if (OP == SC_OP_RECODE256) { recode_radix256(d, s); pop_all<8>(o, d); }
  if (OP == SC_OP_RECODE65536) { recode_radix65536(d, s); pop_all<16>(o, d); }
}

/* ---- digits160: the 4-bit forms' (dsm4, dsm8, dsm16) prologue and pops, one lane per case
   in  11 words: c[5], |d|[5], W (33..38, checked on the host)
   out 80 words: c's W digits at out[it], |d|'s at out[40 + it], it = W-1
   (popped first, read unsigned: & 15) down to 0; the rest stay zero.
   38 pops whatever W: after W of them the registers hold zeros. */
#define D160_IN 11
#define D160_OUT 80
#define D160_WMAX ((FD_HALF_DBITS_MAX + 4) / 4)

__global__ void __launch_bounds__(64) diag_digits160_kernel(const uint32_t* in, uint32_t* out, uint32_t n) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const uint32_t* src = in + (uint64_t)i * D160_IN;
  uint32_t* o = out + (uint64_t)i * D160_OUT;
  uint32_t cd[5], dd[5], x[5], t[5];
  const int W = (int)src[10];
  const int sh = 160 - 4 * W;
#pragma unroll
  for (int w = 0; w < 5; w++) x[w] = src[5 + w];
  shl160v(t, x, sh); recode160<4>(dd, t);
#pragma unroll
  for (int w = 0; w < 5; w++) x[w] = src[w];
  shl160v(t, x, sh); recode160<4>(cd, t);
#pragma unroll
  for (int p = 0; p < D160_WMAX; p++) {
    const int it = W - 1 - p;
    int ea = pop160<4>(cd), er = pop160<4>(dd);
    if (p == 0) { ea &= 15; er &= 15; }   /* top digits in [0,8] */
    if (it >= 0) {
      o[it] = (uint32_t)ea;
      o[40 + it] = (uint32_t)er;
    }
  }
}

/* ---- ge: one lane per case ------------------------------------------------
   in  80 words: P (X, Y, Z, T | a cached's or precomp's fields, ten limbs
       each) and Q likewise; the cneg forms take their flag from Q's word 0
   out 40 words: the result's fields in declaration order (a p2 or precomp
       leaves the last ten zero) */
enum {
  GE_OP_P2_DBL, GE_OP_P3_DBL, GE_OP_ADD, GE_OP_ADD_NT, GE_OP_MADD, GE_OP_TO_CACHED, GE_OP_TO_CACHED_UXY,
  GE_OP_P1P1_TO_P2, GE_OP_P1P1_TO_P3, GE_OP_P1P1_TO_P3_U, GE_OP_P1P1_TO_P3_UXYT, GE_OP_CACHED_CNEG,
  GE_OP_PRECOMP_CNEG, GE_OP_N
};
#define GE_IN 80
#define GE_OUT 40

template <int OP>
__global__ void __launch_bounds__(64) diag_ge_kernel(const uint32_t* in, uint32_t* out, uint32_t n) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const uint32_t* src = in + (uint64_t)i * GE_IN;
  fe a[4], b[4], r[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    ld_fe(a[q], src + 10 * q);
    ld_fe(b[q], src + 40 + 10 * q);
    fe_0(r[q]);
  }
  const bool flag = src[40] != 0u;
  const ge_p2 p2 = {a[0], a[1], a[2]};
  const ge_p3 p3 = {a[0], a[1], a[2], a[3]};
  const ge_p1p1 pp = {a[0], a[1], a[2], a[3]};
  const ge_cached qc = {b[0], b[1], b[2], b[3]};
  const ge_precomp qp = {b[0], b[1], b[2]};
  if (OP == GE_OP_P2_DBL || OP == GE_OP_P3_DBL || OP == GE_OP_ADD || OP == GE_OP_ADD_NT || OP == GE_OP_MADD) {
    ge_p1p1 o;
    if (OP == GE_OP_P2_DBL) ge_p2_dbl(o, p2);
    if (OP == GE_OP_P3_DBL) ge_p3_dbl(o, p3);
    if (OP == GE_OP_ADD) ge_add<false>(o, p3, qc);
    if (OP == GE_OP_ADD_NT) ge_add<true>(o, p3, qc);
    if (OP == GE_OP_MADD) ge_madd(o, p3, qp);
    r[0] = o.X; r[1] = o.Y; r[2] = o.Z; r[3] = o.T;
  }
  if (OP == GE_OP_TO_CACHED || OP == GE_OP_TO_CACHED_UXY) {
    ge_cached o;
    if (OP == GE_OP_TO_CACHED) ge_p3_to_cached<false>(o, p3);
    else ge_p3_to_cached<true>(o, p3);
    r[0] = o.YplusX; r[1] = o.YminusX; r[2] = o.Z2; r[3] = o.T2d;
  }
  if (OP == GE_OP_P1P1_TO_P2) {
    ge_p2 o;
    ge_p1p1_to_p2(o, pp);
    r[0] = o.X; r[1] = o.Y; r[2] = o.Z;
  }
  if (OP == GE_OP_P1P1_TO_P3 || OP == GE_OP_P1P1_TO_P3_U || OP == GE_OP_P1P1_TO_P3_UXYT) {
    ge_p3 o;
    if (OP == GE_OP_P1P1_TO_P3) ge_p1p1_to_p3(o, pp);
    if (OP == GE_OP_P1P1_TO_P3_U) ge_p1p1_to_p3_u(o, pp);
    if (OP == GE_OP_P1P1_TO_P3_UXYT) ge_p1p1_to_p3_uxyt(o, pp);
    r[0] = o.X; r[1] = o.Y; r[2] = o.Z; r[3] = o.T;
  }
  if (OP == GE_OP_CACHED_CNEG) {
    ge_cached o = {a[0], a[1], a[2], a[3]};
    ge_cached_cneg(o, flag);
    r[0] = o.YplusX; r[1] = o.YminusX; r[2] = o.Z2; r[3] = o.T2d;
  }
  if (OP == GE_OP_PRECOMP_CNEG) {
    ge_precomp o = {a[0], a[1], a[2]};
    ge_precomp_cneg(o, flag);
    r[0] = o.yplusx; r[1] = o.yminusx; r[2] = o.xy2d;
  }
  uint32_t* o = out + (uint64_t)i * GE_OUT;
#pragma unroll
  for (int q = 0; q < 4; q++) st_fe(o + 10 * q, r[q]);
}

/* ---- ge4: one quad per case, the ge layout (lane q holds entry q) ---------
   Q is the qc operand of ADD; the cneg forms take their flag from Q's word
   0 (CNEG_P3 negates lanes 0 and 3, CNEG_P1P1 lane 0, as the dsm4 loop
   does). */
enum { GE4_OP_DBL, GE4_OP_ADD, GE4_OP_TO_P3, GE4_OP_TO_QC, GE4_OP_CNEG_P3, GE4_OP_CNEG_P1P1, GE4_OP_N };

template <int OP>
__global__ void __launch_bounds__(64) diag_ge4_kernel(const uint32_t* in, uint32_t* out, uint32_t n) {
  const qmask_t m = quad_masks();
  const uint32_t cs = blockIdx.x * 16u + (threadIdx.x >> 2), q = threadIdx.x & 3u;
  const bool valid = cs < n;
  const uint32_t* src = in + (uint64_t)(valid ? cs : 0u) * GE_IN;
  fe p, c, r;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    p.v[i] = valid ? (int32_t)src[10 * q + i] : 0;
    c.v[i] = valid ? (int32_t)src[40 + 10 * q + i] : 0;
  }
  const bool flag = valid && src[40] != 0u;
  r = p;
  if (OP == GE4_OP_DBL) ge4_dbl(r, p, m);
  if (OP == GE4_OP_ADD) ge4_add(r, p, c, m);
  if (OP == GE4_OP_TO_P3) ge4_to_p3(r, p);
  if (OP == GE4_OP_TO_QC) ge4_to_qc(r, p, m);
  if (OP == GE4_OP_CNEG_P3) ge4_cneg(r, m.l03, flag);
  if (OP == GE4_OP_CNEG_P1P1) ge4_cneg(r, m.l0, flag);
  /* the last DPP operation is behind us */
  if (valid) st_fe(out + (uint64_t)cs * GE_OUT + 10 * q, r);
}

/* ---- ge16: one wave per case, row q holds coordinate q --------------------
   in  128 words: P[64] (lane t's limb: coordinate t >> 4, limb t & 15),
       Q[64] (the qc operand of the additions)
   out 64 words likewise */
enum {
  GE16_OP_DBL2_FF, GE16_OP_DBL2_TF, GE16_OP_DBL2_TT, GE16_OP_ADD2_T, GE16_OP_ADD2_T_NEG, GE16_OP_ADD2_F,
  GE16_OP_ADD2_F_NEG, GE16_OP_TO_QC, GE16_OP_N
};
#define GE16_IN 128
#define GE16_OUT 64

template <int OP>
__global__ void __launch_bounds__(64) diag_ge16_kernel(const uint32_t* in, uint32_t* out, uint32_t n) {
  r16ctx k;
  r16_init(k);
  const uint32_t cs = blockIdx.x;
  const bool valid = cs < n;
  const uint32_t* src = in + (uint64_t)(valid ? cs : 0u) * GE16_IN;
  const uint32_t p = valid ? src[threadIdx.x] : 0u, q = valid ? src[64 + threadIdx.x] : 0u;
  uint32_t r = p;
  if (OP == GE16_OP_DBL2_FF) r = ge16_dbl2<false, false>(p, k);
  if (OP == GE16_OP_DBL2_TF) r = ge16_dbl2<true, false>(p, k);
  if (OP == GE16_OP_DBL2_TT) r = ge16_dbl2<true, true>(p, k);
  if (OP == GE16_OP_ADD2_T) r = ge16_add2<true>(p, q, false, k);
  if (OP == GE16_OP_ADD2_T_NEG) r = ge16_add2<true>(p, q, true, k);
  if (OP == GE16_OP_ADD2_F) r = ge16_add2<false>(p, q, false, k);
  if (OP == GE16_OP_ADD2_F_NEG) r = ge16_add2<false>(p, q, true, k);
  if (OP == GE16_OP_TO_QC) r = ge16_to_qc(p, r16_from_fe(fe{FE_D2}, k), k);
  /* the last cross-lane operation is behind us */
  if (valid) out[(uint64_t)cs * GE16_OUT + threadIdx.x] = r;
}

/* ---- host side ------------------------------------------------------------ */

typedef void (*diag_kernel_t)(const uint32_t*, uint32_t*, uint32_t);

/* n cases of in_words each to the device, one launch of per_block cases per
   64-lane block (the grid rounded up), out_words each back */
static int diag_run(diag_kernel_t kern, unsigned per_block, const uint32_t* in, size_t in_words, uint32_t* out,
                    size_t out_words, unsigned long n) {
  if (!kern || !in || !out || n > DIAG_MAX_N) return (int)hipErrorInvalidValue;
  if (!n) return (int)hipSuccess;
  const size_t in_sz = (size_t)n * in_words * 4u, out_sz = (size_t)n * out_words * 4u;
  uint32_t *d_in = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc((void**)&d_in, in_sz);
  if (e == hipSuccess) e = hipMalloc((void**)&d_out, out_sz);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, in_sz, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_out, 0, out_sz);
  if (e == hipSuccess) {
    const uint32_t grid = (uint32_t)((n + per_block - 1) / per_block);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64), 0, 0, (const uint32_t*)d_in, d_out, (uint32_t)n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, out_sz, hipMemcpyDeviceToHost);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  return (int)e;
}

#define K(T, OP) case OP: return (diag_kernel_t)T<OP>;

static diag_kernel_t fe_kernel(int op) {
  switch (op) {
    K(diag_fe_kernel, FE_OP_MUL) K(diag_fe_kernel, FE_OP_MUL19) K(diag_fe_kernel, FE_OP_SQ) K(diag_fe_kernel, FE_OP_SQ2)
    K(diag_fe_kernel, FE_OP_MUL_U) K(diag_fe_kernel, FE_OP_SQ_U) K(diag_fe_kernel, FE_OP_SQ2_U)
    K(diag_fe_kernel, FE_OP_CARRY) K(diag_fe_kernel, FE_OP_IDENT) K(diag_fe_kernel, FE_OP_FROMBYTES)
    K(diag_fe_kernel, FE_OP_POW22523) K(diag_fe_kernel, FE_OP_INVERT) K(diag_fe_kernel, FE_OP_SQ_SH)
  default: return nullptr;
  }
}

static diag_kernel_t r16_kernel(int op) {
  switch (op) {
    K(diag_r16_kernel, R16_OP_MUL) K(diag_r16_kernel, R16_OP_SQ) K(diag_r16_kernel, R16_OP_IDENT)
    K(diag_r16_kernel, R16_OP_FROM_FE) K(diag_r16_kernel, R16_OP_POW22523)
  default: return nullptr;
  }
}

static diag_kernel_t sc_kernel(int op) {
  switch (op) {
    K(diag_sc_kernel, SC_OP_REDUCE512) K(diag_sc_kernel, SC_OP_IS_CANONICAL) K(diag_sc_kernel, SC_OP_RECODE16)
    K(diag_sc_kernel, SC_OP_RECODE256) K(diag_sc_kernel, SC_OP_RECODE65536)
  default: return nullptr;
  }
}

static diag_kernel_t ge_kernel(int op) {
  switch (op) {
    K(diag_ge_kernel, GE_OP_P2_DBL) K(diag_ge_kernel, GE_OP_P3_DBL) K(diag_ge_kernel, GE_OP_ADD)
    K(diag_ge_kernel, GE_OP_ADD_NT) K(diag_ge_kernel, GE_OP_MADD) K(diag_ge_kernel, GE_OP_TO_CACHED)
    K(diag_ge_kernel, GE_OP_TO_CACHED_UXY) K(diag_ge_kernel, GE_OP_P1P1_TO_P2) K(diag_ge_kernel, GE_OP_P1P1_TO_P3)
    K(diag_ge_kernel, GE_OP_P1P1_TO_P3_U) K(diag_ge_kernel, GE_OP_P1P1_TO_P3_UXYT)
    K(diag_ge_kernel, GE_OP_CACHED_CNEG) K(diag_ge_kernel, GE_OP_PRECOMP_CNEG)
  default: return nullptr;
  }
}

static diag_kernel_t ge4_kernel(int op) {
  switch (op) {
    K(diag_ge4_kernel, GE4_OP_DBL) K(diag_ge4_kernel, GE4_OP_ADD) K(diag_ge4_kernel, GE4_OP_TO_P3)
    K(diag_ge4_kernel, GE4_OP_TO_QC) K(diag_ge4_kernel, GE4_OP_CNEG_P3) K(diag_ge4_kernel, GE4_OP_CNEG_P1P1)
  default: return nullptr;
  }
}

static diag_kernel_t ge16_kernel(int op) {
  switch (op) {
    K(diag_ge16_kernel, GE16_OP_DBL2_FF) K(diag_ge16_kernel, GE16_OP_DBL2_TF) K(diag_ge16_kernel, GE16_OP_DBL2_TT)
    K(diag_ge16_kernel, GE16_OP_ADD2_T) K(diag_ge16_kernel, GE16_OP_ADD2_T_NEG) K(diag_ge16_kernel, GE16_OP_ADD2_F)
    K(diag_ge16_kernel, GE16_OP_ADD2_F_NEG) K(diag_ge16_kernel, GE16_OP_TO_QC)
  default: return nullptr;
  }
}

extern "C" int fd_ed25519_diag_fe(int op, const uint32_t* in, uint32_t* out, unsigned long n) {
  return diag_run(fe_kernel(op), 64, in, FE_IN, out, FE_OUT, n);
}

extern "C" int fd_ed25519_diag_r16(int op, const uint32_t* in, uint32_t* out, unsigned long n) {
  return diag_run(r16_kernel(op), 4, in, R16_IN, out, R16_OUT, n);
}

extern "C" int fd_ed25519_diag_sc(int op, const uint32_t* in, uint32_t* out, unsigned long n) {
  return diag_run(sc_kernel(op), 64, in, SC_IN, out, SC_OUT, n);
}

extern "C" int fd_ed25519_diag_digits160(int op, const uint32_t* in, uint32_t* out, unsigned long n) {
  if (op != 0 || !in || n > DIAG_MAX_N) return (int)hipErrorInvalidValue;
  for (unsigned long i = 0; i < n; i++) {
    const uint32_t W = in[i * D160_IN + 10];
    if (W < 33u || W > (uint32_t)D160_WMAX) return (int)hipErrorInvalidValue;
  }
  return diag_run(diag_digits160_kernel, 64, in, D160_IN, out, D160_OUT, n);
}

extern "C" int fd_ed25519_diag_ge(int op, const uint32_t* in, uint32_t* out, unsigned long n) {
  return diag_run(ge_kernel(op), 64, in, GE_IN, out, GE_OUT, n);
}

extern "C" int fd_ed25519_diag_ge4(int op, const uint32_t* in, uint32_t* out, unsigned long n) {
  return diag_run(ge4_kernel(op), 16, in, GE_IN, out, GE_OUT, n);
}

extern "C" int fd_ed25519_diag_ge16(int op, const uint32_t* in, uint32_t* out, unsigned long n) {
  return diag_run(ge16_kernel(op), 1, in, GE16_IN, out, GE16_OUT, n);
}
