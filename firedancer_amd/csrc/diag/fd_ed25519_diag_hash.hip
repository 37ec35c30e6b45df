/* fd_ed25519_diag_hash.hip -- test-only: the device SHA-512 and SHA-256 of
   fd_sha512_dev.h / fd_sha256_dev.h on caller-chosen bytes, sizes, byte
   shifts and lanes.

   A whole front only ever hashes the lengths, byte shifts and wave mixes
   its inputs happen to have; the padding edges of both hashes, the FULL
   block path crossed with every shift, and the two-wave form's divergent
   block counts are not reachable that way.  This unit includes the
   product's fd_sha512_dev.h, fd_sha256_dev.h and fd_shred_core.h unchanged,
   compiles them with the product's flags, and wraps one function per
   kernel; tests/test_gpu_hash_diag.py compares what comes back with
   hashlib.  A second object of libfd_ed25519_diag.so (beside
   fd_ed25519_diag.hip); not linked into the product library and no part of
   its ABI.

       int fd_ed25519_diag_hash( int op, const uint8_t* buf, unsigned long buf_sz,
                                 const uint32_t* in, uint32_t* out, unsigned long n )

   with host pointers: buf[0..buf_sz) is the byte buffer the cases point
   into, in is n cases of 24 words (off, sz, flag, one spare word, 16
   operand words), out is n cases of 16 words.  The entry point copies buf
   into a device allocation of buf_sz + 16 bytes (the readable tail the
   loaders are promised; the tail holds 0xa5), copies out's n rows up (so a
   word no lane stores keeps the caller's value), launches, synchronises,
   copies n rows back and frees, and returns the HIP error code.
   hipErrorInvalidValue, before any launch, for an unknown op, n above 2^20,
   buf_sz above 2^28 (SHA-256 keeps the bit length in one word), a missing
   pointer, and any case whose bytes do not lie inside [0, buf_sz): off + sz
   (SHA256_BYTES: sz >= 1 too), off + 64 + sz for the leaf (sz >= 38), off +
   20 for the node, off + 64 for SHA256_LEAF65; SHA256_CHAIN32: sz above
   4096.  No case can therefore read outside the allocation:
   the loaders read aligned 16-byte granules from the dword that holds a
   message's first byte to at most 15 bytes past its last (the allocation
   is 256-byte aligned), sha256_node_load the six dwords around the 20
   bytes.  Every load and store is guarded by the case index.

   The device out array is padded to whole blocks with rows of 0xc5c5c5c5;
   a padding row that changed (a lane past n that stored) is hipErrorUnknown.

   SHA-512 ops return the 16 little-endian words the product's callers get
   (sc_reduce512's input); SHA-256 ops return the 8 big-endian words h[0..8)
   in out[0..8) and leave out[8..16) alone.

     SHA512_PRE8      sha512_pre<8>( operand[0..8), m )
     SHA512_RAM       sha512_ram( r = operand[0..8), a = operand[8..16), m )
     SHA512_RAM_2W    the same digest through sha512_sched_wave<16> /
                      sha512_rounds_wave<16>
     SHA256_BYTES     sha256_bytes( buf + off, sz )
     SHA256_LEAF      sha256_leaf( buf + off, sz ): leaf prefix || buf[off+64, off+64+sz)
     SHA256_NODE      sha256_node: the running node h = operand[0..8) (words
                      5..7 are not part of it), the sibling the 20 bytes at
                      buf + off, right = flag & 1
     SHA256_NODE_PAIR sha256_node_pair( left = operand[0..5), right = operand[5..10) )
   and, through fd_ed25519_diag_poh_hash( op 0..3, the same arguments ), the
   proof-of-history hashes (fd_ed25519_poh.hip's):

     SHA256_LEAF65    sha256_leaf65( buf + off ): SHA-256( 0x00 || buf[off, off+64) )
     SHA256_NODE65    sha256_node65( left = operand[0..8), right = operand[8..16) )
     SHA256_CHAIN32   sz times sha256_chain32 on the state operand[0..8), sz <= 4096
     SHA256_MIX64     sha256_mix64( state = operand[0..8), root = operand[8..16) )

   with m = buf[off, off + sz) as the product builds a sha_msg_src: base the
   aligned dword holding byte off, shift = (buf + off) & 3 = off & 3.

   Case-to-lane mapping (the tests choose wave compositions by it):

   One-wave ops: blocks of 64 threads, case i is lane i % 64 of block
   i / 64; lanes past n return early, as fd_ed25519_hash_kernel's do.  A
   lane loops over its own block count, so a wave runs as long as its
   longest lane with the others masked off.

   SHA512_RAM_2W: blocks of 128 threads serve 32 cases each, case i is lane
   i % 32 of block i / 32, in both waves; wave 1 builds the schedules into
   the 40 KiB of LDS (two buffers of 80 words x 32 lanes, one per block
   parity), wave 0 runs the rounds from them.  The wrapper restates the
   ~15 lines of hash16_block (fd_ed25519_kernels.hip) that place a
   signature on a lane, because that function is tied to the engine's work
   arrays: a lane that is not live -- lanes 32..63 of each wave, and lanes
   0..31 past n -- takes case n - 1 and stores nothing; the wave's largest
   block count comes from the same xor-shuffle maximum and readfirstlane
   (so it is the maximum over the block's live cases and case n - 1); every
   lane of both waves reaches every barrier.  sha512_sched_wave and
   sha512_rounds_wave are the product's; hash16_block itself stays covered
   by the parity tests. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "../fd_sha512_dev.h"
#define FD_SHRED_FN __device__ static inline
#include "../fd_shred_core.h"
#include "../fd_sha256_dev.h"

#define DIAG_MAX_N (1ul << 20)
#define DIAG_MAX_BUF (1ul << 28)
#define HASH_IN 24
#define HASH_OUT 16
#define HASH_CANARY 0xc5

enum {
  HASH_OP_SHA512_PRE8, HASH_OP_SHA512_RAM, HASH_OP_SHA512_RAM_2W, HASH_OP_SHA256_BYTES, HASH_OP_SHA256_LEAF,
  HASH_OP_SHA256_NODE, HASH_OP_SHA256_NODE_PAIR, HASH_OP_N,
  /* fd_ed25519_diag_poh_hash's ops 0..3, behind the first entry point's */
  HASH_OP_SHA256_LEAF65 = HASH_OP_N, HASH_OP_SHA256_NODE65, HASH_OP_SHA256_CHAIN32, HASH_OP_SHA256_MIX64, HASH_OP_END
};

FD_DEV void diag_msg(sha_msg_src& m, const uint8_t* buf, const uint32_t* src) {
  const uintptr_t mp = reinterpret_cast<uintptr_t>(buf + src[0]);
  m.base = reinterpret_cast<const uint32_t*>(mp & ~(uintptr_t)3);
  m.shift = (uint32_t)(mp & 3);
  m.sz = src[1];
}

template <int OP>
__global__ void __launch_bounds__(64) diag_hash_kernel(const uint8_t* buf, const uint32_t* in, uint32_t* out, uint32_t n) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const uint32_t* src = in + (uint64_t)i * HASH_IN;
  uint32_t* o = out + (uint64_t)i * HASH_OUT;
  uint32_t x[16];
#pragma unroll
  for (int w = 0; w < 16; w++) x[w] = src[4 + w];
  if (OP == HASH_OP_SHA512_PRE8 || OP == HASH_OP_SHA512_RAM) {
    sha_msg_src m;
    diag_msg(m, buf, src);
    uint32_t dig[16];
    if (OP == HASH_OP_SHA512_PRE8) {
      uint32_t pre[8];
#pragma unroll
      for (int w = 0; w < 8; w++) pre[w] = x[w];
      sha512_pre<8>(dig, pre, m);
    } else {
      uint32_t r[8], a[8];
#pragma unroll
      for (int w = 0; w < 8; w++) { r[w] = x[w]; a[w] = x[8 + w]; }
      sha512_ram(dig, r, a, m);
    }
#pragma unroll
    for (int w = 0; w < 16; w++) o[w] = dig[w];
  } else {
    const uint8_t* s = buf + src[0];
    uint32_t h[8];
    if (OP == HASH_OP_SHA256_BYTES) sha256_bytes(h, s, src[1]);
    if (OP == HASH_OP_SHA256_LEAF) sha256_leaf(h, s, src[1]);
    if (OP == HASH_OP_SHA256_NODE) {
#pragma unroll
      for (int w = 0; w < 8; w++) h[w] = x[w];
      sha256_node_raw r;
      sha256_node_load(r, s);
      sha256_node(h, r, (src[2] & 1u) != 0u);
    }
    if (OP == HASH_OP_SHA256_NODE_PAIR) {
      uint32_t l[5], r[5];
#pragma unroll
      for (int w = 0; w < 5; w++) { l[w] = x[w]; r[w] = x[5 + w]; }
      sha256_node_pair(h, l, r);
    }
    if (OP == HASH_OP_SHA256_LEAF65) sha256_leaf65(h, s);
    if (OP == HASH_OP_SHA256_NODE65 || OP == HASH_OP_SHA256_MIX64) {
      uint32_t l[8], r[8];
#pragma unroll
      for (int w = 0; w < 8; w++) { l[w] = x[w]; r[w] = x[8 + w]; }
      if (OP == HASH_OP_SHA256_NODE65) {
        sha256_node65(h, l, r);
      } else {
#pragma unroll
        for (int w = 0; w < 8; w++) h[w] = l[w];
        sha256_mix64(h, r);
      }
    }
    if (OP == HASH_OP_SHA256_CHAIN32) {
#pragma unroll
      for (int w = 0; w < 8; w++) h[w] = x[w];
#pragma clang loop unroll(disable)
      for (uint32_t t = 0; t < src[1]; t++) sha256_chain32(h);
    }
#pragma unroll
    for (int w = 0; w < 8; w++) o[w] = h[w];
  }
}

/* hash16_block's placement of 32 cases on two waves, restated (see above) */
__global__ void __launch_bounds__(128) diag_hash2w_kernel(const uint8_t* buf, const uint32_t* in, uint32_t* out, uint32_t n) {
  __shared__ uint64_t sched[2 * SHA2W_WORDS];
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t t = (uint64_t)blockIdx.x * SHA2W_LANES + (threadIdx.x & (SHA2W_LANES - 1u));
  const bool live = t < n && (threadIdx.x & 63u) < SHA2W_LANES;
  const uint64_t j = live ? t : n - 1u;
  const uint32_t* src = in + j * HASH_IN;
  uint32_t pre[16];
#pragma unroll
  for (int w = 0; w < 16; w++) pre[w] = src[4 + w];
  sha_msg_src m;
  diag_msg(m, buf, src);
  uint32_t nblk = (m.sz + 64u + 17u + 127u) >> 7;
  /* the wave's largest block count, the same in both waves: the barrier count */
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)nblk, off);
    nblk = o > nblk ? o : nblk;
  }
  const uint32_t nblk_wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)nblk);
  if (wave == 1u) {
    sha512_sched_wave<16>(pre, m, nblk_wave, sched);
    return;
  }
  uint32_t dig[16];
  sha512_rounds_wave<16>(dig, m, nblk_wave, sched);
  if (!live) return;
  uint32_t* o = out + j * HASH_OUT;
#pragma unroll
  for (int w = 0; w < 16; w++) o[w] = dig[w];
}

/* ---- host side ------------------------------------------------------------ */

typedef void (*diag_hash_kernel_t)(const uint8_t*, const uint32_t*, uint32_t*, uint32_t);

#define K(OP) case OP: return (diag_hash_kernel_t)diag_hash_kernel<OP>;

static diag_hash_kernel_t hash_kernel(int op) {
  switch (op) {
    K(HASH_OP_SHA512_PRE8) K(HASH_OP_SHA512_RAM) K(HASH_OP_SHA256_BYTES) K(HASH_OP_SHA256_LEAF) K(HASH_OP_SHA256_NODE)
    K(HASH_OP_SHA256_NODE_PAIR) K(HASH_OP_SHA256_LEAF65) K(HASH_OP_SHA256_NODE65) K(HASH_OP_SHA256_CHAIN32)
    K(HASH_OP_SHA256_MIX64)
  case HASH_OP_SHA512_RAM_2W: return diag_hash2w_kernel;
  default: return nullptr;
  }
}

/* the bytes case c reads lie inside [0, buf_sz) */
static bool hash_case_ok(int op, const uint32_t* c, unsigned long buf_sz) {
  const uint64_t off = c[0], sz = c[1];
  switch (op) {
  case HASH_OP_SHA512_PRE8:
  case HASH_OP_SHA512_RAM:
  case HASH_OP_SHA512_RAM_2W: return off + sz <= buf_sz;
  case HASH_OP_SHA256_BYTES: return sz >= 1u && off + sz <= buf_sz;
  case HASH_OP_SHA256_LEAF: return sz >= 38u && off + 64u + sz <= buf_sz;
  case HASH_OP_SHA256_NODE: return off + 20u <= buf_sz;
  case HASH_OP_SHA256_NODE_PAIR: return true;   /* no bytes */
  case HASH_OP_SHA256_LEAF65: return off + 64u <= buf_sz;
  case HASH_OP_SHA256_NODE65:
  case HASH_OP_SHA256_MIX64: return true;       /* no bytes */
  case HASH_OP_SHA256_CHAIN32: return sz <= 4096u;   /* no bytes; sz is the number of compressions */
  default: return false;
  }
}

static int diag_hash_run(int op, const uint8_t* buf, unsigned long buf_sz, const uint32_t* in, uint32_t* out,
                         unsigned long n) {
  const diag_hash_kernel_t kern = hash_kernel(op);
  if (!kern || !in || !out || n > DIAG_MAX_N || buf_sz > DIAG_MAX_BUF || (!buf && buf_sz)) return (int)hipErrorInvalidValue;
  for (unsigned long i = 0; i < n; i++)
    if (!hash_case_ok(op, in + i * HASH_IN, buf_sz)) return (int)hipErrorInvalidValue;
  if (!n) return (int)hipSuccess;
  const bool two = op == HASH_OP_SHA512_RAM_2W;
  const unsigned per_block = two ? SHA2W_LANES : 64u;
  const unsigned long rows = (n + 63ul) & ~63ul;   /* whole blocks of either form */
  const size_t in_sz = (size_t)n * HASH_IN * 4u, out_sz = (size_t)n * HASH_OUT * 4u;
  const size_t pad_sz = (size_t)(rows - n) * HASH_OUT * 4u;
  uint8_t* d_buf = nullptr;
  uint32_t *d_in = nullptr, *d_out = nullptr;
  uint8_t* pad = nullptr;
  hipError_t e = hipMalloc((void**)&d_buf, buf_sz + 16u);
  if (e == hipSuccess) e = hipMalloc((void**)&d_in, in_sz);
  if (e == hipSuccess) e = hipMalloc((void**)&d_out, out_sz + pad_sz);
  if (e == hipSuccess) e = hipMemset(d_buf + buf_sz, 0xa5, 16u);
  if (e == hipSuccess && buf_sz) e = hipMemcpy(d_buf, buf, buf_sz, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, in_sz, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_out, out, out_sz, hipMemcpyHostToDevice);
  if (e == hipSuccess && pad_sz) e = hipMemset(reinterpret_cast<uint8_t*>(d_out) + out_sz, HASH_CANARY, pad_sz);
  if (e == hipSuccess) {
    const uint32_t grid = (uint32_t)((n + per_block - 1u) / per_block);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(two ? 128 : 64), 0, 0, (const uint8_t*)d_buf, (const uint32_t*)d_in, d_out,
                       (uint32_t)n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, out_sz, hipMemcpyDeviceToHost);
  if (e == hipSuccess && pad_sz) {
    pad = static_cast<uint8_t*>(malloc(pad_sz));
    if (!pad) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipMemcpy(pad, reinterpret_cast<uint8_t*>(d_out) + out_sz, pad_sz, hipMemcpyDeviceToHost);
    for (size_t b = 0; e == hipSuccess && b < pad_sz; b++)
      if (pad[b] != HASH_CANARY) e = hipErrorUnknown;   /* a lane past n stored */
    free(pad);
  }
  if (d_buf) (void)hipFree(d_buf);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  return (int)e;
}

extern "C" int fd_ed25519_diag_hash(int op, const uint8_t* buf, unsigned long buf_sz, const uint32_t* in, uint32_t* out,
                                    unsigned long n) {
  if (op < 0 || op >= HASH_OP_N) return (int)hipErrorInvalidValue;
  return diag_hash_run(op, buf, buf_sz, in, out, n);
}

/* the proof-of-history hashes: op 0 SHA256_LEAF65, 1 SHA256_NODE65, 2 SHA256_CHAIN32, 3 SHA256_MIX64; everything
   else as fd_ed25519_diag_hash */
extern "C" int fd_ed25519_diag_poh_hash(int op, const uint8_t* buf, unsigned long buf_sz, const uint32_t* in, uint32_t* out,
                                        unsigned long n) {
  if (op < 0 || op >= HASH_OP_END - HASH_OP_N) return (int)hipErrorInvalidValue;
  return diag_hash_run(HASH_OP_N + op, buf, buf_sz, in, out, n);
}
