/* fd_ed25519_shred.hip -- the leader signatures of Merkle shreds
   (include/fd_ed25519_hip.h Part 2c): what fd_fec_resolver_add_shred
   (src/disco/shred/fd_fec_resolver.c:283-440) does for a shred that opens a
   FEC set before it calls fd_ed25519_verify, in front of the engine's
   verify phases.  One lane per shred:

     stage  fd_shred_core.h's parse and header rules, then the leaf hash and
            the walk up the inclusion proof (fd_sha256_dev.h); the root goes
            into the workspace as a 32-byte verify message, the signature
            into the 16-byte-aligned SoA, msg_off / msg_sz point at the
            root; the leaders array is the verify phases' key array as it
            is.  A shred that is not judged leaves a dummy slot (zero
            signature, empty message) whose verify code nothing reads.
     verify the engine's phases over the n slots
            (host/fd_ed25519_hip_fronts.c)
     finish the stage's code, else ERR_SIGNATURE for a verify code other
            than success, else 0; the optional roots and verify codes */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/fd_ed25519_hip.h"
#include "fd_ed25519_hip_internal.h"
#include "fd_front_dev.h"

#define FD_SHRED_FN __device__ static inline
#include "fd_shred_core.h"

#define FD_DEV __device__ __forceinline__
#include "fd_sha256_dev.h"

static_assert(FD_ED25519_HIP_SHRED_OK == 0 && FD_ED25519_SUCCESS == 0, "front_verdict's zeros");

/* one wave per block: a lane's work is a chain of about 30 compressions,
   and single-wave blocks spread a small batch over the most SIMDs */
#define FD_SHRED_STAGE_BLOCK 64

__global__ void __launch_bounds__(FD_SHRED_STAGE_BLOCK)
fd_ed25519_shred_stage_kernel(fd_ed25519_shred_stage_params_t p) {
  const uint64_t i = (uint64_t)blockIdx.x * FD_SHRED_STAGE_BLOCK + threadIdx.x;
  if (i >= p.n) return;
  const uint8_t* s = p.shreds + p.shred_off[i];
  fd_shred_core_t c;
  const int pre = fd_shred_core_judge(s, p.shred_sz[i], &c);
  uint4* sg = reinterpret_cast<uint4*>(p.sigs + 64 * i);
  uint4* rt = reinterpret_cast<uint4*>(p.roots + 32 * i);
  p.msg_off[i] = 32 * i;
  p.pre[i] = (int8_t)pre;
  if (pre) {
    FRONT_SLOT_ZERO(sg, rt);   /* the key array is the caller's leaders: a zero root in the key's place */
    p.msg_sz[i] = 0u;
    return;
  }
  FRONT_SIG_GATHER(sg, s);
  uint32_t h[8];
  sha256_shred_root(h, s, c);
  rt[0] = make_uint4(__builtin_bswap32(h[0]), __builtin_bswap32(h[1]), __builtin_bswap32(h[2]), __builtin_bswap32(h[3]));
  rt[1] = make_uint4(__builtin_bswap32(h[4]), __builtin_bswap32(h[5]), __builtin_bswap32(h[6]), __builtin_bswap32(h[7]));
  p.msg_sz[i] = 32u;
}

__global__ void __launch_bounds__(256)
fd_ed25519_shred_finish_kernel(fd_ed25519_shred_finish_params_t p) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const int pre = p.pre[i];
  const int sig = pre ? 0 : p.codes[i];   /* a dummy slot's verify code is never read */
  p.out[i] = (int8_t)front_verdict(pre, sig, FD_ED25519_HIP_SHRED_ERR_SIGNATURE);
  if (p.sig_out) p.sig_out[i] = (int8_t)sig;
  if (p.roots_out) {
    const uint4* src = reinterpret_cast<const uint4*>(p.roots + 32 * i);
    uint4* dst = reinterpret_cast<uint4*>(p.roots_out + 32 * i);   /* 16-byte aligned: shreds_dev checks */
    dst[0] = src[0];
    dst[1] = src[1];
  }
}

extern "C" int fd_ed25519_hip_launch_shred_stage(const fd_ed25519_shred_stage_params_t* p, void* stream) {
  return front_launch_1d(fd_ed25519_shred_stage_kernel, FD_SHRED_STAGE_BLOCK, p->n, stream, *p);
}

extern "C" int fd_ed25519_hip_launch_shred_finish(const fd_ed25519_shred_finish_params_t* p, void* stream) {
  return front_launch_1d(fd_ed25519_shred_finish_kernel, 256, p->n, stream, *p);
}
