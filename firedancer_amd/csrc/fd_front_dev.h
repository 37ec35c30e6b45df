/* fd_front_dev.h -- what the stage and finish kernels of the fronts before
   the verify phases share (fd_ed25519_txn.hip, fd_ed25519_shred.hip,
   fd_ed25519_packet.hip, fd_ed25519_crds.hip; DESIGN.md 3a, "The shape of a
   front"). */
#ifndef FD_FRONT_DEV_H
#define FD_FRONT_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* 4, 8 and 16 bytes at any byte address, from dword-aligned loads.  The
   last dword is loaded only when the address is not dword-aligned, so a
   load reads at most 3 bytes past its own; every front asks for a source
   buffer readable 16 bytes past its end (the payload, shred and packet
   staging allocations leave that room), which covers it. */
__device__ static inline uint32_t load4_any(const uint8_t* src) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(src);
  const uint32_t* w = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  const uint32_t sh = (uint32_t)(a & 3);
  const uint32_t d0 = w[0], d1 = sh ? w[1] : 0u;
  return __builtin_amdgcn_alignbyte(d1, d0, sh);
}

__device__ static inline uint64_t load8_any(const uint8_t* src) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(src);
  const uint32_t* w = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  const uint32_t sh = (uint32_t)(a & 3);
  const uint32_t d0 = w[0], d1 = w[1], d2 = sh ? w[2] : 0u;
  return (uint64_t)__builtin_amdgcn_alignbyte(d1, d0, sh) | ((uint64_t)__builtin_amdgcn_alignbyte(d2, d1, sh) << 32);
}

__device__ static inline uint4 load16_any(const uint8_t* src) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(src);
  const uint32_t* w = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  const uint32_t sh = (uint32_t)(a & 3);
  const uint32_t d0 = w[0], d1 = w[1], d2 = w[2], d3 = w[3], d4 = sh ? w[4] : 0u;
  return make_uint4(__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh),
                    __builtin_amdgcn_alignbyte(d3, d2, sh), __builtin_amdgcn_alignbyte(d4, d3, sh));
}

/* A slot of the signature array (sg, 64 bytes) and of the key array (pk, 32
   bytes), both 16-byte aligned, from the bytes at sig_src and key_src -- and
   the dummy slot: zero signature, zero key (the shred front's roots are 32
   bytes a slot as well).  Macros, and over the slot's two pointers, which the
   caller forms once ahead of the branch between the two: as functions, over
   pointers or over (sigs, pubs, k), these compiled to stage kernels whose
   instructions differed from the hand-written stores' (the address arithmetic
   moved, and with it the schedule and the register allocation).  A source
   expression is evaluated where its load stands. */
#define FRONT_SIG_GATHER(sg, sig_src)                                                            \
  do {                                                                                           \
    _Pragma("unroll") for (int q_ = 0; q_ < 4; q_++) (sg)[q_] = load16_any((sig_src) + 16 * q_); \
  } while (0)

#define FRONT_SLOT_GATHER(sg, pk, sig_src, key_src) \
  do {                                              \
    FRONT_SIG_GATHER(sg, sig_src);                  \
    (pk)[0] = load16_any(key_src);                  \
    (pk)[1] = load16_any((key_src) + 16);           \
  } while (0)

#define FRONT_SLOT_ZERO(sg, pk)                                     \
  do {                                                              \
    const uint4 z_ = make_uint4(0u, 0u, 0u, 0u);                    \
    _Pragma("unroll") for (int q_ = 0; q_ < 4; q_++) (sg)[q_] = z_; \
    (pk)[0] = z_;                                                   \
    (pk)[1] = z_;                                                   \
  } while (0)

/* the finish rule of the shred and packet fronts: the stage's code, else
   err_signature for a verify code other than success (0), else 0.  The
   caller passes code 0 for a dummy slot (pre != 0): its verify code is never
   read. */
__device__ static inline int front_verdict(int pre, int code, int err_signature) {
  return pre ? pre : code != 0 ? err_signature : 0;
}

/* kernel over n items, one lane each, in blocks of blk; nothing for n = 0 */
template <typename K, typename... A>
static inline int front_launch_1d(K kernel, uint32_t blk, uint64_t n, void* stream, A... args) {
  if (!n) return 0;
  hipLaunchKernelGGL(kernel, dim3((uint32_t)((n + blk - 1) / blk)), dim3(blk), 0, (hipStream_t)stream, args...);
  return (int)hipGetLastError();
}

#endif /* FD_FRONT_DEV_H */
