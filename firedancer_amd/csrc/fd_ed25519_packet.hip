/* fd_ed25519_packet.hip -- signed gossip and repair control packets
   (include/fd_ed25519_hip.h Part 2d): what fd_gossip_recv_packet does for a
   ping, a pong and a prune message (src/flamenco/gossip/fd_gossip.c:646-656,
   :940-949, :1201-1236) and fd_repair_recv_serv_packet for a window_index,
   highest_window_index and orphan request
   (src/flamenco/repair/fd_repair.c:1012-1070) before they call
   fd_ed25519_verify, in front of the engine's verify phases.  One lane per
   packet:

     stage  fd_packet_core.h's rules; then signature and key into the
            16-byte-aligned SoA and the message into the workspace's mirror
            of the packet buffer, at the position congruent mod 16 to its
            source bytes (below); msg_off / msg_sz point there.  A packet
            that is not judged leaves a dummy slot (zero signature and key,
            empty message) whose verify code nothing reads.
     verify the engine's phases over the n slots
            (host/fd_ed25519_hip_fronts.c)
     finish the stage's code, else ERR_SIGNATURE for a verify code other
            than success, else 0; the optional verify codes

   The mirrored message area.  A message is one or two runs of packet bytes
   with one 64-byte gap taken out (the signature, every time): a ping's or
   pong's token [36,68) as it lies; a prune's [36,76+32m) as it lies and
   [140+32m,180+32m) 64 bytes lower; a repair request's [68,sz) as it lies
   and its discriminant [0,4) 64 bytes higher, at [64,68).  Written at the
   same offset of a buffer as aligned as the packets', every run moves by 0
   or 64 bytes, so the copy is whole aligned 16-byte granules: aligned loads,
   aligned stores, and a byte select in the one granule where the two runs
   meet.  A lane stores whole granules, so up to 15 bytes before and behind
   its message get packet bytes nobody reads.  Those lie at packet offsets
   21.. (before: the lowest message starts at 36) and below 15 of whatever
   follows the packet (behind: only a repair message ends with its packet),
   so inside no other lane's granules, which start at packet offset 21 or
   above, as long as packets do not overlap; and below pkt_bytes rounded up
   to 16, which the area covers. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/fd_ed25519_hip.h"
#include "fd_ed25519_hip_internal.h"
#include "fd_front_dev.h"

/* 32 packet bytes against the identity in the launch's arguments */
__device__ static inline int key_ne_any(const uint8_t* p, const uint32_t* key) {
  const uint4 a = load16_any(p), b = load16_any(p + 16);
  return ((a.x ^ key[0]) | (a.y ^ key[1]) | (a.z ^ key[2]) | (a.w ^ key[3]) | (b.x ^ key[4]) | (b.y ^ key[5]) |
          (b.z ^ key[6]) | (b.w ^ key[7])) != 0u;
}

#define FD_PACKET_FN __device__ static inline
#define FD_PACKET_U32(p) load4_any(p)
#define FD_PACKET_U64(p) load8_any(p)
#define FD_PACKET_KEY_T const uint32_t*
#define FD_PACKET_KEY_NE(p, key) key_ne_any(p, key)
#include "fd_packet_core.h"

static_assert(FD_ED25519_HIP_PACKET_OK == 0 && FD_ED25519_SUCCESS == 0, "front_verdict's zeros");

/* bytes [0,k) of lo, [k,16) of hi, 0 < k < 16 */
__device__ static inline uint32_t merge4(uint32_t lo, uint32_t hi, int k) {   /* k: bytes of lo in this dword, any int */
  if (k <= 0) return hi;
  if (k >= 4) return lo;
  const uint32_t mask = (1u << (8 * k)) - 1u;
  return (lo & mask) | (hi & ~mask);
}

__device__ static inline uint4 merge16(uint4 lo, uint4 hi, int k) {
  return make_uint4(merge4(lo.x, hi.x, k), merge4(lo.y, hi.y, k - 4), merge4(lo.z, hi.z, k - 8), merge4(lo.w, hi.w, k - 12));
}

/* one wave per block, as the shred stage: single-wave blocks spread a small
   batch over the most SIMDs */
#define FD_PACKET_STAGE_BLOCK 64

__global__ void __launch_bounds__(FD_PACKET_STAGE_BLOCK)
fd_ed25519_packet_stage_kernel(fd_ed25519_packet_stage_params_t p) {
  const uint64_t i = (uint64_t)blockIdx.x * FD_PACKET_STAGE_BLOCK + threadIdx.x;
  if (i >= p.n) return;
  const uint64_t off = p.pkt_off[i];
  const uint64_t sz = p.pkt_sz[i];
  fd_packet_core_plan_t c;
  int pre = FD_PACKET_CORE_ERR_PARSE;   /* a packet that leaves [0,pkt_bytes) is not read */
  if (sz <= p.pkt_bytes && off <= p.pkt_bytes - sz) pre = fd_packet_core_plan(p.proto, p.pkts + off, sz, p.self_key, &c);
  uint4* sg = reinterpret_cast<uint4*>(p.sigs + 64 * i);
  uint4* pk = reinterpret_cast<uint4*>(p.pubs + 32 * i);
  p.pre[i] = (int8_t)pre;
  if (pre) {
    FRONT_SLOT_ZERO(sg, pk);
    p.msg_off[i] = 0UL;
    p.msg_sz[i] = 0u;
    return;
  }
  const uint8_t* s = p.pkts + off;
  FRONT_SLOT_GATHER(sg, pk, s + c.sig_off, s + c.key_off);

  /* the message's place in the mirror: its first run's own place, but for a
     repair request its second run's, the discriminant 64 bytes up in front
     of it; sh0, sh1: source minus destination of each run (0 or -64, 0 or
     64; a message of one run reads its tail granule through sh0 too) */
  const uint32_t first = c.msg0_off == 0 ? (uint32_t)c.msg1_off - c.msg0_sz : (uint32_t)c.msg0_off;
  const uint64_t a = off + first, mid = a + c.msg0_sz, end = mid + c.msg1_sz;
  const int64_t sh0 = (int64_t)c.msg0_off - (int64_t)first;
  const int64_t sh1 = c.msg1_sz ? (int64_t)c.msg1_off - (int64_t)(first + c.msg0_sz) : sh0;
  for (uint64_t g = a & ~(uint64_t)15; g < end; g += 16) {
    uint4 v;
    if (g + 16 <= mid) {
      v = *reinterpret_cast<const uint4*>(p.pkts + (g + sh0));
    } else if (g >= mid) {
      v = *reinterpret_cast<const uint4*>(p.pkts + (g + sh1));
    } else {
      v = merge16(*reinterpret_cast<const uint4*>(p.pkts + (g + sh0)), *reinterpret_cast<const uint4*>(p.pkts + (g + sh1)),
                  (int)(mid - g));
    }
    *reinterpret_cast<uint4*>(p.msgs + g) = v;
  }
  p.msg_off[i] = a;
  p.msg_sz[i] = (uint32_t)(end - a);
}

__global__ void __launch_bounds__(256)
fd_ed25519_packet_finish_kernel(fd_ed25519_packet_finish_params_t p) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const int pre = p.pre[i];
  const int sig = pre ? 0 : p.codes[i];   /* a dummy slot's verify code is never read */
  p.out[i] = (int8_t)front_verdict(pre, sig, FD_ED25519_HIP_PACKET_ERR_SIGNATURE);
  if (p.sig_out) p.sig_out[i] = (int8_t)sig;
}

extern "C" int fd_ed25519_hip_launch_packet_stage(const fd_ed25519_packet_stage_params_t* p, void* stream) {
  return front_launch_1d(fd_ed25519_packet_stage_kernel, FD_PACKET_STAGE_BLOCK, p->n, stream, *p);
}

extern "C" int fd_ed25519_hip_launch_packet_finish(const fd_ed25519_packet_finish_params_t* p, void* stream) {
  return front_launch_1d(fd_ed25519_packet_finish_kernel, 256, p->n, stream, *p);
}
