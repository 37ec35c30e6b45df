/* fd_ed25519_crds.hip -- the CRDS values of gossip pull responses and push
   messages (include/fd_ed25519_hip.h Part 2e): what fd_gossip_recv_packet
   and fd_gossip_recv_crds_value (src/flamenco/gossip/fd_gossip.c:1858-1878,
   :1420-1430, :1020-1105) do for every value before they call
   fd_ed25519_verify, in front of the engine's verify phases.

     stage  one lane per packet: fd_crds_core.h's walk of the whole packet,
            then value by value the signature and the chosen key into the
            16-byte-aligned SoA of the slots the caller reserved; the
            message stays in place in the packet buffer, msg_off / msg_sz
            point there.  A value under the own identity, a contact_info_v2
            (whose re-encode is never the received run: UNSUPPORTED) and
            every slot of a packet without verdicts is a dummy slot (zero
            signature and key, empty message) whose verify code nothing
            reads.
     verify the engine's phases over the n_val slots
            (host/fd_ed25519_hip_fronts.c)
     finish per value the stage's code, else ERR_SIGNATURE for a verify code
            other than success, else 0, and the optional verify codes; per
            packet its code
     hash   only when asked for, one lane per value: SHA-256 of the value's
            own bytes (fd_sha256_dev.h's sha256_bytes) */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/fd_ed25519_hip.h"
#include "../../include/fd_ed25519_hip_tile.h"
#include "fd_ed25519_hip_internal.h"
#include "fd_front_dev.h"

/* 32 packet bytes against the identity in the launch's arguments */
__device__ static inline int crds_key_ne_any(const uint8_t* p, const uint32_t* key) {
  const uint4 a = load16_any(p), b = load16_any(p + 16);
  return ((a.x ^ key[0]) | (a.y ^ key[1]) | (a.z ^ key[2]) | (a.w ^ key[3]) | (b.x ^ key[4]) | (b.y ^ key[5]) |
          (b.z ^ key[6]) | (b.w ^ key[7])) != 0u;
}

#define FD_TXN_FN __device__ static inline
#include "fd_txn_parse_core.h"

#define FD_CRDS_FN __device__ static inline
#define FD_CRDS_U32(p) load4_any(p)
#define FD_CRDS_U64(p) load8_any(p)
#define FD_CRDS_KEY_T const uint32_t*
#define FD_CRDS_KEY_NE(p, key) crds_key_ne_any(p, key)
#include "fd_crds_core.h"

#define FD_SHRED_FN __device__ static inline
#include "fd_shred_core.h"
#define FD_DEV __device__ __forceinline__
#include "fd_sha256_dev.h"

static_assert(FD_ED25519_HIP_CRDS_OK == 0 && FD_ED25519_SUCCESS == 0, "front_verdict's zeros");
static_assert(FD_ED25519_HIP_CRDS_VAL_MAX == FD_CRDS_CORE_VAL_MAX, "value bound");

/* one wave per block, as the packet stage: single-wave blocks spread a
   small batch over the most SIMDs */
#define FD_CRDS_STAGE_BLOCK 64

/* the slots val_first reserves for packet i: [*first, *first + n) inside
   [0, n_val) -- or -1 when val_first does not describe such a range (then no
   slot of i is touched).  A range of more than VAL_MAX slots is one: no
   packet decodes to so many, so all of them get a code and none a verify
   (the engine has put every slot into a state the verify phases can read,
   crds_dev: a slot no lane fills is no wild message offset). */
__device__ static inline int64_t crds_slots(const uint32_t* val_first, uint64_t i, uint64_t n_val, uint32_t* first) {
  const uint32_t f = val_first[i], l = val_first[i + 1];
  *first = f;
  if (l < f || (uint64_t)l > n_val) return -1;
  return (int64_t)(l - f);
}

__global__ void __launch_bounds__(FD_CRDS_STAGE_BLOCK)
fd_ed25519_crds_stage_kernel(fd_ed25519_crds_stage_params_t p) {
  const uint64_t i = (uint64_t)blockIdx.x * FD_CRDS_STAGE_BLOCK + threadIdx.x;
  if (i >= p.n) return;
  const uint64_t off = p.pkt_off[i];
  const uint64_t sz = p.pkt_sz[i];
  uint32_t first;
  const int64_t reserved = crds_slots(p.val_first, i, p.n_val, &first);
  const uint32_t slots = reserved < 0 ? 0u : (uint32_t)reserved;
  const bool inside = sz <= p.pkt_bytes && off <= p.pkt_bytes - sz;   /* a packet that leaves [0,pkt_bytes) is not read */
  const uint64_t base = inside ? off : 0UL;
  const uint8_t* s = p.pkts + base;
  fd_crds_core_idx_t idx;
  idx.cnt = 0u;
  int status = FD_CRDS_CORE_ERR_PARSE;
  if (inside) status = fd_crds_core_walk(s, sz, &idx);
  /* the slots are filled from this walk, so a reservation made from another
     count (a packet changed since the host counted it) fills none of them */
  if (!status && (reserved < 0 || idx.cnt != slots)) status = FD_ED25519_HIP_CRDS_BAD_RESERVATION;
  p.status[i] = (int8_t)status;
  for (uint32_t j = 0; j < slots; j++) {
    const uint64_t k = (uint64_t)first + j;
    uint4* sg = reinterpret_cast<uint4*>(p.sigs + 64 * k);
    uint4* pk = reinterpret_cast<uint4*>(p.pubs + 32 * k);
    if (status) {
      FRONT_SLOT_ZERO(sg, pk);
      p.msg_off[k] = base;
      p.msg_sz[k] = 0u;
      p.val_sz[k] = 0u;
      p.pre[k] = (int8_t)status;
      continue;
    }
    fd_crds_core_val_t v;
    fd_crds_core_value(s, sz, &idx, j, p.self_key, &v);
    if (!v.pre) {
      FRONT_SLOT_GATHER(sg, pk, s + v.sig_off, s + v.key_off);
    } else {
      FRONT_SLOT_ZERO(sg, pk);
    }
    p.msg_off[k] = base + v.msg_off;
    p.msg_sz[k] = v.pre ? 0u : (uint32_t)v.msg_sz;
    p.val_sz[k] = fd_crds_core_reencodes(v.disc) ? (uint32_t)v.msg_sz : 0u;   /* no hash the reference would not take */
    p.pre[k] = v.pre;
  }
}

__global__ void __launch_bounds__(256)
fd_ed25519_crds_finish_kernel(fd_ed25519_crds_finish_params_t p) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < p.n) p.pkt_out[k] = p.status[k];
  if (k >= p.n_val) return;
  const int pre = p.pre[k];
  const int sig = pre ? 0 : p.codes[k];   /* a dummy slot's verify code is never read */
  p.val_out[k] = (int8_t)front_verdict(pre, sig, FD_ED25519_HIP_CRDS_ERR_SIGNATURE);
  if (p.sig_out) p.sig_out[k] = (int8_t)sig;
}

__global__ void __launch_bounds__(FD_CRDS_STAGE_BLOCK)
fd_ed25519_crds_hash_kernel(fd_ed25519_crds_hash_params_t p) {
  const uint64_t k = (uint64_t)blockIdx.x * FD_CRDS_STAGE_BLOCK + threadIdx.x;
  if (k >= p.n_val) return;
  uint32_t* out = reinterpret_cast<uint32_t*>(p.hash_out + 32 * k);
  const uint32_t vsz = p.val_sz[k];
  uint32_t h[8];
  if (vsz) {
    sha256_bytes(h, p.pkts + p.msg_off[k] - 64, 64u + vsz);   /* the signature lies in front of the data */
#pragma unroll
    for (int q = 0; q < 8; q++) out[q] = __builtin_bswap32(h[q]);
  } else {
#pragma unroll
    for (int q = 0; q < 8; q++) out[q] = 0u;
  }
}

extern "C" int fd_ed25519_hip_launch_crds_stage(const fd_ed25519_crds_stage_params_t* p, void* stream) {
  return front_launch_1d(fd_ed25519_crds_stage_kernel, FD_CRDS_STAGE_BLOCK, p->n, stream, *p);
}

extern "C" int fd_ed25519_hip_launch_crds_finish(const fd_ed25519_crds_finish_params_t* p, void* stream) {
  return front_launch_1d(fd_ed25519_crds_finish_kernel, 256, p->n > p->n_val ? p->n : p->n_val, stream, *p);
}

extern "C" int fd_ed25519_hip_launch_crds_hash(const fd_ed25519_crds_hash_params_t* p, void* stream) {
  return front_launch_1d(fd_ed25519_crds_hash_kernel, FD_CRDS_STAGE_BLOCK, p->n_val, stream, *p);
}
