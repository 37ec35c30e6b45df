/* fd_ed25519_recover.hip -- recovering received FEC sets (include/fd_ed25519_hip.h
   Part 2h): what fd_fec_resolver_add_shred does from the moment a set's d-th
   shred is in (src/disco/shred/fd_fec_resolver.c:474-572 on
   fd_reedsol_recover_fini) up to the Merkle tree, which is
   fd_ed25519_fec.hip's.  One launch, one workgroup per set, in the shape of
   the parity kernel (fd_ed25519_reedsol.hip):

     judge    fd_fec_core.h's rules 1-2 on the received slots and
              fd_reedsol_core.h's rules 9-10 reduced to one code per set with
              LDS atomicMin words: the first failing slot, the first received
              code shred (whose data_cnt is d), the first received slot
     basis    a prefix count of the received flags with one ballot a wave:
              the first d received slots are the sources, every other slot a
              target -- the received ones first (they are compared), then the
              erased ones (they are written)
     matrix   log D_r per source and log N_e per target from the engine's
              log / exp tables (d additions each), then one coefficient
              L[e][r] = N_e / ((e ^ r) D_r) a lane into LDS
     compare  the column loop (fd_reedsol_dev.h, fd_reedsol_rows) over the
              received targets, the differences OR-reduced over the
              workgroup: ERR_CORRUPT before any store
     headers  the first seven columns of the erased data shreds into LDS, and
              rule 11 on the data headers as they would stand
     recover  the column loop over the erased targets, the sources from a
              per-source offset kept in LDS (a data shred's region starts at
              0x40, a code shred's at 0x59); then the signature and, of a code
              shred, the header of every erased slot

   The region's stores are the column loop's, under its one rule; bytes
   [0, 0x40) or [0, 0x59) of an erased slot go out as aligned dwords wholly
   inside that range and bytes at its two ends.  No store covers a byte
   outside what rule 12 names. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/fd_ed25519_hip.h"
#include "fd_ed25519_hip_internal.h"
#include "fd_front_dev.h"

#define FD_SHRED_FN __device__ static inline
#include "fd_reedsol_core.h"
#include "fd_reedsol_dev.h"

#define FD_RC_ROW_MAX 160   /* at most 133 targets; a pass may start at any row and runs to a multiple of 8 behind it */
#define FD_RC_HDR_COLS 7    /* the columns that hold a data shred's bytes [0x40, 0x59) */

struct rc_lds_t {
  uint4    mul[FD_REEDSOL_CORE_MUL_BYTES / 16];          /* [256][2]: T0 T1 | T2 pad */
  uint32_t coef[FD_RC_ROW_MAX * FD_REEDSOL_STRIDE / 4];  /* [target row][68], zero beyond the set's d and targets */
  uint64_t src[FD_REEDSOL_CORE_MAX + 1];                 /* where source i's region starts in p.shreds */
  uint32_t hdr[FD_REEDSOL_CORE_MAX * FD_RC_HDR_COLS];    /* bytes [0x40, 0x5c) of every data shred as after recovery */
  fd_reedsol_core_gf_t gf;
  uint8_t  basis[FD_REEDSOL_STRIDE];                     /* the slot of source i */
  uint8_t  log_d[FD_REEDSOL_STRIDE];
  uint8_t  tgt[FD_RC_ROW_MAX];                           /* the slot of target row r */
  uint8_t  log_n[FD_RC_ROW_MAX];
  uint8_t  erased[FD_FEC_CORE_CNT_MAX + 2];
  uint8_t  sig[64];                                      /* of the first received shred */
  uint8_t  ref[28];                                      /* bytes [0x40, 0x59) of the first received code shred */
  uint64_t ballot[2][FD_REEDSOL_BLOCK / 64];             /* received; erased data */
  uint32_t first_bad;    /* (j << 8 | code) of the first failing slot */
  uint32_t first_code;   /* the first received code shred the rules pass */
  uint32_t first_rcvd;
  uint32_t flag;         /* bit 0: a compared target differs; bit 1: rule 11 */
};

/* The column loop over the target rows [row0, row1): STORE writes them (they
   are erased slots), else they are compared and the differences returned. */
template <bool STORE>
__device__ __forceinline__ uint32_t rc_rows(const fd_ed25519_fec_recover_params_t& p, const rc_lds_t& s, const uint64_t first,
                                            const uint32_t d, const uint32_t region, const uint32_t row0, const uint32_t row1) {
  return fd_reedsol_rows<STORE>(
      s.mul, s.coef, d, region, row0, row1, [&](const uint32_t i) { return p.shreds + s.src[i]; },
      [&](const uint32_t r) {
        const uint32_t e = s.tgt[r];
        return p.shreds + p.shred_off[first + e] + fd_reedsol_core_region_at(e, d);
      });
}

/* five waves a SIMD: 87 VGPRs without a spill where the compiler's own choice is 100 (four waves); measured 7 %
   faster on 4,096 sets of 32 + 32.  Six waves (80 VGPRs) spill. */
__global__ void __launch_bounds__(FD_REEDSOL_BLOCK) __attribute__((amdgpu_waves_per_eu(5, 5)))
fd_ed25519_fec_recover_kernel(fd_ed25519_fec_recover_params_t p) {
  __shared__ rc_lds_t s;
  const uint32_t k = blockIdx.x, t = threadIdx.x;
  const uint64_t first = p.set_first[k], last = p.set_first[k + 1];
  /* a set_first that is no prefix sum: a range that runs backwards or leaves [0, n) is rule 1's */
  const bool range_ok = first <= last && last <= p.n && last - first >= 1 && last - first <= FD_FEC_CORE_CNT_MAX;
  const uint32_t cnt = range_ok ? (uint32_t)(last - first) : 0u;
  if (t == 0) { s.first_bad = 0xffffffffu; s.first_code = cnt; s.first_rcvd = cnt; s.flag = 0u; }
  __syncthreads();

  /* ---- judge: lane j has slot j (cnt <= 134 < the block) ---- */
  const bool have = t < cnt;
  const bool er = have && p.erased[first + t] != 0;
  const uint8_t* mine = have ? p.shreds + p.shred_off[first + t] : nullptr;
  const uint32_t mine_sz = have ? p.shred_sz[first + t] : 0u;
  int own = FD_FEC_CORE_OK;
  if (have) {
    s.erased[t] = er;
    if (!er) {
      fd_shred_core_t c;
      own = fd_fec_core_judge(mine, mine_sz, cnt, t, &c);
      if (own) atomicMin(&s.first_bad, (t << 8) | ((uint32_t)own & 0xffu));
      else if ((mine[0x40] & 0xf0u) == 0x40u) atomicMin(&s.first_code, t);
      atomicMin(&s.first_rcvd, t);
    }
  }
  __syncthreads();
  const uint32_t fc = s.first_code, fr = s.first_rcvd;
  const uint32_t d = fc < cnt ? fd_shred_core_u16(p.shreds + p.shred_off[first + fc] + 0x53) : cnt;
  if (have && !own) {
    const int code = fd_reedsol_core_recover_judge(mine, mine_sz, er, cnt, t, d);
    if (code) atomicMin(&s.first_bad, (t << 8) | ((uint32_t)code & 0xffu));
  }
  /* ---- basis: the rank of a slot among the received ones ---- */
  const bool rcvd = have && !er;
  const uint64_t b_rcvd = __ballot(rcvd), b_erd = __ballot(er && t < d);
  if ((t & 63u) == 0u) { s.ballot[0][t >> 6] = b_rcvd; s.ballot[1][t >> 6] = b_erd; }
  __syncthreads();
  uint32_t nrcv = 0u, ned = 0u, rank = 0u;
  for (uint32_t w = 0; w < FD_REEDSOL_BLOCK / 64; w++) {
    const uint32_t c = (uint32_t)__popcll(s.ballot[0][w]);
    if (w < (t >> 6)) rank += c;
    nrcv += c;
    ned += (uint32_t)__popcll(s.ballot[1][w]);
  }
  rank += (uint32_t)__popcll(b_rcvd & ((1ull << (t & 63u)) - 1ull));
  const uint32_t bad = s.first_bad;
  const int set_code = !range_ok ? FD_FEC_CORE_ERR_SET
                     : bad != 0xffffffffu ? (int)(int8_t)(bad & 0xffu)
                     : fc == cnt ? FD_FEC_CORE_ERR_SET
                     : nrcv < d ? FD_REEDSOL_CORE_ERR_PARTIAL : FD_FEC_CORE_OK;
  if (set_code) {   /* rule 12: nothing of the set's slots is written */
    if (t == 0) p.set_out[k] = (int8_t)set_code;
    return;
  }

  /* 1 <= d <= 67 sources, ntgt = cnt - d targets (1 <= ntgt <= 133): rows [0, ncmp) received, [ncmp, ntgt) erased,
     of which the first ned are data shreds */
  const uint32_t ncmp = nrcv - d, ntgt = cnt - d;
  const uint32_t depth = fd_fec_core_depth(cnt), region = FD_REEDSOL_CORE_REGION(depth);
  if (have) {
    if (rcvd && rank < d) {
      s.basis[rank] = (uint8_t)t;
      s.src[rank] = p.shred_off[first + t] + fd_reedsol_core_region_at(t, d);
    } else {
      s.tgt[rcvd ? rank - d : ncmp + (t - rank)] = (uint8_t)t;
    }
  }
  const uint4* gmul = reinterpret_cast<const uint4*>(p.tab);
  for (uint32_t q = t; q < FD_REEDSOL_CORE_MUL_BYTES / 16; q += FD_REEDSOL_BLOCK) s.mul[q] = gmul[q];
  for (uint32_t q = t; q < FD_RC_ROW_MAX * FD_REEDSOL_STRIDE / 4; q += FD_REEDSOL_BLOCK) s.coef[q] = 0u;
  {
    const uint32_t* ggf = reinterpret_cast<const uint32_t*>(p.tab + FD_REEDSOL_CORE_GF_AT);
    uint32_t* lgf = reinterpret_cast<uint32_t*>(&s.gf);
    for (uint32_t q = t; q < sizeof(fd_reedsol_core_gf_t) / 4; q += FD_REEDSOL_BLOCK) lgf[q] = ggf[q];
  }
  if (t < 64) s.sig[t] = p.shreds[p.shred_off[first + fr] + t];
  if (t < FD_REEDSOL_CORE_HDR_BYTES) s.ref[t] = p.shreds[p.shred_off[first + fc] + 0x40u + t];
  __syncthreads();
  if (t < d) s.log_d[t] = (uint8_t)fd_reedsol_core_log_d(&s.gf, s.basis, d, s.basis[t]);
  if (t < ntgt) s.log_n[t] = (uint8_t)fd_reedsol_core_log_n(&s.gf, s.basis, d, s.tgt[t]);
  __syncthreads();
  uint8_t* coef8 = reinterpret_cast<uint8_t*>(s.coef);
  for (uint32_t q = t; q < ntgt * d; q += FD_REEDSOL_BLOCK) {
    const uint32_t r = q / d, i = q % d;
    coef8[r * FD_REEDSOL_STRIDE + i] = (uint8_t)fd_reedsol_core_coef(&s.gf, s.log_n[r], s.log_d[i], s.tgt[r], s.basis[i]);
  }
  __syncthreads();

  /* ---- compare the received targets; the data headers as they would stand ---- */
  if (ncmp) {
    const uint32_t diff = rc_rows<false>(p, s, first, d, region, 0u, ncmp);
    if (diff) atomicOr(&s.flag, 1u);
  }
  for (uint32_t q = t; q < ned * 8u; q += FD_REEDSOL_BLOCK) {
    const uint32_t col = q & 7u, r = ncmp + (q >> 3);
    if (col < FD_RC_HDR_COLS) {
      uint32_t acc = 0u;
      for (uint32_t i0 = 0; i0 < d; i0 += 8) {   /* eight loads in flight: these lanes have one row each */
        uint32_t x[8];
#pragma unroll
        for (int u = 0; u < 8; u++) x[u] = i0 + u < d ? load4_any(p.shreds + s.src[i0 + u] + 4u * col) : 0u;
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const uint32_t c = coef8[r * FD_REEDSOL_STRIDE + i0 + u];   /* zero beyond d */
          acc ^= fd_reedsol_mul(s.mul[2 * c], s.mul[2 * c + 1].x, x[u] & 0x07070707u, (x[u] >> 3) & 0x07070707u, (x[u] >> 6) & 0x03030303u);
        }
      }
      s.hdr[s.tgt[r] * FD_RC_HDR_COLS + col] = acc;
    }
  }
  for (uint32_t q = t; q < d * 8u; q += FD_REEDSOL_BLOCK) {
    const uint32_t col = q & 7u, j = q >> 3;
    if (col < FD_RC_HDR_COLS && !s.erased[j])
      s.hdr[j * FD_RC_HDR_COLS + col] = load4_any(p.shreds + p.shred_off[first + j] + 0x40u + 4u * col);
  }
  __syncthreads();
  if (s.flag & 1u) {
    if (t == 0) p.set_out[k] = (int8_t)FD_REEDSOL_CORE_ERR_CORRUPT;
    return;
  }
  if (have) {   /* rule 11 */
    const uint8_t* hdr8 = reinterpret_cast<const uint8_t*>(s.hdr);
    int code = FD_FEC_CORE_OK;
    if (t < d) {
      const uint8_t* h = hdr8 + 4u * FD_RC_HDR_COLS * t;
      if (er) code = fd_reedsol_core_hdr_judge(h, cnt, t);
      if (!code) code = fd_reedsol_core_hdr_agree(h, hdr8, 1);
    } else if (!er) {
      code = fd_reedsol_core_hdr_agree(mine + 0x40, hdr8, 0);
    }
    if (code) atomicOr(&s.flag, 2u);
  }
  __syncthreads();
  if (s.flag) {
    if (t == 0) p.set_out[k] = (int8_t)FD_FEC_CORE_ERR_SET;
    return;
  }
  if (t == 0) p.set_out[k] = (int8_t)FD_FEC_CORE_OK;

  /* ---- recover: the erased targets, then their signatures and code headers ---- */
  rc_rows<true>(p, s, first, d, region, ncmp, ntgt);
  /* bytes [0, H) of an erased slot, H = 0x40 or 0x59: lane 0 of a slot's 24 has the bytes in front of the first
     aligned dword, lane q the dword q-1 behind it, or what is left of the range */
  for (uint32_t q = t; q < (ntgt - ncmp) * 24u; q += FD_REEDSOL_BLOCK) {
    const uint32_t e = s.tgt[ncmp + q / 24u], part = q % 24u;
    uint8_t* dst = p.shreds + p.shred_off[first + e];
    const uint32_t H = e < d ? 0x40u : FD_SHRED_CORE_CODE_HDR_SZ;
    const uint32_t a = (uint32_t)(0u - (uint32_t)reinterpret_cast<uintptr_t>(dst)) & 3u;
    const uint32_t lo = part ? a + 4u * (part - 1u) : 0u;
    uint32_t hi = part ? lo + 4u : a;
    if (hi > H) hi = H;
    if (lo >= hi) continue;
    uint32_t v = 0u;
    for (uint32_t b = lo; b < hi; b++) {
      const uint32_t x = b < 64u ? s.sig[b] : fd_reedsol_core_code_hdr_byte(s.ref, depth, d, ntgt, e - d, b - 64u);
      v |= x << (8u * (b - lo));
    }
    if (hi - lo == 4u) *reinterpret_cast<uint32_t*>(dst + lo) = v;   /* part >= 1: dst + lo is dword-aligned */
    else for (uint32_t b = lo; b < hi; b++) dst[b] = (uint8_t)(v >> (8u * (b - lo)));
  }
}

extern "C" int fd_ed25519_hip_launch_fec_recover(const fd_ed25519_fec_recover_params_t* p, void* stream) {
  if (!p->n_set) return 0;
  hipLaunchKernelGGL(fd_ed25519_fec_recover_kernel, dim3((uint32_t)p->n_set), dim3(FD_REEDSOL_BLOCK), 0, (hipStream_t)stream, *p);
  return (int)hipGetLastError();
}
