/* The engine's struct and the helpers that touch it, for the two files that
   are the engine: fd_ed25519_hip_engine.c and fd_ed25519_hip_fronts.c (the
   fronts stage their items in the engine's pinned buffers).  Every other
   client goes through the public API and the accessors of
   fd_ed25519_hip_internal.h and never includes this header. */
#ifndef FD_ED25519_HIP_ENGINE_FIELDS_H
#define FD_ED25519_HIP_ENGINE_FIELDS_H

#include "fd_ed25519_hip_host.h"
#include "../fd_ed25519_hip_internal.h"

#define FD_ED25519_HIP_TIMING_MAX 256

struct fd_ed25519_hip_engine {
  int          device;
  int          flags;
  hipStream_t  stream;
  int          cu_cnt;
  int          dsm_blocks_per_cu;
  uint32_t     dsm_grid;
  uint64_t     quad_max;   /* chunks of at most this many signatures run dsm4 */
  uint64_t     oct_max;    /* ... and of at most this many, dsm8            */
  uint64_t     r16_max;    /* ... and of at most this many, dsm16           */
  uint64_t     max_chunk;
  uint64_t     device_bytes;
  char         arch[ 64 ];
  int          pci[ 3 ];   /* domain, bus, device */

  int32_t *    d_btab;
  int32_t *    d_btab16;     /* [0..2^15]B, the verify kernels' wide B table  */
  int32_t *    btabw[2];    /* shared per device: [0..2^24)B, [0..2^24)[2^144]B */
  int32_t *    btabs[2][8]; /* shared per device: dsm16s<4>'s and <8>'s compact tables, when acquired */
  uint8_t *    d_rstab;     /* the parity and recover kernels' tables (fd_reedsol_core.h) */
  /* Pipeline lanes: the per-chunk scratch of a chunk in flight, and the
     streams its phases run on.  Lane 0 runs on the caller's stream (or the
     engine's); the chunks of a multi-chunk call alternate between lane 0
     and lane 1 (its own streams and scratch, made on the first such call),
     so one chunk's hash / scalar / decode run beside the previous chunk's
     dsm and fill the tail of that persistent kernel (its work items last
     ~1 ms, so its last ~0.46 ms per launch leaves SIMDs idle). */
  struct {
    void *      d_atab;      /* dsm lane tables (and the dsm4 quad tables)  */
    uint8_t *   d_work;      /* one allocation carved into the work arrays */
    uint32_t *  d_k;
    uint8_t *   d_sflag;
    uint8_t *   d_pflag;
    int32_t *   d_pts;
    uint32_t *  d_fix;       /* scalar -> dsm full-length list */
    uint32_t *  d_hs;        /* half-size scalars             */
    uint8_t *   d_hflag;
    uint32_t *  d_perm;      /* hash order (length-sorted) */
    uint32_t *  d_hist;      /* counting-sort scratch      */
    hipStream_t stream;      /* lane 1 only (lane 0: the call's stream)       */
    /* overlap: a large chunk's decode (A and R need neither the hash nor
       the scalars) runs on a side stream beside hash + scalar, dsm after */
    hipStream_t side;
    hipEvent_t  ev_dfork, ev_djoin;
  } lane[ 2 ];
  int          overlap;
  int          pipeline;     /* multi-chunk calls alternate lanes */
  hipEvent_t   ev_start, ev_end;   /* lane 1 after the call's prior work; the call's stream after lane 1 */

  /* host-API staging (pinned host + device mirrors), grown on demand */
  uint64_t     st_sig_cap;   /* signatures */
  uint64_t     st_msg_cap;   /* message bytes */
  uint64_t     st_txn_cap;   /* transactions */
  uint8_t *    h_msgs;  uint8_t *  d_msgs;
  uint64_t *   h_off;   uint64_t * d_off;
  uint32_t *   h_sz;    uint32_t * d_sz;
  uint8_t *    h_sigs;  uint8_t *  d_sigs;
  uint8_t *    h_pubs;  uint8_t *  d_pubs;
  int8_t *     h_out;   int8_t *   d_out;
  uint32_t *   h_tfirst; uint32_t * d_tfirst;
  uint32_t *   h_tcnt;  uint32_t * d_tcnt;
  int8_t *     h_tout;  int8_t *   d_tout;
  /* precompile_host, shreds_host, packets_host: a pass's per-item inputs and
     its outputs in one block each, and the device workspace of the _dev call.
     One set: the wrappers are synchronous on the engine's stream */
  uint64_t     fr_in_cap, fr_out_cap, fr_work_cap;   /* bytes */
  uint8_t *    h_fr_in;  uint8_t *  d_fr_in;
  uint8_t *    h_fr_out; uint8_t *  d_fr_out;
  uint8_t *    d_fr_work;

  /* per-phase event timing (bench / profiling) */
  int          timing;
  int          tm_ev_init;
  int          tm_cnt;
  hipEvent_t   tm_ev[ FD_ED25519_HIP_TIMING_MAX ][ FD_ED25519_PHASE_CNT+1 ];
};

/* verify_dev and verify_digests_dev in one (digests not NULL: msgs unused) */
int fd_ed25519_hip_private_verify_common( fd_ed25519_hip_engine_t * e, unsigned long n,
                                          unsigned char const * msgs, unsigned long const * msg_off,
                                          unsigned int const * msg_sz, unsigned char const * digests,
                                          unsigned char const * sigs, unsigned char const * pubs, signed char * out,
                                          void * stream );
/* a pinned host buffer and its device mirror grown to need elements; the
   message staging (h_msgs, d_msgs) grown to bytes */
int fd_ed25519_hip_private_grow_pair( void ** h, void ** d, uint64_t * cap, uint64_t need, uint64_t elem );
int fd_ed25519_hip_private_stage_msgs( fd_ed25519_hip_engine_t * e, uint64_t bytes );
/* the parity kernel's tables (fd_reedsol_core_tables, in the fronts' file with the other cores): their size, and
   the bytes into tab */
unsigned long fd_ed25519_hip_private_reedsol_tab_bytes( void );
void fd_ed25519_hip_private_reedsol_tables( unsigned char * tab );

#endif
