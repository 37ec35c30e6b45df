/* fd_ed25519_hip_dropin.c -- the drop-in fd_ed25519_verify /
   fd_ed25519_verify_batch_single_msg / fd_ed25519_strerror symbols, on
   lazily created process-wide engines.  A client of the engine as the pipe
   is (fd_ed25519_hip_tile.c): the public API and the accessors of
   fd_ed25519_hip_internal.h, never the engine's struct.

   fd_ed25519_verify / fd_ed25519_verify_batch_single_msg for any number of
   calling threads (the reference's are reentrant and keep no global state,
   src/ballet/ed25519/fd_ed25519.h:86-94).  Concurrent calls are coalesced
   by flat combining: each call queues a request; a caller that finds one
   of the process's DROPIN_ENGINES drop-in engines idle takes every queued
   request (its own and the others', up to DROPIN_BATCH_MAX) into one
   launch -- each request one transaction of 1..16 signatures over its
   message, with batch_single_msg's combine -- and hands every caller its
   code; the others wait on a condition variable.  One caller alone pays
   one GPU round trip as before; N concurrent callers share a round trip,
   and four engines keep batches filling while others are on the GPU, so
   calls per second grow with the caller count instead of serialising on
   one lock.  The engines use the compact base tables
   (FD_ED25519_HIP_FLAG_COMPACT_TABLES: 2 x 8 MiB instead of 2 x 2 GiB) and
   small chunks, so a process that only uses the drop-ins holds well under
   600 MB of device memory. */

#define _GNU_SOURCE
#include "fd_ed25519_hip_host.h"
#include "../fd_ed25519_hip_internal.h"
#include "../fd_dropin_block.h"

#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define DROPIN_ENGINES   4
#define DROPIN_BATCH_MAX 4096UL
#define DROPIN_CHUNK     16384UL
#define DROPIN_PENDING 0x55   /* a direct launch's codes before the kernels write them */
#ifndef DROPIN_DIRECT_MAX
#define DROPIN_DIRECT_MAX 64UL   /* launches of at most this many signatures read the pinned block in place */
#endif
/* ... and of at most this many input bytes: the hash kernels read a direct
   launch's messages word by word over the link from uncached coherent
   pinned memory, which pays for a few hundred bytes but not for a
   multi-MB message (one bulk pull into HBM first is faster there). */
#ifndef DROPIN_DIRECT_MAX_BYTES
#define DROPIN_DIRECT_MAX_BYTES 65536UL
#endif

typedef struct dropin_req {
  unsigned char const * msg;
  unsigned long         msg_sz;
  unsigned char const * sigs;
  unsigned char const * pubs;
  unsigned int          cnt;      /* signatures, 1..16                     */
  int                   single;   /* fd_ed25519_verify: the signature's code */
  int                   hashed;   /* dig holds SHA-512(R_j||A_j||M): the message stays on the host */
  int                   result;
  int                   done;
  struct dropin_req *   next;
  unsigned char         dig[ 16 ][ 64 ];
} dropin_req_t;

/* Messages of at least this many bytes are hashed on the host by the
   calling thread (fd_ed25519_hip_private_challenge) and verified from their
   digests: the device hash takes sizes up to FD_ED25519_HIP_MSG_SZ_MAX
   (2^31 - 1: its remaining-byte counts are signed 32-bit values), and the
   reference takes any ulong size (src/ballet/ed25519/fd_ed25519.h:96-101).
   A test hook moves the limit down (fd_ed25519_hip_dropin_set_host_hash_min). */
#define DROPIN_HOST_HASH_MIN_MAX ((unsigned long)FD_ED25519_HIP_MSG_SZ_MAX + 1UL)
static unsigned long dropin_host_hash_min = DROPIN_HOST_HASH_MIN_MAX;

/* clamped to 2 GiB: a limit above that would leave messages the device
   hash cannot carry on the device path */
void
fd_ed25519_hip_dropin_set_host_hash_min( unsigned long bytes ) {
  dropin_host_hash_min = ( bytes && bytes<DROPIN_HOST_HASH_MIN_MAX ) ? bytes : DROPIN_HOST_HASH_MIN_MAX;
}

void fd_ed25519_hip_private_challenge( unsigned char const sig[ 64 ], unsigned char const pub[ 32 ],
                                       unsigned char const * msg, unsigned long msg_sz, unsigned char out[ 64 ] );

/* Direct launches of at most this many signatures take their scalars from
   the calling thread (host/fd_ed25519_hip_hsrec.cc, ~8 us each) while the
   device decompresses A and R, instead of prep16's hash -> search chain of
   one lane; more would cost the caller more than the chain.  Test hook:
   fd_ed25519_hip_dropin_set_host_scalars (0 turns the mode off). */
#ifndef DROPIN_HS_MAX
#define DROPIN_HS_MAX 4UL
#endif
static unsigned long dropin_hs_max = DROPIN_HS_MAX;
#define FD_HALF_DBITS_HOST_MAX 151   /* fd25519_half.h FD_HALF_DBITS_MAX */

void
fd_ed25519_hip_dropin_set_host_scalars( unsigned long max_sigs ) {
  dropin_hs_max = max_sigs>DROPIN_DIRECT_MAX ? DROPIN_DIRECT_MAX : max_sigs;
}

/* Test hook: the host search's bound on |d| (0: the engine's, 151).  No
   random k without a pair at 151 bits turned up in 40M trials, so tests
   reach the launch's fallback (the device path from the digests, at the
   engine's bound) with k that have no pair at 131 bits
   (tests/golden/halfsize.npz). */
static int dropin_hs_dbits;

void
fd_ed25519_hip_dropin_set_host_scalars_dbits( int dbits ) {
  dropin_hs_dbits = dbits>0 && dbits<=FD_HALF_DBITS_HOST_MAX ? dbits : 0;
}

/* Launches of at most this many host-scalar signatures also decompress A
   and R on the calling thread (host/fd_ed25519_hip_hsdec.cc; both points
   of a signature side by side, ~9 us a signature on one core) and launch
   dsm16 alone: the host's scalars plus decompressions then cost less than
   the decode blocks' ~44 us they replace.  At four signatures (~70 us of
   host work) they would not.  Test hook: fd_ed25519_hip_dropin_set_host_decode. */
#ifndef DROPIN_HD_MAX
#define DROPIN_HD_MAX 2UL
#endif
static unsigned long dropin_hd_max = DROPIN_HD_MAX;

/* host-decoded drop-in launches take the split form of this many waves
   (dsm16s: 4 or 8, the host doubling A and R and splitting the scalars;
   2: dsm16) when the engine holds its tables: p50 82.3 / 68.8 / 76.2 us
   with 2 / 4 / 8 for one caller, back to back on one box -- eight waves
   halve the chain again but pay more host doublings, eight table builds
   and three rounds of additions (profiles/r6_dropin_split_waves.json);
   test / A-B hook fd_ed25519_hip_dropin_set_split_waves */
#ifndef DROPIN_SPLIT_WAVES
#define DROPIN_SPLIT_WAVES 4
#endif
static int dropin_split = DROPIN_SPLIT_WAVES;

void
fd_ed25519_hip_dropin_set_split_waves( int waves ) {
  dropin_split = waves==4 || waves==8 ? waves : 2;
}

void
fd_ed25519_hip_dropin_set_host_decode( unsigned long max_sigs ) {
  dropin_hd_max = max_sigs>FD_ED25519_HS_DECODE_MAX ? FD_ED25519_HS_DECODE_MAX : max_sigs;
}

static pthread_once_t  dropin_once = PTHREAD_ONCE_INIT;
static pthread_mutex_t dropin_lock = PTHREAD_MUTEX_INITIALIZER;
static pthread_cond_t  dropin_cv   = PTHREAD_COND_INITIALIZER;
static struct {
  fd_ed25519_hip_engine_t * eng[ DROPIN_ENGINES ];
  int                       eng_device[ DROPIN_ENGINES ];   /* fd_ed25519_hip_engine_info's, read once at creation */
  uint64_t                  eng_chunk[ DROPIN_ENGINES ];    /* ... its max_chunk: the work arrays' stride */
  int                       busy[ DROPIN_ENGINES ];
  unsigned char *           h_blk[ DROPIN_ENGINES ];   /* pinned, coherent: one launch's inputs, then its codes */
  unsigned char *           h_dev[ DROPIN_ENGINES ];   /* h_blk as the device sees it */
  unsigned char *           d_blk[ DROPIN_ENGINES ];
  uint64_t                  blk_cap[ DROPIN_ENGINES ];
  int                       direct_pending[ DROPIN_ENGINES ];   /* last launch returned before its stream ended */
  dropin_req_t *            head;
  dropin_req_t *            tail;
  unsigned long             launches, requests;   /* for fd_ed25519_hip_dropin_stats */
  int                       device, flags;        /* what the engines are made with */
  /* failure policy (fd_ed25519_hip_dropin_set_on_lost), under dropin_lock */
  int                       on_lost;
  int                       lost;                 /* 0, or the code that lost the device */
  unsigned long             recoveries;
} dq;

/* the message, then abort(): the ABORT policy's end */
static void
dropin_fatal( int err, char const * what ) {
  fprintf( stderr, "libfd_ed25519_hip: FATAL: %s: %s (%d): %s; the device is lost to the drop-ins (policy: abort)\n",
           what, fd_ed25519_hip_strerror( err ), err, fd_ed25519_hip_last_error() );
  abort();
}

/* engine k anew (its staging block too): any previous one is deleted
   first.  0 or the creation's error code (dq.eng[k] then NULL). */
static int
dropin_engine_make( int k ) {
  if( dq.eng[k] ) { fd_ed25519_hip_engine_delete( dq.eng[k] ); dq.eng[k] = NULL; }
  hipHostFree( dq.h_blk[k] ); hipFree( dq.d_blk[k] );
  dq.h_blk[k] = NULL; dq.h_dev[k] = NULL; dq.d_blk[k] = NULL; dq.blk_cap[k] = 0UL;
  dq.direct_pending[k] = 0;
  dq.eng[k] = fd_ed25519_hip_engine_new( dq.device, DROPIN_CHUNK, dq.flags );
  if( !dq.eng[k] ) return FD_ED25519_HIP_ERR_INVAL;
  fd_ed25519_hip_info_t info;
  fd_ed25519_hip_engine_info( dq.eng[k], &info );
  dq.eng_device[k] = info.device; dq.eng_chunk[k] = info.max_chunk;
  if( dropin_split>2 ) fd_ed25519_hip_private_want_dsms( dq.eng[k], dropin_split );   /* without: dsm16 */
  return FD_ED25519_HIP_OK;
}

/* every engine, each with one more attempt if its first creation fails */
static int
dropin_engines_make( void ) {
  for( int k=0; k<DROPIN_ENGINES; k++ ) {
    int err = dropin_engine_make( k );
    if( err ) err = dropin_engine_make( k );
    if( err ) return err;
  }
  return FD_ED25519_HIP_OK;
}

static void
dropin_init( void ) {
  char const * dev_s   = getenv( "FD_ED25519_HIP_DEVICE" );
  char const * codes_s = getenv( "FD_ED25519_HIP_CODES" );
  dq.device = dev_s ? atoi( dev_s ) : 0;
  dq.flags  = FD_ED25519_HIP_FLAG_COMPACT_TABLES | FD_ED25519_HIP_FLAG_ONE_STREAM |
              ((codes_s && !strcmp( codes_s, "portable" )) ? FD_ED25519_HIP_FLAG_CODES_PORTABLE : 0);
  int err = dropin_engines_make();
  if( err ) {
    pthread_mutex_lock( &dropin_lock );
    dq.lost = err;
    int abort_now = dq.on_lost==FD_ED25519_HIP_DROPIN_ON_LOST_ABORT;
    pthread_mutex_unlock( &dropin_lock );
    if( abort_now ) dropin_fatal( err, "cannot create the drop-in GPU engines" );
    fprintf( stderr, "libfd_ed25519_hip: cannot create the drop-in GPU engines: %s; every drop-in call returns "
                     "FD_ED25519_ERR_SIG (policy: reject) until fd_ed25519_hip_dropin_reset\n",
             fd_ed25519_hip_last_error() );
  }
}

int
fd_ed25519_hip_dropin_set_on_lost( int policy ) {
  if( policy!=FD_ED25519_HIP_DROPIN_ON_LOST_ABORT && policy!=FD_ED25519_HIP_DROPIN_ON_LOST_REJECT )
    return FD_ED25519_HIP_ERR_INVAL;
  pthread_mutex_lock( &dropin_lock );
  int prev = dq.on_lost;
  dq.on_lost = policy;
  pthread_mutex_unlock( &dropin_lock );
  return prev;
}

int
fd_ed25519_hip_dropin_status( unsigned long * recoveries ) {
  pthread_mutex_lock( &dropin_lock );
  int lost = dq.lost;
  if( recoveries ) *recoveries = dq.recoveries;
  pthread_mutex_unlock( &dropin_lock );
  return lost;
}

/* One combined launch of the requests in list (n of them) on drop-in
   engine k, step by step (dropin_run).  The launch moves one pinned block
   each way (fd_dropin_block.h).  The per-transaction combine
   (batch_single_msg's priority rule) runs only when a request has more
   than one signature; a lone signature's code is its request's result. */
typedef struct {
  int                       k;
  fd_ed25519_hip_engine_t * e;
  hipStream_t               st;
  dropin_req_t *            list;
  uint64_t                  n;                       /* requests */
  uint64_t                  nsig, nsig_h;            /* signatures; those of requests hashed on the host */
  int                       multi;                   /* a request has more than one signature */
  int                       hsmode, hdmode, split;   /* host scalars; host decode too; dsm16s's waves or 0 */
  uint64_t                  cap_hs;                  /* the host-scalar block's stride */
  int                       direct;                  /* the kernels read and write the pinned block in place */
  fd_dropin_block_t         b;
  unsigned char *           h;                       /* the pinned block */
  unsigned char *           d;                       /* its device copy */
  unsigned char *           src;                     /* what the kernels use: h as the device sees it (direct), or d */
} dropin_launch_t;

#ifdef FD_ED25519_HIP_HOST_FAULT
/* test build only (tests/test_gpu_dropin_fault.py): with
   $FD_ED25519_HIP_FAULT_DROPIN = "a:b", drop-in launches a .. a+b-1 (counted
   from 1 over the process, retries included) fail as a launch failure
   would, after their inputs are staged */
static int
dropin_fault( void ) {
  static unsigned long cnt;
  char const * f = getenv( "FD_ED25519_HIP_FAULT_DROPIN" );
  unsigned long i = __atomic_add_fetch( &cnt, 1UL, __ATOMIC_RELAXED );
  if( !f || !*f ) return 0;
  char * e;
  unsigned long a = strtoul( f, &e, 10 ), b = *e==':' ? strtoul( e+1, NULL, 10 ) : 1UL;
  return i>=a && i<a+b;
}
#endif

/* A direct launch returned when its codes landed, before its stream's
   completion signal (dropin_wait): an error raised after that (a wave
   faulting on its way out) surfaces here, before this launch restages the
   block.  It is reported as the earlier launch's, and this launch then
   runs on a re-created engine (dropin_retry). */
static int
dropin_pending_query( int k, hipStream_t st ) {
  if( !dq.direct_pending[k] ) return FD_ED25519_HIP_OK;
  dq.direct_pending[k] = 0;
  hipError_t q = hipStreamQuery( st );
  if( q==hipSuccess || q==hipErrorNotReady ) return FD_ED25519_HIP_OK;
  fd_ed25519_hip_private_set_errorf( "drop-in: engine %d's previous direct launch ended with %s after its codes landed", k,
                                     hipGetErrorString( q ) );
  return FD_ED25519_HIP_ERR_HIP - (int)q;
}

/* the signatures counted, which fixes the launch's mode, and the block laid out */
static void
dropin_plan( dropin_launch_t * L ) {
  /* signatures of requests hashed on the host go after the others: the
     device hashes [0, nsig_m), takes digests for [nsig_m, nsig) */
  uint64_t bytes = 0UL;
  for( dropin_req_t * r=L->list; r; r=r->next ) {
    L->nsig += r->cnt; L->multi |= r->cnt>1U;
    if( r->hashed ) L->nsig_h += r->cnt; else bytes += r->msg_sz;
  }
  /* host scalars (a launch of a few signatures -- fd_ed25519_verify calls,
     or batch_single_msg transactions of a few signatures, whose codes are
     then combined on the host -- any message size below the host-hash
     limit): the calling thread hashes and finds
     the scalars, the device reads sflag / hflag [cap] and hs [19][cap] in
     the block (the work arrays' stride, the first nsig of each row
     written) and never the messages, which are not staged; a signature
     without a half-size pair (~1e-6) takes the device path from its
     digest (room for nsig digests) */
  L->hsmode = L->nsig<=dropin_hs_max && !L->nsig_h;
  L->hdmode = L->hsmode && L->nsig<=dropin_hd_max;
  /* the host arrays' stride: the work arrays' when the device decodes
     (its pts / pflag), a small one when every array is the caller's */
  L->cap_hs = L->hdmode ? FD_ED25519_HS_STRIDE : dq.eng_chunk[ L->k ];
  L->split  = L->hdmode && dropin_split>2 && fd_ed25519_hip_private_want_dsms( L->e, dropin_split ) ? dropin_split : 0;
  fd_dropin_block( L->n, L->nsig, L->nsig_h, bytes, L->hsmode,
                   L->hsmode ? fd_ed25519_hip_private_hs_bytes( L->cap_hs, L->hdmode ) : 0UL, &L->b );
}

/* engine k's block (pinned, and its device copy) of at least need bytes */
static int
dropin_room( int k, uint64_t need, hipStream_t st ) {
  if( need<=dq.blk_cap[k] ) return FD_ED25519_HIP_OK;
  uint64_t cap = dq.blk_cap[k] ? dq.blk_cap[k] : (1UL<<20);
  while( cap<need ) cap *= 2UL;
  hipStreamSynchronize( st );   /* a direct launch may still be ending (dropin_wait) */
  hipHostFree( dq.h_blk[k] ); hipFree( dq.d_blk[k] );
  dq.h_blk[k] = NULL; dq.h_dev[k] = NULL; dq.d_blk[k] = NULL; dq.blk_cap[k] = 0UL;
  HIPCHK( hipHostMalloc( (void **)&dq.h_blk[k], cap, hipHostMallocCoherent ), "hipHostMalloc(drop-in)" );
  HIPCHK( hipHostGetDevicePointer( (void **)&dq.h_dev[k], dq.h_blk[k], 0U ), "hipHostGetDevicePointer(drop-in)" );
  HIPCHK( hipMalloc( (void **)&dq.d_blk[k], cap ), "hipMalloc(drop-in)" );
  dq.blk_cap[k] = cap;
  return FD_ED25519_HIP_OK;
}

/* the requests into the pinned block */
static void
dropin_stage( dropin_launch_t * L ) {
  fd_dropin_block_t const * b = &L->b;
  unsigned char * h   = L->h;
  unsigned long * off = (unsigned long *)(h + b->o_off);
  unsigned int *  sz  = (unsigned int  *)(h + b->o_sz);
  uint32_t *      tf  = (uint32_t      *)(h + b->o_tf);
  uint32_t *      tc  = (uint32_t      *)(h + b->o_tc);
  uint64_t nsig_m = L->nsig - L->nsig_h, pos = 0UL, j = 0UL, jh = nsig_m, t = 0UL;
  for( dropin_req_t * r=L->list; r; r=r->next, t++ ) {
    uint64_t s0 = r->hashed ? jh : j;
    tf[t] = (uint32_t)s0;
    tc[t] = r->cnt;
    memcpy( h + b->o_sig + 64UL*s0, r->sigs, 64UL*r->cnt );
    memcpy( h + b->o_pub + 32UL*s0, r->pubs, 32UL*r->cnt );
    int      staged = !r->hashed && !L->hsmode;   /* else the device never reads the message */
    uint64_t msg_sz = staged ? r->msg_sz : 0UL;
    if( r->hashed ) memcpy( h + b->o_dig + 64UL*(s0 - nsig_m), r->dig, 64UL*r->cnt );
    if( msg_sz ) memcpy( h + b->o_msg + pos, r->msg, msg_sz );
    for( uint32_t i=0U; i<r->cnt; i++ ) { off[s0+i] = staged ? pos : 0UL; sz[s0+i] = (unsigned int)msg_sz; }
    pos += msg_sz;
    if( r->hashed ) jh += r->cnt; else j += r->cnt;
  }
}

/* The host-scalar launch: the device's decompressions now and the group
   equation after the scalars this thread computes meanwhile -- or, for the
   fewest signatures, the group equation launched first, waiting, and this
   thread's scalars and decompressions while it is dispatched (a signature
   without a half-size pair, ~1e-6, sends the launch down the device's own
   path instead) */
static int
dropin_launch_hs( dropin_launch_t * L ) {
  fd_dropin_block_t const * b = &L->b;
  unsigned char * h = L->h, * src = L->src;
  uint32_t const * tf = (uint32_t const *)(h + b->o_tf);
  fd_ed25519_hip_hs_t hb;
  fd_ed25519_hip_private_hs_init( &hb, h + b->o_hsb, L->cap_hs, L->hdmode, L->nsig, L->split,
                                  !fd_ed25519_hip_private_codes_portable( L->e ) );
  int err = fd_ed25519_hip_private_hs_begin( &hb, L->e, src + b->o_hsb, src + b->o_sig, src + b->o_pub,
                                             (signed char *)(src + b->o_out), L->st );
  if( err ) return err;
  int all = 1;
  int dbits = dropin_hs_dbits ? dropin_hs_dbits : fd_ed25519_hip_private_half_dbits( L->e );
  /* signature j (the requests' signatures in order): A at enc[2j], R at enc[2j+1] */
  unsigned char const * enc[ 2UL*FD_ED25519_HS_DECODE_MAX ];
  uint64_t t = 0UL;
  for( dropin_req_t * r=L->list; r && all; r=r->next, t++ ) {
    for( uint32_t i=0U; i<r->cnt && all; i++ ) {   /* a batch_single_msg request: its signatures over one message */
      uint64_t j = tf[ t ] + i;
      all = fd_ed25519_hip_private_hs_scalars( &hb, j, r->sigs + 64UL*i, r->pubs + 32UL*i, r->msg, r->msg_sz, dbits );
      if( L->hdmode ) { enc[ 2UL*j ] = r->pubs + 32UL*i; enc[ 2UL*j + 1UL ] = r->sigs + 64UL*i; }
    }
  }
  if( all && L->hdmode ) fd_ed25519_hip_private_hs_points( &hb, enc );
  err = fd_ed25519_hip_private_hs_end( &hb, all );
  if( err || all ) return err;
  /* the device path from the digests (the messages were not staged) */
  t = 0UL;
  for( dropin_req_t * r=L->list; r; r=r->next, t++ )
    for( uint32_t i=0U; i<r->cnt; i++ )
      fd_ed25519_hip_private_challenge( r->sigs + 64UL*i, r->pubs + 32UL*i, r->msg, r->msg_sz,
                                        h + b->o_dig + 64UL*( tf[ t ] + i ) );
  return fd_ed25519_hip_verify_digests_dev( L->e, L->nsig, src + b->o_dig, src + b->o_sig, src + b->o_pub,
                                            (signed char *)(src + b->o_out), L->st );
}

/* Everything the launch queues on the stream.  Not 0: a launch failed, and
   dropin_run drains what was queued before it.

   A launch of a few signatures (one caller alone, the latency case) has
   the kernels read its inputs and write its codes through the pinned
   block's device-visible address: no copy launches, two kernels fewer on
   the call's path (the hash's first loads wait on the link instead, a
   few hundred bytes).  A larger combined launch moves the block by
   device launches (fd_ed25519_hip_launch_pull), not copy-engine calls:
   several drop-in engines submit from their callers' threads at once
   (DESIGN.md 3c), and one bulk read beats every lane reading over the
   link. */
static int
dropin_launch( dropin_launch_t * L ) {
  fd_dropin_block_t const * b = &L->b;
  fd_ed25519_hip_engine_t * e = L->e;
  hipStream_t st = L->st;
  uint64_t nsig = L->nsig, nsig_m = nsig - L->nsig_h;
  unsigned char * d = L->d, * h_dev = dq.h_dev[ L->k ];
  L->direct = L->hsmode || ( nsig<=DROPIN_DIRECT_MAX && !L->multi && b->in_sz<=DROPIN_DIRECT_MAX_BYTES );
  unsigned char * src = L->src = L->direct ? h_dev : d;
  if( L->direct ) memset( L->h + b->o_out, DROPIN_PENDING, nsig );   /* no code is this value */
  fd_ed25519_pull_params_t pp;
  memset( &pp, 0, sizeof(pp) );
  if( !L->direct ) {   /* pull in */
    pp.src[0] = h_dev; pp.dst[0] = d; pp.n[0] = b->in_sz ? b->in_sz : 1UL; pp.cnt = 1U;
    HIPCHK( (hipError_t)fd_ed25519_hip_launch_pull( &pp, st ), "H2D drop-in" );
  }
  int err;
  if( L->hsmode ) err = dropin_launch_hs( L );   /* a direct launch, none of its requests hashed on the host */
  else err = fd_ed25519_hip_verify_dev( e, nsig_m, src + b->o_msg, (unsigned long const *)(src + b->o_off),
                                        (unsigned int const *)(src + b->o_sz), src + b->o_sig, src + b->o_pub,
                                        (signed char *)(src + b->o_out), st );
  if( !err && L->nsig_h )
    err = fd_ed25519_hip_verify_digests_dev( e, L->nsig_h, src + b->o_dig, src + b->o_sig + 64UL*nsig_m,
                                             src + b->o_pub + 32UL*nsig_m, (signed char *)(src + b->o_out + nsig_m), st );
  if( !err && L->multi && !L->direct )   /* (a direct multi-signature launch is a host-scalar one: combined in dropin_results) */
    err = fd_ed25519_hip_txn_combine_dev( e, L->n, (signed char const *)(d + b->o_out), (uint32_t const *)(d + b->o_tf),
                                          (uint32_t const *)(d + b->o_tc), (signed char *)(d + b->o_tout), st );
  if( err ) return err;
  if( !L->direct ) {   /* pull out */
    pp.src[0] = d + b->o_out; pp.dst[0] = h_dev + b->o_out; pp.n[0] = L->multi ? nsig + L->n : nsig;
    HIPCHK( (hipError_t)fd_ed25519_hip_launch_pull( &pp, st ), "D2H drop-in" );
  }
  return FD_ED25519_HIP_OK;
}

/* until the codes are in the pinned block */
static int
dropin_wait( dropin_launch_t * L ) {
  if( !L->direct ) {
    HIPCHK( hipStreamSynchronize( L->st ), "drop-in verify" );
    return FD_ED25519_HIP_OK;
  }
  /* The codes land in the pinned block as the kernels write them: the
     call returns when all are there, without waiting for the stream's
     completion signal (the kernels read nothing of this block after
     writing a code, and the engine's next launch is ordered behind
     them on its stream).  The stream is queried every 64 polls, so a
     failed launch still ends the wait with its error. */
  uint64_t nsig = L->nsig;
  volatile signed char const * c = (volatile signed char const *)(L->h + L->b.o_out);
  for( unsigned long spin=1UL;; spin++ ) {
    unsigned long i = 0UL;
    while( i<nsig && c[ i ]!=(signed char)DROPIN_PENDING ) i++;
    if( i==nsig ) break;
    if( !(spin & 63UL) ) {
      hipError_t q = hipStreamQuery( L->st );
      if( q==hipErrorNotReady ) continue;
      HIPCHK( q, "drop-in verify" );
      /* the stream is done: every code must be there */
      for( i=0UL; i<nsig && c[ i ]!=(signed char)DROPIN_PENDING; i++ ) ;
      if( i<nsig ) {
        fd_ed25519_hip_private_set_error( "drop-in: a launch ended without a code" );
        return FD_ED25519_HIP_ERR_HIP - (int)hipErrorLaunchFailure;
      }
      break;
    }
    __builtin_ia32_pause();
  }
  dq.direct_pending[ L->k ] = 1;
  return FD_ED25519_HIP_OK;
}

/* every request's code out of the block */
static void
dropin_results( dropin_launch_t * L ) {
  unsigned char * h = L->h;
  uint32_t const *    tf    = (uint32_t const *)(h + L->b.o_tf);
  signed char const * codes = (signed char const *)(h + L->b.o_out);
  signed char *       tcode = (signed char *)(h + L->b.o_tout);
  uint64_t t = 0UL;
  if( L->multi && L->direct ) {
    /* batch_single_msg's rule per request (1..16 signatures: the guard ran
       before submit) */
    for( dropin_req_t * r=L->list; r; r=r->next, t++ )
      tcode[ t ] = (signed char)fd_ed25519_hip_private_hs_combine( codes, tf[ t ], r->cnt );
  }
  t = 0UL;
  for( dropin_req_t * r=L->list; r; r=r->next, t++ )
    r->result = (r->single || !L->multi) ? (int)codes[ tf[t] ] : (int)tcode[t];
}

static int
dropin_run( int k, dropin_req_t * list, unsigned long n ) {
  dropin_launch_t L = { .k = k, .e = dq.eng[k], .list = list, .n = n };
  if( !L.e ) {
    fd_ed25519_hip_private_set_errorf( "drop-in engine %d was not created", k );
    return FD_ED25519_HIP_ERR_INVAL;
  }
  HIPCHK( hipSetDevice( dq.eng_device[k] ), "hipSetDevice" );
  L.st = (hipStream_t)fd_ed25519_hip_engine_stream( L.e );
  int err = dropin_pending_query( k, L.st );
  if( err ) return err;
  dropin_plan( &L );
  if( (err = dropin_room( k, L.b.need, L.st )) ) return err;
  L.h = dq.h_blk[k]; L.d = dq.d_blk[k];
  dropin_stage( &L );
#ifdef FD_ED25519_HIP_HOST_FAULT
  if( dropin_fault() ) {
    fd_ed25519_hip_private_set_error( "drop-in: injected launch failure (fault-injection build)" );
    return FD_ED25519_HIP_ERR_HIP - (int)hipErrorLaunchFailure;
  }
#endif
  if( (err = dropin_launch( &L )) ) {
    hipStreamSynchronize( L.st );   /* the one exit of a failed launch: what it did queue has drained */
    return err;
  }
  if( (err = dropin_wait( &L )) ) return err;
  dropin_results( &L );
  return FD_ED25519_HIP_OK;
}

/* a failed launch on engine k: the engine is made anew and the launch run
   once more (outside the lock, engine k is this thread's while busy) */
static int
dropin_retry( int k, dropin_req_t * list, unsigned long n, int err ) {
  fprintf( stderr, "libfd_ed25519_hip: drop-in launch failed: %s (%d): %s; re-creating engine %d and retrying once\n",
           fd_ed25519_hip_strerror( err ), err, fd_ed25519_hip_last_error(), k );
  int e2 = dropin_engine_make( k );
  if( !e2 ) e2 = dropin_run( k, list, n );
  return e2;
}

/* the device is lost (under dropin_lock): the ABORT policy ends here; the
   REJECT one fails every queued request closed */
static void
dropin_lose( int err ) {
  if( !dq.lost ) dq.lost = err;
  if( dq.on_lost==FD_ED25519_HIP_DROPIN_ON_LOST_ABORT ) dropin_fatal( err, "GPU verify failed twice (after a retry)" );
  for( dropin_req_t * q=dq.head; q; ) { dropin_req_t * nx = q->next; q->result = FD_ED25519_ERR_SIG; q->done = 1; q = nx; }
  dq.head = dq.tail = NULL;
}

static int
dropin_submit( dropin_req_t * r ) {
  pthread_once( &dropin_once, dropin_init );
  r->done = 0; r->next = NULL;
  pthread_mutex_lock( &dropin_lock );
  if( dq.lost ) {   /* fail closed (REJECT; ABORT never gets here) */
    pthread_mutex_unlock( &dropin_lock );
    return FD_ED25519_ERR_SIG;
  }
  if( dq.tail ) dq.tail->next = r; else dq.head = r;
  dq.tail = r;
  while( !r->done ) {
    int k = -1;
    for( int i=0; i<DROPIN_ENGINES; i++ ) if( !dq.busy[i] ) { k = i; break; }
    if( k<0 || !dq.head ) { pthread_cond_wait( &dropin_cv, &dropin_lock ); continue; }
    /* combine: take up to DROPIN_BATCH_MAX queued requests onto engine k */
    dropin_req_t * list = dq.head, * last = dq.head;
    unsigned long n = 1UL;
    while( last->next && n<DROPIN_BATCH_MAX ) { last = last->next; n++; }
    dq.head = last->next;
    if( !dq.head ) dq.tail = NULL;
    last->next = NULL;
    dq.busy[k] = 1;
    dq.launches++; dq.requests += n;
    pthread_mutex_unlock( &dropin_lock );
    int err = dropin_run( k, list, n ), retried = 0;
    if( err ) { err = dropin_retry( k, list, n, err ); retried = 1; }
    pthread_mutex_lock( &dropin_lock );
    if( err ) {
      for( dropin_req_t * q=list; q; q=q->next ) q->result = FD_ED25519_ERR_SIG;
      dropin_lose( err );
    } else if( retried ) {
      dq.recoveries++;
    }
    for( dropin_req_t * q=list; q; ) { dropin_req_t * nx = q->next; q->done = 1; q = nx; }
    dq.busy[k] = 0;
    pthread_cond_broadcast( &dropin_cv );
  }
  pthread_mutex_unlock( &dropin_lock );
  return r->result;
}

void
fd_ed25519_hip_dropin_stats( unsigned long * launches, unsigned long * requests ) {
  pthread_mutex_lock( &dropin_lock );
  if( launches ) *launches = dq.launches;
  if( requests ) *requests = dq.requests;
  pthread_mutex_unlock( &dropin_lock );
}

unsigned long
fd_ed25519_hip_dropin_device_bytes( void ) {
  pthread_once( &dropin_once, dropin_init );
  unsigned long b = 0UL;
  fd_ed25519_hip_info_t info;
  for( int k=0; k<DROPIN_ENGINES; k++ )
    if( !fd_ed25519_hip_engine_info( dq.eng[k], &info ) ) b += info.device_bytes + dq.blk_cap[k];
  return b + fd_ed25519_hip_shared_device_bytes( dq.device );
}

int
fd_ed25519_hip_dropin_reset( void ) {
  pthread_once( &dropin_once, dropin_init );
  pthread_mutex_lock( &dropin_lock );
  /* every engine idle, then held: no launch starts while they are re-made */
  for( ;; ) {
    int any = 0;
    for( int k=0; k<DROPIN_ENGINES; k++ ) any |= dq.busy[k];
    if( !any ) break;
    pthread_cond_wait( &dropin_cv, &dropin_lock );
  }
  for( int k=0; k<DROPIN_ENGINES; k++ ) dq.busy[k] = 1;
  pthread_mutex_unlock( &dropin_lock );
  int err = dropin_engines_make();
  pthread_mutex_lock( &dropin_lock );
  if( !err ) dq.lost = 0;
  else if( !dq.lost ) dq.lost = err;
  for( int k=0; k<DROPIN_ENGINES; k++ ) dq.busy[k] = 0;
  pthread_cond_broadcast( &dropin_cv );
  pthread_mutex_unlock( &dropin_lock );
  return err;
}

/* The device hash takes message sizes below 2^31; the reference
   takes any ulong size.  A message of dropin_host_hash_min bytes or more
   (2 GiB: the first size the device hash cannot carry) is hashed here, in the
   calling thread, with the library's own SHA-512 (one digest of R_j||A_j||M
   per signature), before the request is queued; everything after the hash
   -- the reduction mod L, decompression, the group equation, the batch
   priority rule -- runs on the GPU as for any other request.  The message
   is never truncated. */
static void
dropin_prepare( dropin_req_t * r ) {
  /* the second test is the guard whatever the limit says: a size the
     device hash cannot carry is never sent there */
  r->hashed = r->msg_sz>=dropin_host_hash_min || r->msg_sz>(unsigned long)FD_ED25519_HIP_MSG_SZ_MAX;
  if( !r->hashed ) return;
  for( unsigned int j=0U; j<r->cnt; j++ )
    fd_ed25519_hip_private_challenge( r->sigs + 64UL*j, r->pubs + 32UL*j, r->msg, r->msg_sz, r->dig[ j ] );
}

int
fd_ed25519_verify( unsigned char const msg[], unsigned long msg_sz, unsigned char const sig[ 64 ],
                   unsigned char const public_key[ 32 ], fd_sha512_t * sha ) {
  (void)sha;
  dropin_req_t r;
  r.msg = msg; r.msg_sz = msg_sz; r.sigs = sig; r.pubs = public_key; r.cnt = 1U; r.single = 1;
  dropin_prepare( &r );
  return dropin_submit( &r );
}

int
fd_ed25519_verify_batch_single_msg( unsigned char const msg[], unsigned long const msg_sz,
                                    unsigned char const signatures[ 64 ], unsigned char const pubkeys[ 32 ],
                                    fd_sha512_t * shas[ 1 ], unsigned char const batch_sz ) {
  (void)shas;
  if( batch_sz==0 || batch_sz>16 ) return FD_ED25519_ERR_SIG;
  dropin_req_t r;
  r.msg = msg; r.msg_sz = msg_sz; r.sigs = signatures; r.pubs = pubkeys; r.cnt = batch_sz;
  r.single = 0;
  dropin_prepare( &r );
  return dropin_submit( &r );
}

char const *
fd_ed25519_strerror( int err ) {
  switch( err ) {
  case FD_ED25519_SUCCESS:    return "success";
  case FD_ED25519_ERR_SIG:    return "bad signature";
  case FD_ED25519_ERR_PUBKEY: return "bad public key";
  case FD_ED25519_ERR_MSG:    return "bad message";
  default: break;
  }
  return "unknown";
}
