/* fd_ed25519_hip_pool.c -- the multi-GPU pool and the page-locked-memory
   helpers (include/fd_ed25519_hip_tile.h), over the engine's public API.

   One feeder thread per device, batches dealt round-robin (batch b
   to device b % N, the analogue of seq % verify_tile_count,
   src/app/fdctl/run/tiles/fd_verify.c:46).

   A batch reaches the device without its bytes being touched on the host
   when the caller's arrays are page-locked (fd_ed25519_hip_host_register,
   or hipHostMalloc'd): its messages go as one DMA of the byte range they
   span (the kernels index that range with the caller's own offsets, the
   device base pointer shifted by the range's start), msg_off / msg_sz /
   sigs / pubs as one DMA each, and the codes come back by DMA straight
   into out.  Pageable arrays, or messages scattered so widely that their
   span is far larger than their bytes, are packed into the slot's pinned
   staging block first.  Each slot has its own engine (stream and work
   arrays), so one batch's copies overlap another's kernels; the feeder
   thread runs on the CPUs of its GPU's NUMA node. */

#define _GNU_SOURCE
#include "fd_ed25519_hip_host.h"
#include "../../../include/fd_ed25519_hip_tile.h"

#include <pthread.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
  fd_ed25519_hip_engine_t * eng;
  hipEvent_t                ev;
  hipEvent_t                ev_h2d;    /* this slot's last batch has crossed the link */
  unsigned char *           d_msgs;
  unsigned long *           d_off;
  unsigned int *            d_sz;
  unsigned char *           d_sigs;
  unsigned char *           d_pubs;
  signed char *             d_out;
  unsigned char *           h_stage;   /* pinned: [sigs | pubs | off | sz | msgs], staged batches only (lazy) */
  signed char *             h_out;     /* pinned codes, when out is pageable (lazy)                           */
  unsigned long             i0, i1;
  int                       busy;
} pool_slot_t;

#define POOL_DEV_MAX  64U
#define POOL_SLOT_MAX 8U

struct fd_ed25519_hip_pool {
  unsigned      device_cnt, slot_cnt;
  unsigned long batch_sigs, msg_cap;
  int           device[ POOL_DEV_MAX ];
  pool_slot_t   slot[ POOL_DEV_MAX ][ POOL_SLOT_MAX ];
};

typedef struct {
  fd_ed25519_hip_pool_t * pool;
  unsigned                rank;
  hipEvent_t              h2d_tail;   /* ev_h2d of the batch submitted last on this device (or NULL) */
  unsigned long           n;
  unsigned char const *   msgs;
  unsigned long const *   msg_off;
  unsigned int const *    msg_sz;
  unsigned char const *   sigs;
  unsigned char const *   pubs;
  signed char *           out;
  int                     direct_in, direct_out;   /* caller arrays page-locked */
  int                     err;
  char                    errmsg[ 256 ];   /* the feeder's last_error for err (last_error is per thread) */
  fd_ed25519_hip_pool_stats_t st;
} pool_job_t;

static int
host_locked( void const * p ) {
  if( !p ) return 0;
  hipPointerAttribute_t a;
  memset( &a, 0, sizeof(a) );
  if( hipPointerGetAttributes( &a, p )!=hipSuccess ) { (void)hipGetLastError(); return 0; }
  return a.type==hipMemoryTypeHost;
}

int
fd_ed25519_hip_host_register( void * ptr, unsigned long sz ) {
  if( !ptr || !sz ) return FD_ED25519_HIP_ERR_INVAL;
  HIPCHK( hipHostRegister( ptr, sz, hipHostRegisterPortable | hipHostRegisterMapped ), "hipHostRegister" );
  return FD_ED25519_HIP_OK;
}

int
fd_ed25519_hip_host_unregister( void * ptr ) {
  if( !ptr ) return FD_ED25519_HIP_ERR_INVAL;
  HIPCHK( hipHostUnregister( ptr ), "hipHostUnregister" );
  return FD_ED25519_HIP_OK;
}

void *
fd_ed25519_hip_host_alloc( unsigned long sz ) {
  void * p = NULL;
  hipError_t e = hipHostMalloc( &p, sz ? sz : 1UL, hipHostMallocPortable );
  if( e!=hipSuccess ) { fd_ed25519_hip_private_hip_fail( e, "hipHostMalloc" ); return NULL; }
  return p;
}

void
fd_ed25519_hip_host_free( void * ptr ) {
  if( ptr ) hipHostFree( ptr );
}

/* the calling thread onto the CPUs of the device's NUMA node (within its
   current affinity); no change when that cannot be read */
static void
pin_near_device( int device ) {
  char bdf[ 64 ];
  if( hipDeviceGetPCIBusId( bdf, (int)sizeof(bdf), device )!=hipSuccess ) return;
  for( char * c=bdf; *c; c++ ) if( *c>='A' && *c<='F' ) *c = (char)(*c - 'A' + 'a');
  char path[ 160 ];
  snprintf( path, sizeof(path), "/sys/bus/pci/devices/%s/local_cpulist", bdf );
  FILE * f = fopen( path, "r" );
  if( !f ) return;
  char list[ 1024 ];
  size_t len = fread( list, 1, sizeof(list)-1UL, f );
  fclose( f );
  list[ len ] = 0;
  cpu_set_t cur, want;
  if( pthread_getaffinity_np( pthread_self(), sizeof(cur), &cur ) ) return;
  CPU_ZERO( &want );
  for( char * t=list; *t; ) {
    char * e;
    long lo = strtol( t, &e, 10 ), hi = lo;
    if( e==t ) break;
    if( *e=='-' ) { t = e+1; hi = strtol( t, &e, 10 ); }
    for( long c=lo; c<=hi && c<CPU_SETSIZE; c++ ) if( c>=0 && CPU_ISSET( (int)c, &cur ) ) CPU_SET( (int)c, &want );
    if( *e!=',' ) break;
    t = e+1;
  }
  if( CPU_COUNT( &want ) ) pthread_setaffinity_np( pthread_self(), sizeof(want), &want );
}

/* a batch's message span [lo, hi) and its bytes */
static void
batch_span( pool_job_t const * j, unsigned long i0, unsigned long i1, unsigned long * lo, unsigned long * hi,
            unsigned long * bytes ) {
  unsigned long l = ~0UL, h = 0UL, b = 0UL;
  for( unsigned long i=i0; i<i1; i++ ) {
    unsigned long o = j->msg_off[i], e = o + j->msg_sz[i];
    l = o<l ? o : l;
    h = e>h ? e : h;
    b += j->msg_sz[i];
  }
  if( l>h ) l = h = 0UL;
  *lo = l; *hi = h; *bytes = b;
}

/* the span goes as it is when it fits and is not much larger than the
   bytes in it */
static int
span_direct( fd_ed25519_hip_pool_t const * pl, unsigned long span, unsigned long bytes ) {
  return span<=pl->msg_cap && span<=2UL*bytes + 65536UL;
}

static int
pool_slot_init( pool_slot_t * s, int device, unsigned long batch_sigs, unsigned long msg_cap ) {
  /* one stream per slot: the slots in flight overlap one another, a side
     stream per slot would only crowd the device's hardware queues */
  s->eng = fd_ed25519_hip_engine_new( device, batch_sigs, FD_ED25519_HIP_FLAG_ONE_STREAM );
  if( !s->eng ) return FD_ED25519_HIP_ERR_INVAL;
  unsigned long dsz = 112UL*batch_sigs + msg_cap + 64UL + 1024UL;
  unsigned char * d = NULL;
  HIPCHK( hipMalloc( (void **)&d, dsz ), "hipMalloc(pool slot)" );
  s->d_sigs = d;                                     d += 64UL*batch_sigs;
  s->d_pubs = d;                                     d += 32UL*batch_sigs;
  s->d_off  = (unsigned long *)d;                    d += 8UL*batch_sigs;
  s->d_sz   = (unsigned int *)d;                     d += 4UL*batch_sigs;
  s->d_out  = (signed char *)d;                      d += (batch_sigs + 255UL) & ~255UL;
  s->d_msgs = d;
  HIPCHK( hipEventCreateWithFlags( &s->ev, hipEventDisableTiming ), "hipEventCreate" );
  HIPCHK( hipEventCreateWithFlags( &s->ev_h2d, hipEventDisableTiming ), "hipEventCreate" );
  return FD_ED25519_HIP_OK;
}

static void
pool_slot_fini( pool_slot_t * s ) {
  if( s->eng ) fd_ed25519_hip_engine_sync( s->eng );
  hipFree( s->d_sigs );
  hipHostFree( s->h_stage ); hipHostFree( s->h_out );
  if( s->ev ) hipEventDestroy( s->ev );
  if( s->ev_h2d ) hipEventDestroy( s->ev_h2d );
  if( s->eng ) fd_ed25519_hip_engine_delete( s->eng );
  memset( s, 0, sizeof(*s) );
}

void
fd_ed25519_hip_pool_delete( fd_ed25519_hip_pool_t * pl ) {
  if( !pl ) return;
  for( unsigned r=0U; r<pl->device_cnt; r++ ) {
    hipSetDevice( pl->device[r] );
    for( unsigned k=0U; k<pl->slot_cnt; k++ ) pool_slot_fini( &pl->slot[r][k] );
  }
  free( pl );
}

fd_ed25519_hip_pool_t *
fd_ed25519_hip_pool_new( int const * devices, unsigned device_cnt, unsigned slot_cnt, unsigned long batch_sigs,
                         unsigned long msg_cap ) {
  if( !devices || !device_cnt || device_cnt>POOL_DEV_MAX || slot_cnt<1U || slot_cnt>POOL_SLOT_MAX || !batch_sigs ) {
    fd_ed25519_hip_private_set_error( "pool_new: 1..64 devices, 1..8 slots, batch_sigs > 0" );
    return NULL;
  }
  fd_ed25519_hip_pool_t * pl = (fd_ed25519_hip_pool_t *)calloc( 1, sizeof(*pl) );
  if( !pl ) return NULL;
  pl->device_cnt = device_cnt; pl->slot_cnt = slot_cnt; pl->batch_sigs = batch_sigs;
  pl->msg_cap = msg_cap ? msg_cap : 1UL;
  for( unsigned r=0U; r<device_cnt; r++ ) {
    pl->device[r] = devices[r];
    if( hipSetDevice( devices[r] )!=hipSuccess ) { fd_ed25519_hip_private_hip_fail( hipErrorInvalidDevice, "hipSetDevice" ); goto fail; }
    for( unsigned k=0U; k<slot_cnt; k++ )
      if( pool_slot_init( &pl->slot[r][k], devices[r], batch_sigs, pl->msg_cap ) ) goto fail;
  }
  return pl;
fail:
  fd_ed25519_hip_pool_delete( pl );
  return NULL;
}

static int
pool_enqueue( pool_job_t * j, pool_slot_t * s, unsigned long b ) {
  fd_ed25519_hip_pool_t * pl = j->pool;
  unsigned long i0 = b*pl->batch_sigs, i1 = i0+pl->batch_sigs < j->n ? i0+pl->batch_sigs : j->n, cnt = i1-i0;
  hipStream_t st = (hipStream_t)fd_ed25519_hip_engine_stream( s->eng );
  unsigned long lo, hi, bytes;
  batch_span( j, i0, i1, &lo, &hi, &bytes );
  unsigned char const * dmsgs;
  /* One batch crosses the link at a time: this batch's copies start once
     the previous batch's are done (its kernels still overlap them).  Two
     batches copying at once split the link between two DMA streams and
     move fewer bytes in total than one (the host-fed rate fell to ~46M/s
     with 3 slots, 69M/s with 2, depending on where the slots' streams
     land on the device's hardware queues). */
  if( j->h2d_tail ) HIPCHK( hipStreamWaitEvent( st, j->h2d_tail, 0U ), "hipStreamWaitEvent(h2d)" );
  if( j->direct_in && span_direct( pl, hi-lo, bytes ) ) {
    if( hi>lo ) HIPCHK( hipMemcpyAsync( s->d_msgs, j->msgs + lo, hi-lo, hipMemcpyHostToDevice, st ), "H2D msgs" );
    HIPCHK( hipMemcpyAsync( s->d_off,  j->msg_off + i0, 8UL*cnt,  hipMemcpyHostToDevice, st ), "H2D off"  );
    HIPCHK( hipMemcpyAsync( s->d_sz,   j->msg_sz  + i0, 4UL*cnt,  hipMemcpyHostToDevice, st ), "H2D sz"   );
    HIPCHK( hipMemcpyAsync( s->d_sigs, j->sigs + 64UL*i0, 64UL*cnt, hipMemcpyHostToDevice, st ), "H2D sigs" );
    HIPCHK( hipMemcpyAsync( s->d_pubs, j->pubs + 32UL*i0, 32UL*cnt, hipMemcpyHostToDevice, st ), "H2D pubs" );
    j->st.direct_batches++;
    j->st.h2d_bytes += (hi-lo) + 108UL*cnt;
    dmsgs = s->d_msgs - lo;   /* msg_off[i] indexes the span from its start */
  } else {
    /* pack into pinned staging: [sigs | pubs | off | sz | msgs] */
    if( bytes>pl->msg_cap ) {
      fd_ed25519_hip_private_set_error( "pool: a batch's messages exceed the pool's msg_cap" );
      return FD_ED25519_HIP_ERR_INVAL;
    }
    if( !s->h_stage )
      HIPCHK( hipHostMalloc( (void **)&s->h_stage, 108UL*pl->batch_sigs + pl->msg_cap + 64UL, hipHostMallocDefault ),
            "hipHostMalloc(pool stage)" );
    unsigned char * h = s->h_stage;
    memcpy( h,               j->sigs + 64UL*i0, 64UL*cnt );
    memcpy( h + 64UL*cnt,    j->pubs + 32UL*i0, 32UL*cnt );
    unsigned long * off = (unsigned long *)(h + 96UL*cnt);
    unsigned int *  sz  = (unsigned int  *)(h + 104UL*cnt);
    unsigned char * m   = h + 108UL*cnt;
    unsigned long pos = 0UL;
    for( unsigned long i=i0; i<i1; i++ ) {
      unsigned long k = i-i0;
      if( j->msg_sz[i] ) memcpy( m + pos, j->msgs + j->msg_off[i], j->msg_sz[i] );
      off[k] = pos; sz[k] = j->msg_sz[i];
      pos += j->msg_sz[i];
    }
    HIPCHK( hipMemcpyAsync( s->d_sigs, h,            64UL*cnt, hipMemcpyHostToDevice, st ), "H2D sigs" );
    HIPCHK( hipMemcpyAsync( s->d_pubs, h + 64UL*cnt, 32UL*cnt, hipMemcpyHostToDevice, st ), "H2D pubs" );
    HIPCHK( hipMemcpyAsync( s->d_off,  off,          8UL*cnt,  hipMemcpyHostToDevice, st ), "H2D off"  );
    HIPCHK( hipMemcpyAsync( s->d_sz,   sz,           4UL*cnt,  hipMemcpyHostToDevice, st ), "H2D sz"   );
    if( pos ) HIPCHK( hipMemcpyAsync( s->d_msgs, m, pos, hipMemcpyHostToDevice, st ), "H2D msgs" );
    j->st.staged_batches++;
    j->st.h2d_bytes += pos + 108UL*cnt;
    dmsgs = s->d_msgs;
  }
  HIPCHK( hipEventRecord( s->ev_h2d, st ), "hipEventRecord(h2d)" );
  j->h2d_tail = s->ev_h2d;
#ifdef FD_ED25519_HIP_HOST_FAULT
  /* test build only (tests/test_gpu_pool_fault.py): the second batch's
     launch fails after its copies from the caller's arrays are enqueued */
  if( b==1UL ) {
    fd_ed25519_hip_private_set_error( "pool: injected launch failure (fault-injection build)" );
    return FD_ED25519_HIP_ERR_HIP - (int)hipErrorLaunchFailure;
  }
#endif
  int err = fd_ed25519_hip_verify_dev( s->eng, cnt, dmsgs, s->d_off, s->d_sz, s->d_sigs, s->d_pubs, s->d_out, st );
  if( err ) return err;
  if( !j->direct_out && !s->h_out )
    HIPCHK( hipHostMalloc( (void **)&s->h_out, pl->batch_sigs, hipHostMallocDefault ), "hipHostMalloc(pool out)" );
  signed char * dst = j->direct_out ? j->out + i0 : s->h_out;
  HIPCHK( hipMemcpyAsync( dst, s->d_out, cnt, hipMemcpyDeviceToHost, st ), "D2H codes" );
  HIPCHK( hipEventRecord( s->ev, st ), "hipEventRecord" );
  s->i0 = i0; s->i1 = i1; s->busy = 1;
  return FD_ED25519_HIP_OK;
}

/* A batch whose enqueue failed part way may have left copies from or into
   the caller's page-locked arrays on the slot's stream: they finish before
   the error is reported, so pool_run never returns while DMA may still
   touch memory the caller is free to release. */
static int
pool_submit( pool_job_t * j, pool_slot_t * s, unsigned long b ) {
  int err = pool_enqueue( j, s, b );
  if( err ) hipStreamSynchronize( (hipStream_t)fd_ed25519_hip_engine_stream( s->eng ) );
  return err;
}

static void *
pool_main( void * arg ) {
  pool_job_t * j = (pool_job_t *)arg;
  fd_ed25519_hip_pool_t * pl = j->pool;
  int dev = pl->device[ j->rank ];
  pin_near_device( dev );
  if( hipSetDevice( dev )!=hipSuccess ) {
    j->err = fd_ed25519_hip_private_hip_fail( hipErrorInvalidDevice, "hipSetDevice" );
    snprintf( j->errmsg, sizeof(j->errmsg), "%s", fd_ed25519_hip_last_error() );
    return NULL;
  }
  pool_slot_t * slot = pl->slot[ j->rank ];
  unsigned sc = pl->slot_cnt, ranks = pl->device_cnt;
  unsigned long nb = (j->n + pl->batch_sigs - 1UL) / pl->batch_sigs;
  unsigned long b_sub = j->rank, b_done = j->rank;
  unsigned next = 0U, oldest = 0U;
  while( b_done<nb ) {
    pool_slot_t * s = &slot[ next ];
    if( !j->err && b_sub<nb && !s->busy ) {
      int err = pool_submit( j, s, b_sub );
      if( err ) {   /* drain what is in flight */
        j->err = err;
        snprintf( j->errmsg, sizeof(j->errmsg), "%s", fd_ed25519_hip_last_error() );
        continue;
      }
      b_sub += ranks;
      next = (next+1U) % sc;
      continue;
    }
    pool_slot_t * d = &slot[ oldest ];
    if( !d->busy ) break;   /* an error stopped submission and everything drained */
    hipError_t e = hipEventSynchronize( d->ev );
    if( e!=hipSuccess && !j->err ) {
      j->err = fd_ed25519_hip_private_hip_fail( e, "pool batch" );
      snprintf( j->errmsg, sizeof(j->errmsg), "%s", fd_ed25519_hip_last_error() );
    }
    if( !j->direct_out && e==hipSuccess ) memcpy( j->out + d->i0, d->h_out, d->i1 - d->i0 );
    d->busy = 0;
    oldest = (oldest+1U) % sc;
    b_done += ranks;
  }
  return NULL;
}

int
fd_ed25519_hip_pool_run( fd_ed25519_hip_pool_t * pl, unsigned long n, unsigned char const * msgs,
                         unsigned long const * msg_off, unsigned int const * msg_sz, unsigned char const * sigs,
                         unsigned char const * pubs, signed char * out, double * seconds,
                         fd_ed25519_hip_pool_stats_t * stats ) {
  if( !pl || !out ) return FD_ED25519_HIP_ERR_INVAL;
  if( n && (!msg_off || !msg_sz || !sigs || !pubs || !msgs) ) return FD_ED25519_HIP_ERR_INVAL;
  pool_job_t job[ POOL_DEV_MAX ];
  pthread_t  th[ POOL_DEV_MAX ];
  int direct_in  = n && host_locked( msgs ) && host_locked( msg_off ) && host_locked( msg_sz ) &&
                   host_locked( sigs ) && host_locked( pubs );
  int direct_out = n && host_locked( out );
  double t0 = now_s();
  unsigned started = 0U;
  int err = 0;
  for( unsigned r=0U; r<pl->device_cnt; r++ ) {
    memset( &job[r], 0, sizeof(job[r]) );
    job[r].pool = pl; job[r].rank = r; job[r].n = n; job[r].msgs = msgs; job[r].msg_off = msg_off;
    job[r].msg_sz = msg_sz; job[r].sigs = sigs; job[r].pubs = pubs; job[r].out = out;
    job[r].direct_in = direct_in; job[r].direct_out = direct_out;
    if( pthread_create( &th[r], NULL, pool_main, &job[r] ) ) { err = FD_ED25519_HIP_ERR_NOMEM; break; }
    started++;
  }
  if( stats ) memset( stats, 0, sizeof(*stats) );
  for( unsigned r=0U; r<started; r++ ) {
    pthread_join( th[r], NULL );
    if( job[r].err && !err ) { err = job[r].err; fd_ed25519_hip_private_set_error( job[r].errmsg ); }
    if( stats ) {
      stats->direct_batches += job[r].st.direct_batches;
      stats->staged_batches += job[r].st.staged_batches;
      stats->h2d_bytes      += job[r].st.h2d_bytes;
    }
  }
  if( seconds ) *seconds = now_s() - t0;
  return err;
}

int
fd_ed25519_hip_pool_verify( int const * devices, unsigned device_cnt, unsigned slot_cnt, unsigned long batch_sigs,
                            unsigned long n, unsigned char const * msgs, unsigned long const * msg_off,
                            unsigned int const * msg_sz, unsigned char const * sigs, unsigned char const * pubs,
                            signed char * out, double * seconds ) {
  if( !batch_sigs ) return FD_ED25519_HIP_ERR_INVAL;
  /* capacity: the largest span of a batch */
  unsigned long cap = 1UL;
  pool_job_t tmp;
  memset( &tmp, 0, sizeof(tmp) );
  tmp.msg_off = msg_off; tmp.msg_sz = msg_sz;
  for( unsigned long i0=0UL; n && msg_off && msg_sz && i0<n; i0+=batch_sigs ) {
    unsigned long lo, hi, bytes;
    batch_span( &tmp, i0, i0+batch_sigs<n ? i0+batch_sigs : n, &lo, &hi, &bytes );
    unsigned long need = hi-lo<=2UL*bytes + 65536UL ? hi-lo : bytes;
    if( need>cap ) cap = need;
  }
  fd_ed25519_hip_pool_t * pl = fd_ed25519_hip_pool_new( devices, device_cnt, slot_cnt, batch_sigs, cap );
  if( !pl ) return FD_ED25519_HIP_ERR_INVAL;
  double t0 = now_s();
  int err = fd_ed25519_hip_pool_run( pl, n, msgs, msg_off, msg_sz, sigs, pubs, out, NULL, NULL );
  fd_ed25519_hip_pool_delete( pl );
  if( seconds ) *seconds = now_s() - t0;
  return err;
}

double
fd_ed25519_hip_h2d_gbps( int device, unsigned long bytes, unsigned reps ) {
  if( !bytes || !reps || hipSetDevice( device )!=hipSuccess ) return 0.0;
  void * h = NULL, * d = NULL;
  hipStream_t st = NULL;
  double r = 0.0;
  if( hipHostMalloc( &h, bytes, hipHostMallocDefault )==hipSuccess && hipMalloc( &d, bytes )==hipSuccess &&
      hipStreamCreateWithFlags( &st, hipStreamNonBlocking )==hipSuccess ) {
    memset( h, 0x5a, bytes );
    int ok = hipMemcpyAsync( d, h, bytes, hipMemcpyHostToDevice, st )==hipSuccess &&
             hipStreamSynchronize( st )==hipSuccess;   /* warm-up */
    double t0 = now_s();
    for( unsigned i=0U; ok && i<reps; i++ ) ok = hipMemcpyAsync( d, h, bytes, hipMemcpyHostToDevice, st )==hipSuccess;
    ok = ok && hipStreamSynchronize( st )==hipSuccess;
    double dt = now_s() - t0;
    if( ok && dt>0.0 ) r = (double)bytes * reps / dt * 1e-9;
  }
  if( st ) hipStreamDestroy( st );
  hipFree( d ); hipHostFree( h );
  return r;
}
