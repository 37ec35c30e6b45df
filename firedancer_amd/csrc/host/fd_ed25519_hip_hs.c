/* fd_ed25519_hip_hs.c -- one host-scalar launch (fd_ed25519_hip_internal.h):
   the block the calling thread fills and dsm16 / dsm16s read in place, the
   order of its launches and writes, and the host's copy of
   batch_single_msg's combine rule.  The drop-in (fd_ed25519_hip_dropin.c
   dropin_launch_hs) and the verify tile's pipe (fd_ed25519_hip_tile.c
   pipe_submit_hs) each walk their own inputs through it.

   The order that must hold: the launch that waits goes before any host
   arithmetic, the go word is zeroed before that launch, and every write of
   the block comes before the release store of the go word.  A launch begun
   ends in hs_end on every path, or the kernel spins to its bound
   (FD_ED25519_GO_SPIN_MAX). */
#include "../fd_ed25519_hip_internal.h"
#include "../../../include/fd_ed25519_hip.h"

_Static_assert( sizeof(fd_ed25519_hip_hs_t)<=FD_ED25519_HS_DESC_MAX, "FD_ED25519_HS_DESC_MAX" );

unsigned long
fd_ed25519_hip_private_hs_bytes( unsigned long stride, int decode ) {
  return decode ? FD_ED25519_HS_O_GO( stride ) + 16UL : FD_ED25519_HS_O_HS( stride ) + 19UL*4UL*stride;
}

void
fd_ed25519_hip_private_hs_init( fd_ed25519_hip_hs_t * b, void * host, unsigned long stride, int decode, unsigned long n,
                                int split, int avx_rule ) {
  *b = (fd_ed25519_hip_hs_t){ .host = (unsigned char *)host, .stride = stride, .decode = decode, .n = n,
                              .split = decode ? split : 0, .avx_rule = avx_rule };
}

int
fd_ed25519_hip_private_hs_begin( fd_ed25519_hip_hs_t * b, struct fd_ed25519_hip_engine * e, unsigned char const * dev,
                                 unsigned char const * sigs, unsigned char const * pubs, signed char * out,
                                 void * stream ) {
  b->eng = e; b->dev = dev; b->sigs = sigs; b->pubs = pubs; b->out = out; b->stream = stream;
  if( !b->decode ) return fd_ed25519_hip_private_hs_launch( b, 0 );
  if( b->n>FD_ED25519_HS_DECODE_MAX ) return FD_ED25519_HIP_ERR_INVAL;
  *(volatile uint32_t *)( b->host + FD_ED25519_HS_O_GO( b->stride ) ) = 0U;
  return fd_ed25519_hip_private_hs_launch( b, 1 );
}

int
fd_ed25519_hip_private_hs_scalars( fd_ed25519_hip_hs_t * b, unsigned long j, unsigned char const sig[ 64 ],
                                   unsigned char const pub[ 32 ], unsigned char const * msg, unsigned long msg_sz,
                                   int dbits ) {
  uint32_t rec[ 32 ];
  if( !fd_ed25519_hip_private_hsrec( sig, pub, msg, msg_sz, dbits, rec ) ) return 0;
  uint32_t * hs = (uint32_t *)( b->host + FD_ED25519_HS_O_HS( b->stride ) );
  if( b->split ) fd_ed25519_hip_private_hssplit( rec, b->split, hs, b->stride, j );
  else for( unsigned long w=0UL; w<19UL; w++ ) hs[ w*b->stride + j ] = rec[ 8UL + w ];
  b->host[ FD_ED25519_HS_O_SFLAG( b->stride ) + j ] = (unsigned char)rec[ 27 ];
  b->host[ FD_ED25519_HS_O_HFLAG( b->stride ) + j ] = (unsigned char)rec[ 28 ];
  return 1;
}

void
fd_ed25519_hip_private_hs_points( fd_ed25519_hip_hs_t * b, unsigned char const * const * enc ) {
  if( !b->decode || b->n>FD_ED25519_HS_DECODE_MAX ) return;
  int32_t       pt[ 2UL*FD_ED25519_HS_DECODE_MAX ][ 20 ], ptx[ 2UL*FD_ED25519_HS_DECODE_MAX*3UL ][ 40 ];
  unsigned char fl[ 2UL*FD_ED25519_HS_DECODE_MAX ];
  int split = b->split, nx = split ? split/2 - 1 : 0, step = split==4 ? 66 : 33;
  fd_ed25519_hip_private_hsdec3_n( enc, 2UL*b->n, b->avx_rule, &pt[0][0], split ? &ptx[0][0] : NULL, nx, step, fl );
  unsigned long   sc  = b->stride;
  int32_t *       pts = (int32_t *)( b->host + FD_ED25519_HS_O_PTS( sc ) );
  unsigned char * pfl = b->host + FD_ED25519_HS_O_PFLAG( sc );
  unsigned long   rs  = split ? 40UL : 20UL;   /* the row stride in limbs: dsm16s's, dsm16's */
  for( unsigned long j=0UL; j<b->n; j++ )
    for( unsigned long side=0UL; side<2UL; side++ ) {   /* rows 2m + side: A, R, A_1, R_1, .. */
      unsigned long pi = 2UL*j + side;
      for( unsigned long l=0UL; l<20UL; l++ ) pts[ ( side*rs + l )*sc + j ] = pt[ pi ][ l ];
      for( int m=1; m<=nx; m++ )
        for( unsigned long l=0UL; l<40UL; l++ )
          pts[ ( ( 2UL*(unsigned long)m + side )*40UL + l )*sc + j ] = ptx[ pi*(unsigned long)nx + (unsigned long)(m-1) ][ l ];
      pfl[ side*sc + j ] = fl[ pi ];
    }
}

int
fd_ed25519_hip_private_hs_end( fd_ed25519_hip_hs_t * b, int run ) {
  if( b->decode ) {
    __atomic_store_n( (uint32_t *)( b->host + FD_ED25519_HS_O_GO( b->stride ) ),
                      run ? FD_ED25519_GO_RUN : FD_ED25519_GO_CANCEL, __ATOMIC_RELEASE );
    return FD_ED25519_HIP_OK;
  }
  return run ? fd_ed25519_hip_private_hs_launch( b, 1 ) : FD_ED25519_HIP_OK;
}

int
fd_ed25519_hip_private_hs_combine( signed char const * codes, unsigned long first, unsigned long cnt ) {
  if( cnt==0UL || cnt>16UL ) return FD_ED25519_ERR_SIG;
  int msg_fail = 0;
  for( unsigned long j=0UL; j<cnt; j++ ) {
    int c = codes[ first + j ];
    if( c==FD_ED25519_ERR_MSG ) msg_fail = 1;
    else if( c!=FD_ED25519_SUCCESS ) return c;
  }
  return msg_fail ? FD_ED25519_ERR_MSG : FD_ED25519_SUCCESS;
}
