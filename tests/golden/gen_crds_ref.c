/* gen_crds_ref.c -- asks the reference's own bincode decoders and encoders
   what they make of each packet of tests/golden/crds.npz
   (tests/golden/gen_crds.py builds and runs this in a scratch directory
   against the reference's sources; it is never built by the project's build
   or by a test, and its binary is not kept).

     gen_crds_ref IN OUT

   IN:  u32 count, then per packet u32 size and the bytes, little-endian.
   OUT: per packet u8 decodes -- fd_gossip_msg_decode, as
        fd_gossip_recv_packet calls it, succeeded and consumed every byte --,
        u32 the decoded discriminant (0xffffffff without a decode), u64
        crds_len (of a decoded pull response or push message, else 0); then
        per value of those, in order: u32 the data discriminant, u8 whether
        the bytes fd_crds_data_encode writes for the decoded value (what
        fd_gossip_recv_crds_value hands to fd_ed25519_verify) equal the
        received run -- the bytes fd_crds_value_decode_preflight consumed
        behind the signature --, u32 their size and the bytes. */
#include "flamenco/types/fd_types.h"
#include "util/scratch/fd_scratch.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define SMAX  (1UL<<22)
#define DEPTH (16UL)

static uchar smem[ SMAX ] __attribute__((aligned(FD_SCRATCH_SMEM_ALIGN)));
static ulong fmem[ DEPTH ];

int
main( int argc, char ** argv ) {
  if( argc!=3 ) return 2;
  FILE * in  = fopen( argv[ 1 ], "rb" );
  FILE * out = fopen( argv[ 2 ], "wb" );
  if( !in || !out ) return 2;
  fd_scratch_attach( smem, fmem, SMAX, DEPTH );
  uint n = 0U;
  if( fread( &n, 4, 1, in )!=1 ) return 2;
  for( uint t=0U; t<n; t++ ) {
    uint sz = 0U;
    if( fread( &sz, 4, 1, in )!=1 ) return 2;
    uchar * p = (uchar *)malloc( sz ? sz : 1U );   /* exactly the packet: a decoder that reads past it is caught by a checker */
    if( !p || ( sz && fread( p, 1, sz, in )!=sz ) ) return 2;
    uchar decodes = 0; uint disc = 0xffffffffU; ulong crds_len = 0UL;
    fd_crds_value_t * crds = NULL;
    fd_scratch_push();
    fd_bincode_decode_ctx_t ctx;
    ctx.data    = p;
    ctx.dataend = p + sz;
    ctx.valloc  = fd_scratch_virtual();
    fd_gossip_msg_t gmsg;
    if( !fd_gossip_msg_decode( &gmsg, &ctx ) && ctx.data==ctx.dataend ) {
      decodes = 1; disc = gmsg.discriminant;
      if( fd_gossip_msg_is_pull_resp( &gmsg ) ) { crds_len = gmsg.inner.pull_resp.crds_len; crds = gmsg.inner.pull_resp.crds; }
      if( fd_gossip_msg_is_push_msg ( &gmsg ) ) { crds_len = gmsg.inner.push_msg.crds_len;  crds = gmsg.inner.push_msg.crds;  }
    }
    fwrite( &decodes, 1, 1, out ); fwrite( &disc, 4, 1, out ); fwrite( &crds_len, 8, 1, out );
    /* the received runs: the preflight decoder again, value by value */
    fd_bincode_decode_ctx_t run;
    run.data    = p + 44;
    run.dataend = p + sz;
    run.valloc  = fd_scratch_virtual();
    for( ulong k=0UL; k<crds_len; k++ ) {
      uchar const * start = (uchar const *)run.data;
      if( fd_crds_value_decode_preflight( &run ) ) return 3;
      ulong rsz = (ulong)( (uchar const *)run.data - start ) - 64UL;
      uchar buf[ 1232 ];   /* PACKET_DATA_SIZE, as fd_gossip_recv_crds_value's */
      fd_bincode_encode_ctx_t ectx = { .data = buf, .dataend = buf + sizeof(buf) };
      if( fd_crds_data_encode( &crds[ k ].data, &ectx ) ) return 4;
      uint  esz   = (uint)( (uchar *)ectx.data - buf );
      uchar equal = (uchar)( esz==rsz && !memcmp( buf, start + 64, rsz ) );
      uint  vdisc = crds[ k ].data.discriminant;
      fwrite( &vdisc, 4, 1, out ); fwrite( &equal, 1, 1, out ); fwrite( &esz, 4, 1, out );
      fwrite( buf, 1, esz, out );
    }
    if( crds_len && run.data!=run.dataend ) return 5;
    fd_scratch_pop();
    free( p );
  }
  fclose( in );
  if( fclose( out ) ) return 2;
  return 0;
}
