/* gen_packets_ref.c -- asks the reference's own bincode decoders what they
   make of each packet of tests/golden/packets.npz (tests/golden/gen_packets.py
   builds and runs this in a scratch directory against the reference's
   sources; it is never built by the project's build or by a test, and its
   binary is not kept).

     gen_packets_ref IN OUT

   IN:  u32 count, then per packet u8 proto (0 gossip, 1 repair serve), u32
        size and the bytes, little-endian.
   OUT: per packet u8 decodes -- fd_gossip_msg_decode (proto 0, as
        fd_gossip_recv_packet calls it) or fd_repair_protocol_decode (proto
        1, as fd_repair_recv_serv_packet does) succeeded and consumed every
        byte --, u32 the decoded discriminant (0xffffffff without a decode),
        u32 size and the bytes of fd_gossip_prune_sign_data_encode over the
        fields fd_gossip_handle_prune copies (size 0 for anything but a
        decoded gossip prune). */
#include "flamenco/types/fd_types.h"
#include "util/scratch/fd_scratch.h"
#include <stdio.h>
#include <stdlib.h>

#define SMAX  (1UL<<20)
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
    uchar proto = 0; uint sz = 0U;
    if( fread( &proto, 1, 1, in )!=1 || fread( &sz, 4, 1, in )!=1 ) return 2;
    uchar * p = (uchar *)malloc( sz ? sz : 1U );   /* exactly the packet: a decoder that reads past it is caught by a checker */
    if( !p || ( sz && fread( p, 1, sz, in )!=sz ) ) return 2;
    uchar decodes = 0; uint disc = 0xffffffffU; uint ssz = 0U;
    uchar sign[ 2048 ];
    fd_scratch_push();
    fd_bincode_decode_ctx_t ctx;
    ctx.data    = p;
    ctx.dataend = p + sz;
    ctx.valloc  = fd_scratch_virtual();
    if( proto==0 ) {
      fd_gossip_msg_t gmsg;
      if( !fd_gossip_msg_decode( &gmsg, &ctx ) && ctx.data==ctx.dataend ) {
        decodes = 1; disc = gmsg.discriminant;
        if( fd_gossip_msg_is_prune_msg( &gmsg ) ) {
          fd_gossip_prune_data_t const * d = &gmsg.inner.prune_msg.data;
          fd_gossip_prune_sign_data_t sd = { .pubkey = d->pubkey, .prunes_len = d->prunes_len, .prunes = d->prunes,
                                             .destination = d->destination, .wallclock = d->wallclock };
          fd_bincode_encode_ctx_t ectx = { .data = sign, .dataend = sign + sizeof(sign) };
          if( fd_gossip_prune_sign_data_encode( &sd, &ectx ) ) return 3;
          ssz = (uint)( (uchar *)ectx.data - sign );
        }
      }
    } else {
      fd_repair_protocol_t protocol;
      if( !fd_repair_protocol_decode( &protocol, &ctx ) && ctx.data==ctx.dataend ) {
        decodes = 1; disc = protocol.discriminant;
      }
    }
    fd_scratch_pop();
    fwrite( &decodes, 1, 1, out ); fwrite( &disc, 4, 1, out ); fwrite( &ssz, 4, 1, out );
    if( ssz ) fwrite( sign, 1, ssz, out );
    free( p );
  }
  fclose( in );
  if( fclose( out ) ) return 2;
  return 0;
}
