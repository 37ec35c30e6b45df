/* packet_walk_main.c -- the gossip and repair packet rules
   (fd_packet_core.h) as a stand-alone program for hostile input
   (tests/test_packet_hostile.py builds it with
   -fsanitize=address,undefined).  Reads a file of packets (u32 count, then
   per packet the 32-byte own identity it is judged under, u8 protocol, u32
   size and the bytes, little-endian), runs fd_packet_core_plan on a heap
   copy of exactly the packet's size -- a read one byte past it is a
   sanitizer report --, reads every byte the plan names, and prints per
   packet
     code disc key_off sig_off msg0_off msg0_sz msg1_off msg1_sz
   as the library's fd_ed25519_hip_packet_plan reports them. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fd_packet_core.h"

static unsigned
sum( unsigned char const * p, unsigned off, unsigned sz ) {
  unsigned s = 0U;
  for( unsigned i=0U; i<sz; i++ ) s += p[ off+i ];
  return s;
}

int
main( int argc, char ** argv ) {
  if( argc!=2 ) return 2;
  FILE * f = fopen( argv[ 1 ], "rb" );
  if( !f ) return 2;
  unsigned n = 0U;
  unsigned char self[ 32 ];
  if( fread( &n, 4, 1, f )!=1 ) return 2;
  unsigned touched = 0U;
  for( unsigned t=0U; t<n; t++ ) {
    unsigned char proto = 0; unsigned sz = 0U;
    if( fread( self, 1, 32, f )!=32 || fread( &proto, 1, 1, f )!=1 || fread( &sz, 4, 1, f )!=1 ) return 2;
    unsigned char * p = (unsigned char *)malloc( sz ? sz : 1U );   /* a packet of no bytes: nothing may be read */
    if( !p || ( sz && fread( p, 1, sz, f )!=sz ) ) return 2;
    fd_packet_core_plan_t pl;
    memset( &pl, 0xA5, sizeof(pl) );
    int code = fd_packet_core_plan( proto, p, sz, self, &pl );
    if( code ) {   /* no plan without a judged packet */
      if( pl.key_off | pl.sig_off | pl.msg0_off | pl.msg0_sz | pl.msg1_off | pl.msg1_sz ) return 3;
    } else {       /* every planned byte lies in the block */
      touched += sum( p, pl.key_off, 32U ) + sum( p, pl.sig_off, 64U ) + sum( p, pl.msg0_off, pl.msg0_sz ) +
                 sum( p, pl.msg1_off, pl.msg1_sz );
    }
    printf( "%d %u %u %u %u %u %u %u\n", code, pl.disc, (unsigned)pl.key_off, (unsigned)pl.sig_off, (unsigned)pl.msg0_off,
            (unsigned)pl.msg0_sz, (unsigned)pl.msg1_off, (unsigned)pl.msg1_sz );
    free( p );
  }
  fclose( f );
  fprintf( stderr, "%u packets, byte sum %u\n", n, touched );
  return 0;
}
