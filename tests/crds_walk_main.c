/* crds_walk_main.c -- the CRDS rules (fd_crds_core.h, with the prefix form of
   the transaction parser it calls) as a stand-alone program for hostile
   input (tests/test_crds_hostile.py builds it with
   -fsanitize=address,undefined).  Reads a file of packets (u32 count, then
   per packet the 32-byte own identity it is judged under, u32 size and the
   bytes, little-endian), runs fd_crds_core_walk and fd_crds_core_value on a
   heap copy of exactly the packet's size -- a read one byte past it is a
   sanitizer report --, reads every byte the values name, and prints per
   packet
     code count
   and per value
     disc pre sig_off key_off msg_off msg_sz
   as the library's fd_ed25519_hip_crds_plan reports them. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fd_ed25519_hip_tile.h"   /* fd_ed25519_hip_txn_t, for the parse core */
#include "fd_txn_parse_core.h"
#include "fd_crds_core.h"

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
    unsigned sz = 0U;
    if( fread( self, 1, 32, f )!=32 || fread( &sz, 4, 1, f )!=1 ) return 2;
    unsigned char * p = (unsigned char *)malloc( sz ? sz : 1U );   /* a packet of no bytes: nothing may be read */
    if( !p || ( sz && fread( p, 1, sz, f )!=sz ) ) return 2;
    fd_crds_core_idx_t idx;
    memset( &idx, 0xA5, sizeof(idx) );
    int code = fd_crds_core_walk( p, sz, &idx );
    if( code && idx.cnt ) return 3;                                /* no values without a decoded packet */
    if( idx.cnt>FD_CRDS_CORE_VAL_MAX ) return 3;
    printf( "%d %u\n", code, idx.cnt );
    for( unsigned k=0U; k<idx.cnt; k++ ) {                         /* every planned byte lies in the block */
      fd_crds_core_val_t v;
      memset( &v, 0xA5, sizeof(v) );
      fd_crds_core_value( p, sz, &idx, k, self, &v );
      touched += sum( p, v.sig_off, 64U ) + sum( p, v.key_off, 32U ) + sum( p, v.msg_off, v.msg_sz );
      printf( "%u %d %u %u %u %u\n", v.disc, (int)v.pre, (unsigned)v.sig_off, (unsigned)v.key_off, (unsigned)v.msg_off,
              (unsigned)v.msg_sz );
    }
    free( p );
  }
  fclose( f );
  fprintf( stderr, "%u packets, byte sum %u\n", n, touched );
  return 0;
}
