/* shred_walk_main.c -- the shred rules, the leaf hash and the walk of the
   inclusion proof (fd_shred_core.h) as a stand-alone program for hostile
   input (tests/test_shred_hostile.py builds it with
   -fsanitize=address,undefined).  Reads a file of shreds (u32 count, then
   u32 size and the bytes of each, little-endian), runs fd_shred_core_root on
   a heap copy of exactly the shred's size -- a read one byte past it is a
   sanitizer report -- and prints per shred
     code root
   (the root in hex, or - when none is derived) as the library's
   fd_ed25519_hip_shred_root reports them. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fd_shred_core.h"

int
main( int argc, char ** argv ) {
  if( argc!=2 ) return 2;
  FILE * f = fopen( argv[ 1 ], "rb" );
  if( !f ) return 2;
  unsigned n = 0U;
  if( fread( &n, 4, 1, f )!=1 ) return 2;
  for( unsigned t=0U; t<n; t++ ) {
    unsigned sz = 0U;
    if( fread( &sz, 4, 1, f )!=1 ) return 2;
    unsigned char * p = (unsigned char *)malloc( sz ? sz : 1U );
    if( !p || ( sz && fread( p, 1, sz, f )!=sz ) ) return 2;
    if( !sz ) { free( p ); p = (unsigned char *)malloc( 1 ); }   /* a shred of no bytes: nothing may be read */
    unsigned char root[ 32 ];
    memset( root, 0xA5, 32 );
    int code = fd_shred_core_root( p, sz, root );
    printf( "%d ", code );
    if( code ) {
      for( int i=0; i<32; i++ ) if( root[ i ]!=0xA5 ) return 3;   /* untouched without a root */
      printf( "-\n" );
    } else {
      for( int i=0; i<32; i++ ) printf( "%02x", root[ i ] );
      printf( "\n" );
    }
    free( p );
  }
  fclose( f );
  return 0;
}
