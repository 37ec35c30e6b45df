/* poh_walk_main.c -- the proof-of-history rules and the block walk
   (fd_poh_core.h) as a stand-alone program for hostile input
   (tests/test_poh_hostile.py builds it with -fsanitize=address,undefined).

     poh_walk IN OUT

   Reads a file of cases (u32 count; per case a u8 kind), little-endian:

     kind 0, a raw block: u64 hash_cnt_max, 32 bytes of in state, u32 size,
       the block.  The in state and the block stand together in one heap
       block of exactly 32 + size bytes -- a read one byte outside it is a
       sanitizer report --, the walk runs once for the counts and once into
       arrays of exactly those counts, and every microblock is verified.
       Out: i32 the walk's code, u32 n, then per microblock i8 code and the
       32-byte state.
     kind 1, descriptors: u64 hash_cnt_max, u32 size and the buffer, u32 n,
       hdr_off u64 [n], in_off u64 [n], sig_first u32 [n+1], u32 n_sig,
       sig_off u64 [n_sig], each array in a heap block of its own.  Out: per
       microblock i8 code and the 32-byte state. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fd_ed25519_hip_tile.h"   /* fd_ed25519_hip_txn_t, for the parse core */
#include "fd_txn_parse_core.h"
#include "fd_shred_core.h"
#include "fd_poh_core.h"

#define RD( p, sz ) do { size_t sz_ = (size_t)(sz); if( sz_!=0 && fread( (p), 1, sz_, f )!=sz_ ) return 2; } while(0)

static void *
exact( size_t bytes ) {
  void * p = malloc( bytes ? bytes : 1 );
  if( !p ) exit( 2 );
  return p;
}

int
main( int argc, char ** argv ) {
  if( argc!=3 ) return 2;
  FILE * f   = fopen( argv[ 1 ], "rb" );
  FILE * out = fopen( argv[ 2 ], "wb" );
  if( !f || !out ) return 2;
  unsigned cases = 0U;
  RD( &cases, 4 );
  for( unsigned c=0U; c<cases; c++ ) {
    unsigned char kind;
    unsigned long hash_cnt_max;
    unsigned size;
    RD( &kind, 1 ); RD( &hash_cnt_max, 8 );
    if( kind==0 ) {
      unsigned char in_state[ 32 ];
      RD( in_state, 32 ); RD( &size, 4 );
      unsigned char * buf = (unsigned char *)exact( 32UL + size );
      memcpy( buf, in_state, 32 );
      RD( buf + 32, size );
      unsigned long n = 0UL, n_sig = 0UL, n2, s2;
      int code = fd_poh_core_walk( buf + 32, size, 32UL, 0UL, NULL, NULL, NULL, 0UL, NULL, 0UL, &n, &n_sig );
      unsigned n32 = code ? 0U : (unsigned)n;
      fwrite( &code, 4, 1, out ); fwrite( &n32, 4, 1, out );
      if( !code ) {
        unsigned long * hdr_off   = (unsigned long *)exact( n*8UL );
        unsigned long * in_off    = (unsigned long *)exact( n*8UL );
        unsigned int *  sig_first = (unsigned int *) exact( ( n+1UL )*4UL );
        unsigned long * sig_off   = (unsigned long *)exact( n_sig*8UL );
        if( fd_poh_core_walk( buf + 32, size, 32UL, 0UL, hdr_off, in_off, sig_first, n, sig_off, n_sig, &n2, &s2 ) ) return 3;
        if( n2!=n || s2!=n_sig || sig_first[ n ]!=n_sig ) return 3;
        for( unsigned long i=0UL; i<n; i++ ) {
          unsigned char state[ 32 ];
          signed char v = (signed char)fd_poh_core_verify( buf, 32UL + size, hdr_off[ i ], in_off[ i ], sig_first[ i ],
                                                           sig_first[ i+1UL ], n_sig, sig_off, hash_cnt_max, state );
          fwrite( &v, 1, 1, out ); fwrite( state, 1, 32, out );
        }
        free( hdr_off ); free( in_off ); free( sig_first ); free( sig_off );
      }
      free( buf );
    } else if( kind==1 ) {
      unsigned n, n_sig;
      RD( &size, 4 );
      unsigned char * buf = (unsigned char *)exact( size );
      RD( buf, size );
      RD( &n, 4 );
      unsigned long * hdr_off   = (unsigned long *)exact( n*8UL );
      unsigned long * in_off    = (unsigned long *)exact( n*8UL );
      unsigned int *  sig_first = (unsigned int *) exact( ( n+1UL )*4UL );
      RD( hdr_off, n*8UL ); RD( in_off, n*8UL ); RD( sig_first, ( n+1UL )*4UL );
      RD( &n_sig, 4 );
      unsigned long * sig_off = (unsigned long *)exact( n_sig*8UL );
      RD( sig_off, n_sig*8UL );
      for( unsigned i=0U; i<n; i++ ) {
        unsigned char state[ 32 ];
        signed char v = (signed char)fd_poh_core_verify( buf, size, hdr_off[ i ], in_off[ i ], sig_first[ i ], sig_first[ i+1U ],
                                                         n_sig, sig_off, hash_cnt_max, state );
        fwrite( &v, 1, 1, out ); fwrite( state, 1, 32, out );
      }
      free( buf ); free( hdr_off ); free( in_off ); free( sig_first ); free( sig_off );
    } else return 2;
  }
  fclose( f );
  if( fclose( out ) ) return 2;
  return 0;
}
