/* shredder_walk_main.c -- the shredder's counts, plan, header writers and
   batch judgement (fd_shredder_core.h) as a stand-alone program for hostile
   input (tests/test_shredder_hostile.py builds it with
   -fsanitize=address,undefined).

     shredder_walk IN OUT

   IN:  u32 batches; per batch the 24-byte descriptor, u32 sz and the sz
        bytes; then u32 judgements; per judgement nine u64: off, sz, buf_sz,
        s0, s1, n_set, h0, h1, n.  Little-endian.
   OUT: per batch i32 code and, for code 0, u32 sets, data shreds, parity
        shreds, set_first[sets+1] and every shred, 1203 or 1228 bytes; per
        judgement i32.

   fd_shredder_core_batch runs with the batch in a heap block of exactly sz
   bytes and every shred in a heap block of exactly its size, filled with
   0xA5 -- a read or a write one byte outside is a sanitizer report, and the
   parity regions come back as 0xA5. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fd_shredder_core.h"

int
main( int argc, char ** argv ) {
  if( argc!=3 ) return 2;
  FILE * f   = fopen( argv[ 1 ], "rb" );
  FILE * out = fopen( argv[ 2 ], "wb" );
  if( !f || !out ) return 2;
  unsigned nb = 0U;
  if( fread( &nb, 4, 1, f )!=1 ) return 2;
  for( unsigned b=0U; b<nb; b++ ) {
    fd_shredder_core_desc_t desc;
    unsigned sz = 0U;
    if( fread( &desc, 24, 1, f )!=1 || fread( &sz, 4, 1, f )!=1 ) return 2;
    unsigned char * batch = (unsigned char *)malloc( sz ? sz : 1U );
    if( !batch || ( sz && fread( batch, 1, sz, f )!=sz ) ) return 2;
    unsigned long sets, nd, np;
    fd_shredder_core_count( sz, &sets, &nd, &np );
    unsigned long n = nd + np;
    unsigned char ** blk   = (unsigned char **)calloc( n ? n : 1UL, sizeof(unsigned char *) );
    unsigned long *  off   = (unsigned long *) calloc( n ? n : 1UL, sizeof(unsigned long) );
    unsigned int *   ssz   = (unsigned int *)  calloc( n ? n : 1UL, sizeof(unsigned int) );
    unsigned int *   first = (unsigned int *)  calloc( sets+1UL, sizeof(unsigned int) );
    if( !blk || !off || !ssz || !first ) return 2;
    /* each shred is its own block, sized from the plan: offsets are relative to the lowest of them */
    uintptr_t base = UINTPTR_MAX;
    unsigned long at = 0UL;
    for( unsigned long q=0UL; q<sets; q++ ) {
      fd_shredder_core_plan_t pl;
      fd_shredder_core_plan( sz, q, desc.data_idx, desc.parity_idx, &pl );
      if( pl.shred0!=at || pl.off!=q*FD_SHREDDER_CORE_SET_BYTES ) return 4;
      for( unsigned j=0U; j<pl.d+pl.p; j++, at++ ) {
        unsigned long len = j<pl.d ? FD_SHRED_CORE_MIN_SZ : FD_SHRED_CORE_MAX_SZ;
        blk[ at ] = (unsigned char *)malloc( len );
        if( !blk[ at ] ) return 2;
        memset( blk[ at ], 0xA5, len );
        if( (uintptr_t)blk[ at ]<base ) base = (uintptr_t)blk[ at ];
      }
    }
    if( at!=n ) return 4;
    for( unsigned long i=0UL; i<n; i++ ) off[ i ] = (unsigned long)( (uintptr_t)blk[ i ] - base );
    int code = fd_shredder_core_batch( batch, sz, &desc, (unsigned char *)base, off, ssz, first );
    fwrite( &code, 4, 1, out );
    if( !code ) {
      unsigned cnt[ 3 ] = { (unsigned)sets, (unsigned)nd, (unsigned)np };
      fwrite( cnt, 4, 3, out );
      fwrite( first, 4, sets+1UL, out );
      for( unsigned long i=0UL; i<n; i++ ) fwrite( blk[ i ], 1, ssz[ i ], out );
    }
    for( unsigned long i=0UL; i<n; i++ ) free( blk[ i ] );
    free( blk ); free( off ); free( ssz ); free( first ); free( batch );
  }
  unsigned nj = 0U;
  if( fread( &nj, 4, 1, f )!=1 ) return 2;
  for( unsigned j=0U; j<nj; j++ ) {
    uint64_t a[ 9 ];
    if( fread( a, 8, 9, f )!=9 ) return 2;
    int code = fd_shredder_core_judge( a[ 0 ], a[ 1 ], a[ 2 ], a[ 3 ], a[ 4 ], a[ 5 ], a[ 6 ], a[ 7 ], a[ 8 ] );
    fwrite( &code, 4, 1, out );
  }
  fclose( f );
  if( fclose( out ) ) return 2;
  return 0;
}
