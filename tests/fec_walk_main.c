/* fec_walk_main.c -- the FEC set rules, the Merkle tree and the proofs
   (fd_fec_core.h) as a stand-alone program for hostile input
   (tests/test_fec_hostile.py builds it with -fsanitize=address,undefined).
   Reads a file of sets (u32 set count; per set u32 shred count, then u32 size
   and the bytes of each shred, little-endian), runs fd_fec_core_root with
   every shred in a heap block of exactly its size -- a read one byte past it
   is a sanitizer report -- and the proofs in a block of exactly 20 depth cnt
   bytes, and prints per set
     code root proofs
   (hex, or - - when the set has a code) as the library's
   fd_ed25519_hip_fec_root reports them. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fd_fec_core.h"

int
main( int argc, char ** argv ) {
  if( argc!=2 ) return 2;
  FILE * f = fopen( argv[ 1 ], "rb" );
  if( !f ) return 2;
  unsigned n_set = 0U;
  if( fread( &n_set, 4, 1, f )!=1 ) return 2;
  for( unsigned k=0U; k<n_set; k++ ) {
    unsigned cnt = 0U;
    if( fread( &cnt, 4, 1, f )!=1 ) return 2;
    unsigned char ** blk = (unsigned char **)calloc( cnt ? cnt : 1U, sizeof(unsigned char *) );
    unsigned long *  off = (unsigned long *) calloc( cnt ? cnt : 1U, sizeof(unsigned long) );
    unsigned int *   sz  = (unsigned int *)  calloc( cnt ? cnt : 1U, sizeof(unsigned int) );
    if( !blk || !off || !sz ) return 2;
    /* each shred is its own block: offsets are relative to the lowest of them */
    uintptr_t base = UINTPTR_MAX;
    for( unsigned j=0U; j<cnt; j++ ) {
      if( fread( &sz[ j ], 4, 1, f )!=1 ) return 2;
      blk[ j ] = (unsigned char *)malloc( sz[ j ] ? sz[ j ] : 1U );
      if( !blk[ j ] || ( sz[ j ] && fread( blk[ j ], 1, sz[ j ], f )!=sz[ j ] ) ) return 2;
      if( !sz[ j ] ) { free( blk[ j ] ); blk[ j ] = (unsigned char *)malloc( 1 ); }   /* nothing of it may be read */
      if( (uintptr_t)blk[ j ]<base ) base = (uintptr_t)blk[ j ];
    }
    for( unsigned j=0U; j<cnt; j++ ) off[ j ] = (unsigned long)( (uintptr_t)blk[ j ] - base );
    unsigned depth = ( cnt>=1U && cnt<=FD_FEC_CORE_CNT_MAX ) ? fd_fec_core_depth( cnt ) : 0U;
    unsigned long proof_sz = 20UL*depth*cnt;
    unsigned char * proofs = (unsigned char *)malloc( proof_sz ? proof_sz : 1UL );
    if( !proofs ) return 2;
    memset( proofs, 0xA5, proof_sz );
    unsigned char root[ 32 ];
    memset( root, 0xA5, 32 );
    /* a set of no shreds comes without arrays */
    int code = cnt ? fd_fec_core_root( (unsigned char const *)base, off, sz, cnt, root, proofs ) : fd_fec_core_root( NULL, NULL, NULL, 0UL, root, NULL );
    printf( "%d ", code );
    if( code ) {
      for( int i=0; i<32; i++ ) if( root[ i ]!=0xA5 ) return 3;                 /* untouched without a root */
      for( unsigned long i=0UL; i<proof_sz; i++ ) if( proofs[ i ]!=0xA5 ) return 3;
      printf( "- -\n" );
    } else {
      for( int i=0; i<32; i++ ) printf( "%02x", root[ i ] );
      printf( " " );
      for( unsigned long i=0UL; i<proof_sz; i++ ) printf( "%02x", proofs[ i ] );
      printf( "%s\n", proof_sz ? "" : "-" );
    }
    for( unsigned j=0U; j<cnt; j++ ) free( blk[ j ] );
    free( proofs ); free( blk ); free( off ); free( sz );
  }
  fclose( f );
  return 0;
}
