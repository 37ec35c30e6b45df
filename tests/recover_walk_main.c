/* recover_walk_main.c -- the recovery's rules and its decoder
   (fd_reedsol_core.h, rules 9-12) as a stand-alone program for hostile input
   (tests/test_recover_hostile.py builds it with -fsanitize=address,undefined).

     recover_walk IN OUT

   Reads a file of sets (u32 set count; per set u32 slot count, then per slot
   u8 erased, u32 size and the bytes of the slot, little-endian), runs
   fd_reedsol_core_recover with every slot in a heap block of exactly its size
   -- a read or a write one byte outside it is a sanitizer report -- and an
   erased array of exactly the slot count, and writes per set the code (i32)
   and, for code 0, the bytes of every slot after the call.  A set with a code
   must come back as it went in: the program compares and returns 3.  First it
   builds the device kernels' tables in a block of exactly their size. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fd_reedsol_core.h"

int
main( int argc, char ** argv ) {
  if( argc!=3 ) return 2;
  FILE * f   = fopen( argv[ 1 ], "rb" );
  FILE * out = fopen( argv[ 2 ], "wb" );
  if( !f || !out ) return 2;
  unsigned char * tab = (unsigned char *)malloc( FD_REEDSOL_CORE_TAB_BYTES );
  if( !tab ) return 2;
  fd_reedsol_core_tables( tab );
  /* exp[ 0 ] = 1, exp[ 8 ] = 0x1d, log[ 2 ] = 1, and the last byte is log[ 255 ] */
  if( tab[ FD_REEDSOL_CORE_GF_AT ]!=1U || tab[ FD_REEDSOL_CORE_GF_AT + 8 ]!=0x1dU || tab[ FD_REEDSOL_CORE_GF_AT + 512 + 2 ]!=1U ||
      tab[ FD_REEDSOL_CORE_TAB_BYTES - 1 ]!=175U ) return 4;
  free( tab );
  unsigned n_set = 0U;
  if( fread( &n_set, 4, 1, f )!=1 ) return 2;
  for( unsigned k=0U; k<n_set; k++ ) {
    unsigned cnt = 0U;
    if( fread( &cnt, 4, 1, f )!=1 ) return 2;
    unsigned char ** blk = (unsigned char **)calloc( cnt ? cnt : 1U, sizeof(unsigned char *) );
    unsigned char ** cpy = (unsigned char **)calloc( cnt ? cnt : 1U, sizeof(unsigned char *) );
    unsigned long *  off = (unsigned long *) calloc( cnt ? cnt : 1U, sizeof(unsigned long) );
    unsigned int *   sz  = (unsigned int *)  calloc( cnt ? cnt : 1U, sizeof(unsigned int) );
    unsigned char *  er  = (unsigned char *) malloc( cnt ? cnt : 1U );
    if( !blk || !cpy || !off || !sz || !er ) return 2;
    /* each slot is its own block: offsets are relative to the lowest of them */
    uintptr_t base = UINTPTR_MAX;
    for( unsigned j=0U; j<cnt; j++ ) {
      if( fread( &er[ j ], 1, 1, f )!=1 || fread( &sz[ j ], 4, 1, f )!=1 ) return 2;
      blk[ j ] = (unsigned char *)malloc( sz[ j ] ? sz[ j ] : 1U );
      cpy[ j ] = (unsigned char *)malloc( sz[ j ] ? sz[ j ] : 1U );
      if( !blk[ j ] || !cpy[ j ] || ( sz[ j ] && fread( blk[ j ], 1, sz[ j ], f )!=sz[ j ] ) ) return 2;
      if( !sz[ j ] ) { free( blk[ j ] ); blk[ j ] = (unsigned char *)malloc( 1 ); }   /* nothing of it may be read */
      if( sz[ j ] ) memcpy( cpy[ j ], blk[ j ], sz[ j ] );
      if( (uintptr_t)blk[ j ]<base ) base = (uintptr_t)blk[ j ];
    }
    for( unsigned j=0U; j<cnt; j++ ) off[ j ] = (unsigned long)( (uintptr_t)blk[ j ] - base );
    /* a set of no slots comes without arrays */
    int code = cnt ? fd_reedsol_core_recover( (unsigned char *)base, off, sz, er, cnt )
                   : fd_reedsol_core_recover( NULL, NULL, NULL, NULL, 0UL );
    fwrite( &code, 4, 1, out );
    for( unsigned j=0U; j<cnt; j++ ) {
      if( code ) { if( sz[ j ] && memcmp( blk[ j ], cpy[ j ], sz[ j ] ) ) return 3; }
      else       fwrite( blk[ j ], 1, sz[ j ], out );
    }
    for( unsigned j=0U; j<cnt; j++ ) { free( blk[ j ] ); free( cpy[ j ] ); }
    free( blk ); free( cpy ); free( off ); free( sz ); free( er );
  }
  fclose( f );
  if( fclose( out ) ) return 2;
  return 0;
}
