/* The workspace layout of the proof-of-history check (front_work_poh,
   firedancer_amd/csrc/fd_front_work.h) against the public
   FD_ED25519_HIP_POH_WORK_BYTES macro a caller sizes the buffer with.
   Stand-alone, built under ASan and UBSan by tests/test_poh_work.py; only
   pointers are formed, no array is touched.

   Prints the number of layouts checked; exit 1 with the first failure. */
#include "fd_ed25519_hip.h"
#include "fd_front_work.h"

#include <stdio.h>
#include <stdlib.h>

#define BUF_BYTES ( 96UL<<20 )

static uint8_t * buf;

static int
poh( uint64_t n, uint64_t n_sig ) {
# define FAIL( ... ) do { printf( "poh(%lu,%lu): ", (unsigned long)n, (unsigned long)n_sig ); printf( __VA_ARGS__ ); \
                          printf( "\n" ); return 1; } while(0)
  front_work_poh_t w;
  uint64_t end = front_work_poh( buf, n, n_sig, &w ), public_bytes = FD_ED25519_HIP_POH_WORK_BYTES( n, n_sig );
  if( end>public_bytes ) FAIL( "end %lu past the public %lu", (unsigned long)end, (unsigned long)public_bytes );
  if( public_bytes>BUF_BYTES ) FAIL( "test buffer too small" );
  /* the rows of eight words are read and written as two uint4 */
  if( (uint8_t *)w.leaves!=buf || (uintptr_t)w.leaves % 16UL ) FAIL( "leaves" );
  if( (uint8_t *)w.roots!=buf + 32UL*n_sig || (uintptr_t)w.roots % 16UL ) FAIL( "roots" );
  if( (uint8_t *)w.pre!=buf + 32UL*n_sig + 32UL*n ) FAIL( "pre" );
  if( end!=32UL*n_sig + 33UL*n ) FAIL( "end %lu", (unsigned long)end );
  return 0;
# undef FAIL
}

int
main( void ) {
  buf = aligned_alloc( 16UL, BUF_BYTES );
  if( !buf ) return 2;
  uint64_t ns[ 8 ] = { 0UL, 1UL, 2UL, 63UL, 64UL, 65UL, 257UL, 16384UL }, cases = 0UL;
  for( int i=0; i<8; i++ ) {
    uint64_t n = ns[i];
    uint64_t n_sig[ 6 ] = { 0UL, 1UL, n, 20UL*n + 1UL, 127UL*n, 300UL };
    for( int k=0; k<6; k++, cases++ ) if( poh( n, n_sig[k] ) ) return 1;
  }
  free( buf );
  printf( "%lu layouts\n", (unsigned long)cases );
  return 0;
}
