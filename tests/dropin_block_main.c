/* The pinned block of a drop-in launch (firedancer_amd/csrc/fd_dropin_block.h)
   over a grid of launches, one line a case for tests/test_dropin_block.py,
   which holds every offset to the formulas the drop-in used before the
   layout had a header of its own.  Stand-alone, built under ASan and UBSan;
   integer arithmetic only, no array is touched.

   A line: n nsig nsig_h bytes hsmode hs_bytes, then the struct's members in
   its order.  The first line is the two host-scalar block sizes
   (fd_ed25519_hip_private_hs_bytes's: the host-decoded stride, and the
   drop-in engines' work arrays' stride with the device decoding), from
   fd_ed25519_hip_internal.h's constants. */
#include "fd_ed25519_hip_internal.h"
#include "fd_dropin_block.h"

#include <stdio.h>

#define DROPIN_CHUNK 16384UL   /* the drop-in engines' max_chunk (host/fd_ed25519_hip_dropin.c) */

int
main( void ) {
  uint64_t hs_decode = FD_ED25519_HS_O_GO( FD_ED25519_HS_STRIDE ) + 16UL;
  uint64_t hs_device = FD_ED25519_HS_O_HS( DROPIN_CHUNK ) + 19UL*4UL*DROPIN_CHUNK;
  printf( "%lu %lu\n", (unsigned long)hs_decode, (unsigned long)hs_device );
  static uint64_t const ns[ 3 ] = { 1UL, 2UL, 17UL }, per[ 3 ] = { 1UL, 2UL, 16UL };
  static uint64_t const bytes[ 7 ] = { 0UL, 1UL, 15UL, 16UL, 17UL, 65536UL, 65537UL };
  uint64_t const hs_bytes[ 4 ] = { 0UL /* hsmode off */, 0UL, hs_decode, hs_device };
  for( int a=0; a<3; a++ ) for( int p=0; p<3; p++ ) for( int m=0; m<7; m++ ) for( int g=0; g<3; g++ ) for( int s=0; s<4; s++ ) {
    uint64_t n = ns[ a ], nsig = n*per[ p ], nsig_h = g==0 ? 0UL : g==1 ? 1UL : nsig;
    fd_dropin_block_t b;
    fd_dropin_block( n, nsig, nsig_h, bytes[ m ], s>0, hs_bytes[ s ], &b );
    printf( "%lu %lu %lu %lu %d %lu  %lu %lu %lu %lu %lu %lu %lu %lu %lu %lu %lu %lu %lu\n", (unsigned long)n,
            (unsigned long)nsig, (unsigned long)nsig_h, (unsigned long)bytes[ m ], s>0, (unsigned long)hs_bytes[ s ],
            (unsigned long)b.o_off, (unsigned long)b.o_sz, (unsigned long)b.o_tf, (unsigned long)b.o_tc,
            (unsigned long)b.o_sig, (unsigned long)b.o_pub, (unsigned long)b.o_dig, (unsigned long)b.o_msg,
            (unsigned long)b.in_sz, (unsigned long)b.o_out, (unsigned long)b.o_tout, (unsigned long)b.o_hsb,
            (unsigned long)b.need );
  }
  return 0;
}
