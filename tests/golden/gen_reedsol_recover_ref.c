/* gen_reedsol_recover_ref.c -- asks the reference's own Reed-Solomon decoder
   to recover each case of tests/golden/gen_reedsol_recover.py (which builds
   and runs this in a scratch directory against the reference's sources; it
   is never built by the project's build or by a test, and its binary is not
   kept).

     gen_reedsol_recover_ref IN OUT

   IN:  u32 count, then per case u32 d, u32 p, u32 shred_sz, d + p erased
        flags (one byte each) and the d + p slots of shred_sz bytes each, in
        set order, little-endian.
   OUT: per case i32, what fd_reedsol_recover_fini returned, and the d + p
        slots as fd_reedsol_recover_init / _add_rcvd_shred /
        _add_erased_shred / _fini leave them.  Every slot is a heap block of
        exactly its size. */
#include "ballet/reedsol/fd_reedsol.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uchar rs_mem[ FD_REEDSOL_FOOTPRINT ] __attribute__((aligned(FD_REEDSOL_ALIGN)));

int
main( int argc, char ** argv ) {
  if( argc!=3 ) return 2;
  FILE * in  = fopen( argv[ 1 ], "rb" );
  FILE * out = fopen( argv[ 2 ], "wb" );
  if( !in || !out ) return 2;
  uint n = 0U;
  if( fread( &n, 4, 1, in )!=1 ) return 2;
  for( uint t=0U; t<n; t++ ) {
    uint hdr[ 3 ];
    if( fread( hdr, 4, 3, in )!=3 ) return 2;
    uint d = hdr[ 0 ], p = hdr[ 1 ], sz = hdr[ 2 ];
    if( !d || d>FD_REEDSOL_DATA_SHREDS_MAX || !p || p>FD_REEDSOL_PARITY_SHREDS_MAX || sz<32U ) return 3;
    uchar   erased[ FD_REEDSOL_DATA_SHREDS_MAX + FD_REEDSOL_PARITY_SHREDS_MAX ];
    uchar * slot  [ FD_REEDSOL_DATA_SHREDS_MAX + FD_REEDSOL_PARITY_SHREDS_MAX ];
    if( fread( erased, 1, d+p, in )!=d+p ) return 2;
    fd_reedsol_t * rs = fd_reedsol_recover_init( rs_mem, sz );
    for( uint i=0U; i<d+p; i++ ) {
      slot[ i ] = (uchar *)malloc( sz );
      if( !slot[ i ] || fread( slot[ i ], 1, sz, in )!=sz ) return 2;
      if( erased[ i ] ) fd_reedsol_recover_add_erased_shred( rs, i<d, slot[ i ] );
      else              fd_reedsol_recover_add_rcvd_shred  ( rs, i<d, slot[ i ] );
    }
    int ret = fd_reedsol_recover_fini( rs );
    fwrite( &ret, 4, 1, out );
    for( uint i=0U; i<d+p; i++ ) { fwrite( slot[ i ], 1, sz, out ); free( slot[ i ] ); }
  }
  fclose( in );
  if( fclose( out ) ) return 2;
  return 0;
}
