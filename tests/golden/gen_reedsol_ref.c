/* gen_reedsol_ref.c -- asks the reference's own Reed-Solomon encoder for the
   parity of each case of tests/golden/gen_reedsol.py (which builds and runs
   this in a scratch directory against the reference's sources; it is never
   built by the project's build or by a test, and its binary is not kept).

     gen_reedsol_ref IN OUT

   IN:  u32 count, then per case u32 d, u32 p, u32 shred_sz and the d data
        shreds of shred_sz bytes each, little-endian.
   OUT: per case the p parity shreds of shred_sz bytes each, as
        fd_reedsol_encode_init / _add_data_shred / _add_parity_shred / _fini
        leave them.  Every shred is a heap block of exactly its size. */
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
    uchar * data  [ FD_REEDSOL_DATA_SHREDS_MAX   ];
    uchar * parity[ FD_REEDSOL_PARITY_SHREDS_MAX ];
    fd_reedsol_t * rs = fd_reedsol_encode_init( rs_mem, sz );
    for( uint i=0U; i<d; i++ ) {
      data[ i ] = (uchar *)malloc( sz );
      if( !data[ i ] || fread( data[ i ], 1, sz, in )!=sz ) return 2;
      fd_reedsol_encode_add_data_shred( rs, data[ i ] );
    }
    for( uint j=0U; j<p; j++ ) {
      parity[ j ] = (uchar *)malloc( sz );
      if( !parity[ j ] ) return 2;
      memset( parity[ j ], 0xA5, sz );
      fd_reedsol_encode_add_parity_shred( rs, parity[ j ] );
    }
    fd_reedsol_encode_fini( rs );
    for( uint j=0U; j<p; j++ ) { fwrite( parity[ j ], 1, sz, out ); free( parity[ j ] ); }
    for( uint i=0U; i<d; i++ ) free( data[ i ] );
  }
  fclose( in );
  if( fclose( out ) ) return 2;
  return 0;
}
