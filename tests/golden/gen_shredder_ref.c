/* gen_shredder_ref.c -- asks the reference's own shredder for the FEC sets of
   each case of tests/golden/gen_shredder.py (which builds and runs this in a
   scratch directory against the reference's sources; it is never built by the
   project's build or by a test, and its binary is not kept).

     gen_shredder_ref IN OUT

   IN:  u32 cases; per case u64 slot, u16 version, u64 skip_sz (a batch size
        handed to fd_shredder_skip_batch first, 0 for none), u32 batches; per
        batch u64 parent_offset, u64 reference_tick, u32 block_complete, u32 sz
        and the sz bytes.  Little-endian.
   OUT: per batch u32 fd_shredder_count_fec_sets, _data_shreds, _parity_shreds
        of sz; then per set of fd_shredder_next_fec_set u32 d, u32 p, the d
        data shreds of 1203 bytes and the p parity shreds of 1228.

   The signer writes 64 zero bytes, so no private key is involved.  Every
   shred is a heap block of exactly its size. */
#include "disco/shred/fd_shredder.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uchar shredder_mem[ sizeof(fd_shredder_t) ] __attribute__((aligned(FD_SHREDDER_ALIGN)));

static void
zero_signer( void * ctx, uchar * sig, uchar const * root ) {
  (void)ctx; (void)root;
  memset( sig, 0, 64UL );
}

int
main( int argc, char ** argv ) {
  if( argc!=3 ) return 2;
  FILE * in  = fopen( argv[ 1 ], "rb" );
  FILE * out = fopen( argv[ 2 ], "wb" );
  if( !in || !out ) return 2;
  uint cases = 0U;
  if( fread( &cases, 4, 1, in )!=1 ) return 2;
  for( uint c=0U; c<cases; c++ ) {
    ulong slot, skip_sz; ushort version; uint batches;
    if( fread( &slot, 8, 1, in )!=1 || fread( &version, 2, 1, in )!=1 || fread( &skip_sz, 8, 1, in )!=1 ||
        fread( &batches, 4, 1, in )!=1 ) return 2;
    if( !fd_shredder_new( shredder_mem, zero_signer, NULL, version ) ) return 3;
    fd_shredder_t * shredder = fd_shredder_join( shredder_mem );
    if( !shredder ) return 3;
    if( skip_sz && !fd_shredder_skip_batch( shredder, skip_sz, slot ) ) return 3;
    for( uint b=0U; b<batches; b++ ) {
      ulong parent_offset, reference_tick; uint block_complete, sz;
      if( fread( &parent_offset, 8, 1, in )!=1 || fread( &reference_tick, 8, 1, in )!=1 || fread( &block_complete, 4, 1, in )!=1 ||
          fread( &sz, 4, 1, in )!=1 ) return 2;
      uchar * batch = (uchar *)malloc( sz ? sz : 1U );
      if( !batch || ( sz && fread( batch, 1, sz, in )!=sz ) ) return 2;
      uint cnt[ 3 ] = { (uint)fd_shredder_count_fec_sets( sz ), (uint)fd_shredder_count_data_shreds( sz ),
                        (uint)fd_shredder_count_parity_shreds( sz ) };
      fwrite( cnt, 4, 3, out );
      fd_entry_batch_meta_t meta[ 1 ];
      memset( meta, 0, sizeof(fd_entry_batch_meta_t) );
      meta->parent_offset  = parent_offset;
      meta->reference_tick = reference_tick;
      meta->block_complete = (int)block_complete;
      if( !fd_shredder_init_batch( shredder, batch, sz, slot, meta ) ) return 3;
      for( uint s=0U; s<cnt[ 0 ]; s++ ) {
        fd_fec_set_t set[ 1 ];
        memset( set, 0, sizeof(fd_fec_set_t) );
        for( ulong j=0UL; j<FD_REEDSOL_DATA_SHREDS_MAX; j++ ) {
          set->data_shreds[ j ] = (uchar *)malloc( 1203UL );
          if( !set->data_shreds[ j ] ) return 2;
          memset( set->data_shreds[ j ], 0xA5, 1203UL );
        }
        for( ulong j=0UL; j<FD_REEDSOL_PARITY_SHREDS_MAX; j++ ) {
          set->parity_shreds[ j ] = (uchar *)malloc( 1228UL );
          if( !set->parity_shreds[ j ] ) return 2;
          memset( set->parity_shreds[ j ], 0xA5, 1228UL );
        }
        if( !fd_shredder_next_fec_set( shredder, set ) ) return 4;
        uint dp[ 2 ] = { (uint)set->data_shred_cnt, (uint)set->parity_shred_cnt };
        fwrite( dp, 4, 2, out );
        for( uint j=0U; j<dp[ 0 ]; j++ ) fwrite( set->data_shreds[ j ],   1, 1203UL, out );
        for( uint j=0U; j<dp[ 1 ]; j++ ) fwrite( set->parity_shreds[ j ], 1, 1228UL, out );
        for( ulong j=0UL; j<FD_REEDSOL_DATA_SHREDS_MAX;   j++ ) free( set->data_shreds[ j ] );
        for( ulong j=0UL; j<FD_REEDSOL_PARITY_SHREDS_MAX; j++ ) free( set->parity_shreds[ j ] );
      }
      fd_fec_set_t none[ 1 ];
      if( fd_shredder_next_fec_set( shredder, none ) ) return 4;   /* the batch is used up */
      fd_shredder_fini_batch( shredder );
      free( batch );
    }
  }
  fclose( in );
  if( fclose( out ) ) return 2;
  return 0;
}
