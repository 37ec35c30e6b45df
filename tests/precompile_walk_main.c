/* precompile_walk_main.c -- the Ed25519 precompile walk (fd_precompile_core.h
   on fd_txn_parse_core.h) as a stand-alone program for hostile input
   (tests/test_precompile_hostile.py builds it with
   -fsanitize=address,undefined).  Reads a file of payloads (u32 count, then
   u32 size and the bytes of each, little-endian), runs the count and the
   plan on a heap copy of exactly the payload's size -- a read one byte past
   it is a sanitizer report -- and prints per payload
     count entries code instr checksum
   as the library's precompile_count and precompile_plan report them. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fd_ed25519_hip_tile.h"   /* fd_ed25519_hip_txn_t */
#include "fd_txn_parse_core.h"
#include "fd_precompile_core.h"

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
    if( !sz ) { free( p ); p = (unsigned char *)malloc( 1 ); }   /* a payload of no bytes: nothing may be read */
    fd_precompile_core_sum_t sum, sum0;
    fd_precompile_core_ent_t ents[ FD_PRECOMPILE_CORE_ENT_MAX ];
    int parsed, parsed0;
    fd_precompile_core_plan( p, sz, NULL, 0UL, &sum0, &parsed0 );                             /* the count */
    int k = fd_precompile_core_plan( p, sz, ents, FD_PRECOMPILE_CORE_ENT_MAX, &sum, &parsed ); /* the plan  */
    if( parsed!=parsed0 || sum.ent_cnt!=sum0.ent_cnt || (unsigned)k!=sum.ent_cnt ) return 3;
    unsigned long h = 0UL;
    for( int i=0; i<k; i++ )
      h = h*1000003UL + ents[ i ].instr + 3UL*(unsigned char)ents[ i ].pre + 5UL*ents[ i ].sig_off + 7UL*ents[ i ].pub_off
        + 11UL*ents[ i ].msg_off + 13UL*ents[ i ].msg_sz;
    printf( "%u %d %d %u %lu\n", sum0.ent_cnt, k,
            !parsed ? -16 : sum.hdr_instr!=0xFF ? FD_PRECOMPILE_CORE_ERR_INSTR_DATA_SIZE : 0, (unsigned)sum.hdr_instr, h );
    free( p );
  }
  fclose( f );
  return 0;
}
