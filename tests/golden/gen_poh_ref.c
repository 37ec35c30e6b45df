/* gen_poh_ref.c -- asks the reference's own proof-of-history functions for
   the cases of tests/golden/gen_poh.py (which builds and runs this in a
   scratch directory against the reference's sources; it is never built by
   the project's build or by a test, and its binary is not kept).

     gen_poh_ref IN OUT

   IN: u32 count, then per op a u8 kind and, little-endian:
     1 root        u32 S, S signatures of 64 bytes
                   -> 32 bytes fd_wbmtree32's root, 32 bytes fd_bmtree_commit's
                      (32-byte nodes, 1-byte prefix)
     2 append      32-byte state, u64 k            -> 32 bytes fd_poh_append
     3 mixin       32-byte state, 32-byte root     -> 32 bytes fd_poh_mixin
     4 microblock  32-byte in, u64 hash_cnt, u64 txn_cnt, u32 S, S signatures
                   -> 32 bytes: the steps of fd_runtime_poh_verify_wide_task
                      (fd_runtime.c:2017-2057) made with those functions
     5 txn         u32 size, the bytes             -> u64 payload size, 0 for a
                      transaction fd_txn_parse_core rejects (offered
                      min( size, 1232 ) bytes, as fd_runtime_parse_microblock_txns
                      offers them)
     6 rates       u64 hashes, u64 roots           -> f64 fd_poh_append hashes/s
                      over one call of `hashes`, f64 20-leaf roots/s over
                      `roots` calls, one core */
#include "ballet/poh/fd_poh.h"
#include "ballet/bmtree/fd_bmtree.h"
#include "ballet/bmtree/fd_wbmtree.h"
#include "ballet/txn/fd_txn.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

static void
wb_root( uchar out[ 32 ], uchar * sigs, ulong cnt ) {
  void *                mem   = aligned_alloc( FD_WBMTREE32_ALIGN, ( fd_wbmtree32_footprint( cnt ) + 127UL ) & ~127UL );
  fd_wbmtree32_leaf_t * leafs = (fd_wbmtree32_leaf_t *)malloc( cnt*sizeof(fd_wbmtree32_leaf_t) );
  uchar *               mbuf  = (uchar *)malloc( cnt*65UL );
  if( !mem || !leafs || !mbuf ) exit( 2 );
  fd_wbmtree32_t * tree = fd_wbmtree32_init( mem, cnt );
  for( ulong j=0UL; j<cnt; j++ ) { leafs[ j ].data = sigs + 64UL*j; leafs[ j ].data_len = 64UL; }
  fd_wbmtree32_append( tree, leafs, cnt, mbuf );
  memcpy( out, fd_wbmtree32_fini( tree ), 32UL );
  free( mem ); free( leafs ); free( mbuf );
}

static void
bm_root( uchar out[ 32 ], uchar * sigs, ulong cnt ) {
  void * mem = aligned_alloc( 128UL, ( fd_bmtree_commit_footprint( 0UL ) + 127UL ) & ~127UL );
  if( !mem ) exit( 2 );
  fd_bmtree_commit_t * st = fd_bmtree_commit_init( mem, 32UL, FD_BMTREE_SHORT_PREFIX_SZ, 0UL );
  for( ulong j=0UL; j<cnt; j++ ) {
    fd_bmtree_node_t leaf[ 1 ];
    fd_bmtree_hash_leaf( leaf, sigs + 64UL*j, 64UL, FD_BMTREE_SHORT_PREFIX_SZ );
    fd_bmtree_commit_append( st, leaf, 1UL );
  }
  memcpy( out, fd_bmtree_commit_fini( st ), 32UL );
  free( mem );
}

static double
now( void ) {
  struct timespec ts;
  clock_gettime( CLOCK_MONOTONIC, &ts );
  return (double)ts.tv_sec + 1e-9*(double)ts.tv_nsec;
}

#define RD( p, sz ) do { if( fread( (p), 1, (sz), in )!=(size_t)(sz) ) return 2; } while(0)

int
main( int argc, char ** argv ) {
  if( argc!=3 ) return 2;
  FILE * in  = fopen( argv[ 1 ], "rb" );
  FILE * out = fopen( argv[ 2 ], "wb" );
  if( !in || !out ) return 2;
  uint n = 0U;
  RD( &n, 4 );
  for( uint t=0U; t<n; t++ ) {
    uchar kind, state[ 32 ], root[ 32 ];
    RD( &kind, 1 );
    if( kind==1 ) {
      uint s; RD( &s, 4 );
      uchar * sigs = (uchar *)malloc( 64UL*s );
      if( !s || !sigs ) return 3;
      RD( sigs, 64UL*s );
      wb_root( root, sigs, s );  fwrite( root, 1, 32, out );
      bm_root( root, sigs, s );  fwrite( root, 1, 32, out );
      free( sigs );
    } else if( kind==2 ) {
      ulong k; RD( state, 32 ); RD( &k, 8 );
      fd_poh_append( state, k );
      fwrite( state, 1, 32, out );
    } else if( kind==3 ) {
      RD( state, 32 ); RD( root, 32 );
      fd_poh_mixin( state, root );
      fwrite( state, 1, 32, out );
    } else if( kind==4 ) {
      ulong hash_cnt, txn_cnt; uint s;
      RD( state, 32 ); RD( &hash_cnt, 8 ); RD( &txn_cnt, 8 ); RD( &s, 4 );
      uchar * sigs = (uchar *)malloc( s ? 64UL*s : 1UL );
      if( !sigs ) return 3;
      RD( sigs, 64UL*s );
      if( txn_cnt==0UL ) {
        fd_poh_append( state, hash_cnt );
      } else {
        if( hash_cnt>0UL ) fd_poh_append( state, hash_cnt-1UL );
        if( !s ) return 3;
        wb_root( root, sigs, s );
        fd_poh_mixin( state, root );
      }
      fwrite( state, 1, 32, out );
      free( sigs );
    } else if( kind==5 ) {
      uint sz; RD( &sz, 4 );
      uchar * p = (uchar *)malloc( sz ? sz : 1U );
      uchar   txn[ FD_TXN_MAX_SZ ] __attribute__((aligned(8)));
      if( !p ) return 3;
      RD( p, sz );
      ulong pay = 0UL;
      ulong got = fd_txn_parse_core( p, sz<FD_TXN_MTU ? sz : FD_TXN_MTU, txn, NULL, &pay, 0 );
      if( !got || got>FD_TXN_MTU ) pay = 0UL;
      fwrite( &pay, 8, 1, out );
      free( p );
    } else if( kind==6 ) {
      ulong hashes, roots; RD( &hashes, 8 ); RD( &roots, 8 );
      memset( state, 7, 32 );
      double t0 = now();
      fd_poh_append( state, hashes );
      double r_hash = (double)hashes/( now()-t0 );
      uchar sigs[ 20*64 ];
      for( ulong i=0UL; i<sizeof(sigs); i++ ) sigs[ i ] = (uchar)( state[ i & 31 ] + i );
      t0 = now();
      for( ulong i=0UL; i<roots; i++ ) { wb_root( root, sigs, 20UL ); sigs[ 0 ] ^= root[ 0 ]; }
      double r_root = (double)roots/( now()-t0 );
      fwrite( &r_hash, 8, 1, out ); fwrite( &r_root, 8, 1, out );
    } else return 3;
  }
  fclose( in );
  if( fclose( out ) ) return 2;
  return 0;
}
