/* A pass of fd_ed25519_hip_shredder_host (firedancer_amd/csrc/fd_shredder_pass.h):
   the reservation, the cut, the in block's layout, the staging and the copy
   back, on buffers of exactly the sizes the header states -- item_bytes of
   item staging, total of in block, n_set + 1 elements of set_first_out -- so
   that ASan sees any write past them.  Stand-alone, built under ASan and
   UBSan by tests/test_shredder_pass.py.

   The calls, each without and with keys:
     inside   112 batches of 63,679 bytes (134 shreds), one of 700,000, two
              more of 63,679: the first pass stops inside the large batch
     front    123 batches of 63,679: the first pass stops exactly in front of
              batch 122 (122 x 134 = 16,348, and the next 134 do not fit)
     zeros    the same with batches of no bytes in front of the first batch,
              between batches 121 and 122 and behind the last
     tiny     911 batches of 1 byte (18 shreds): the boundary falls between
              two of them (910 x 18 = 16,380)
     none     batches of no bytes alone: no pass
   and, sizes only, 16,384 batches of 0xFFFFFFFF bytes, which the reservation
   must refuse.  What a pass should hold is worked out here from a table of
   the call's sets made with fd_shredder_core_count and the public header's
   words (every set of a batch but the last: 31,840 bytes, 64 shreds).

   Prints the passes, sets and shreds checked; exit 1 with the first
   failure. */
#define _POSIX_C_SOURCE 200112L   /* posix_memalign */
#include "fd_ed25519_hip.h"
#include "fd_shredder_pass.h"

#include <stdio.h>
#include <stdlib.h>

#define FAIL( ... ) do { printf( "%s keys %d pass at set %lu: ", name, has_keys, (unsigned long)k0 ); \
                         printf( __VA_ARGS__ ); printf( "\n" ); fflush( stdout ); return 1; } while(0)

#define FILL   0xA5
#define GAP    3UL      /* bytes between two batches in the caller's buffer */
#define STRIDE 1231UL   /* the caller's shreds_out */

static uint32_t
hash32( uint32_t x ) { x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16; return x; }

static uint64_t passes, sets_cut, shreds_cut;

/* one set of the call, as the public header's words have it */
typedef struct { uint64_t batch, q, shreds, bytes; } set_t;

static int
run( char const * name, uint64_t nb, unsigned int const * batch_sz, int has_keys ) {
  uint64_t k0 = 0UL;

  /* ---- the caller's arrays ---- */
  uint64_t buf_bytes = 0UL;
  unsigned long * batch_off = malloc( sizeof(unsigned long)*nb );
  if( !batch_off ) return 2;
  for( uint64_t b=0UL; b<nb; b++ ) { batch_off[b] = buf_bytes; buf_bytes += batch_sz[b] + GAP; }
  unsigned char *           batches   = malloc( buf_bytes );
  fd_shredder_core_desc_t * desc      = malloc( sizeof(fd_shredder_core_desc_t)*nb );
  unsigned char *           privs     = malloc( 32UL*nb );
  signed char *             batch_out = malloc( nb );
  uint32_t *                gs        = malloc( 4UL*( nb+1UL ) );
  uint32_t *                gh        = malloc( 4UL*( nb+1UL ) );
  uint32_t *                want_gs   = malloc( 4UL*( nb+1UL ) );
  uint32_t *                want_gh   = malloc( 4UL*( nb+1UL ) );
  if( !batches || !desc || !privs || !batch_out || !gs || !gh || !want_gs || !want_gh ) return 2;
  for( uint64_t i=0UL; i<buf_bytes; i++ ) batches[i] = (unsigned char)( hash32( (uint32_t)i ) | 1U );   /* no zero byte */
  for( uint64_t i=0UL; i<sizeof(fd_shredder_core_desc_t)*nb; i++ ) ( (unsigned char *)desc )[i] = (unsigned char)hash32( (uint32_t)i ^ 0xde5cU );
  for( uint64_t i=0UL; i<32UL*nb; i++ ) privs[i] = (unsigned char)hash32( (uint32_t)i ^ 0x4e75U );

  /* ---- the call's sets, from the counts ---- */
  uint64_t N = 0UL, M = 0UL;
  for( uint64_t b=0UL; b<nb; b++ ) {
    unsigned long sets, nd, np;
    fd_shredder_core_count( batch_sz[b], &sets, &nd, &np );
    want_gs[b] = (uint32_t)N; want_gh[b] = (uint32_t)M;
    N += sets; M += nd + np;
  }
  want_gs[nb] = (uint32_t)N; want_gh[nb] = (uint32_t)M;
  set_t * set = malloc( sizeof(set_t)*( N ? N : 1UL ) );
  if( !set ) return 2;
  for( uint64_t b=0UL, k=0UL; b<nb; b++ ) {
    uint64_t sets = want_gs[b+1UL]-want_gs[b], total = want_gh[b+1UL]-want_gh[b];
    for( uint64_t q=0UL; q<sets; q++, k++ ) {
      set[k].batch = b; set[k].q = q;
      set[k].shreds = q+1UL<sets ? 64UL : total - 64UL*( sets-1UL );
      set[k].bytes  = q+1UL<sets ? 31840UL : batch_sz[b] - 31840UL*( sets-1UL );
    }
  }

  /* ---- the reservation ---- */
  uint64_t got_N = ~0UL, got_M = ~0UL;
  memset( gs, FILL, 4UL*( nb+1UL ) ); memset( gh, FILL, 4UL*( nb+1UL ) ); memset( batch_out, FILL, nb );
  if( fd_shredder_pass_reserve( batch_sz, nb, gs, gh, batch_out, &got_N, &got_M ) ) FAIL( "the reservation failed" );
  if( got_N!=N || got_M!=M ) FAIL( "reserved %lu sets, %lu shreds, not %lu, %lu", (unsigned long)got_N, (unsigned long)got_M, (unsigned long)N, (unsigned long)M );
  if( memcmp( gs, want_gs, 4UL*( nb+1UL ) ) || memcmp( gh, want_gh, 4UL*( nb+1UL ) ) ) FAIL( "the prefix arrays differ" );
  for( uint64_t b=0UL; b<nb; b++ )
    if( batch_out[b]!=( batch_sz[b] ? 0 : FD_ED25519_HIP_SHREDDER_ERR_BATCH ) ) FAIL( "batch %lu got code %d", (unsigned long)b, batch_out[b] );

  unsigned int * set_first_out = malloc( 4UL*( N+1UL ) );
  if( !set_first_out ) return 2;
  memset( set_first_out, FILL, 4UL*( N+1UL ) );
  set_first_out[0] = 0U;

  fd_shredder_pass_cur_t cur = { 0UL, 0UL, 0UL, 0UL };
  uint64_t h0 = 0UL;
  while( cur.k<N ) {
    fd_shredder_pass_t ps = fd_shredder_pass_cut( batch_sz, gs, N, &cur, set_first_out );

    /* ---- the cut: it starts where the last one stopped, advances, keeps the bound and is greedy ---- */
    if( ps.k!=k0 || ps.h!=h0 ) FAIL( "it starts at set %lu, shred %lu, not at shred %lu", (unsigned long)ps.k, (unsigned long)ps.h, (unsigned long)h0 );
    if( !ps.ms || ps.k+ps.ms>N ) FAIL( "%lu sets", (unsigned long)ps.ms );
    if( ps.b!=set[k0].batch || ps.q!=set[k0].q ) FAIL( "it starts at set %lu of batch %lu", (unsigned long)ps.q, (unsigned long)ps.b );
    uint64_t k1 = k0+ps.ms, want_m = 0UL, want_bytes = 0UL;
    for( uint64_t k=k0; k<k1; k++ ) {
      want_m += set[k].shreds; want_bytes += set[k].bytes;
      if( set_first_out[ k+1UL ]!=h0+want_m ) FAIL( "set_first_out[%lu] is %u, not %lu", (unsigned long)( k+1UL ), set_first_out[ k+1UL ], (unsigned long)( h0+want_m ) );
    }
    for( uint64_t k=k1+1UL; k<=N; k++ ) if( set_first_out[k]!=FILL*0x01010101U ) FAIL( "set_first_out[%lu] written early", (unsigned long)k );
    if( ps.m!=want_m || ps.bytes!=want_bytes ) FAIL( "%lu shreds, %lu bytes; its sets have %lu, %lu", (unsigned long)ps.m, (unsigned long)ps.bytes, (unsigned long)want_m, (unsigned long)want_bytes );
    if( ps.m>16384UL || ps.ms>16384UL ) FAIL( "%lu shreds, %lu sets", (unsigned long)ps.m, (unsigned long)ps.ms );
    if( k1<N && ps.m+set[k1].shreds<=16384UL ) FAIL( "set %lu would have fit", (unsigned long)k1 );
    if( ps.b1!=set[k1-1UL].batch || ps.q1!=set[k1-1UL].q+1UL ) FAIL( "it ends with %lu sets of batch %lu", (unsigned long)ps.q1, (unsigned long)ps.b1 );
    if( ps.nbp!=ps.b1-ps.b+1UL ) FAIL( "nbp %lu", (unsigned long)ps.nbp );
    if( cur.k!=k1 || cur.h!=h0+want_m ) FAIL( "the cursor stands at set %lu, shred %lu", (unsigned long)cur.k, (unsigned long)cur.h );
    if( k1<N && ( cur.b>set[k1].batch || ( cur.b==set[k1].batch ? cur.q!=set[k1].q : cur.q!=0UL ) ) )
      FAIL( "the cursor stands at set %lu of batch %lu", (unsigned long)cur.q, (unsigned long)cur.b );
    for( uint64_t c=cur.b; k1<N && c<set[k1].batch; c++ ) if( batch_sz[c] ) FAIL( "the cursor stands in front of batch %lu, which has bytes", (unsigned long)c );

    /* ---- the in block and the item staging ---- */
    fd_shredder_pass_in_t at = fd_shredder_pass_in( &ps, has_keys );
    uint64_t nbp = ps.nbp;
    struct { char const * name; uint64_t at, elem, cnt, align; } arr[ 9 ] = {
      { "keys",          at.keys_at,      32UL, has_keys ? nbp : 0UL, 16UL },
      { "batch_off",     at.off_at,        8UL, nbp,                   8UL },
      { "desc",          at.desc_at,      24UL, nbp,                   8UL },
      { "set_first_b",   at.sfb_at,        4UL, nbp+1UL,               4UL },
      { "shred_first_b", at.hfb_at,        4UL, nbp+1UL,               4UL },
      { "batch_sz",      at.sz_at,         4UL, nbp,                   4UL },
      { "shred_off",     at.shred_off_at,  8UL, ps.m,                  8UL },
      { "shred_sz",      at.shred_sz_at,   4UL, ps.m,                  4UL },
      { "set_first",     at.set_first_at,  4UL, ps.ms+1UL,             4UL },
    };
    uint64_t up = 0UL, tail = 0UL;
    for( int i=0; i<9; i++ ) {
      uint64_t len = arr[i].elem*arr[i].cnt, end = i<6 ? at.in_bytes : at.total;
      if( arr[i].at % arr[i].align ) FAIL( "%s at %lu not aligned to %lu", arr[i].name, (unsigned long)arr[i].at, (unsigned long)arr[i].align );
      if( arr[i].at+len>end ) FAIL( "%s ends at %lu past %lu", arr[i].name, (unsigned long)( arr[i].at+len ), (unsigned long)end );
      if( i>=6 && arr[i].at<at.in_bytes ) FAIL( "%s starts inside the uploaded part", arr[i].name );
      for( int j=0; j<i; j++ )
        if( len && arr[j].cnt && arr[i].at<arr[j].at+arr[j].elem*arr[j].cnt && arr[j].at<arr[i].at+len ) FAIL( "%s overlaps %s", arr[i].name, arr[j].name );
      if( i<6 ) up += len; else tail += len;
    }
    if( up!=at.in_bytes ) FAIL( "in_bytes %lu, the uploaded arrays hold %lu", (unsigned long)at.in_bytes, (unsigned long)up );
    if( at.shred_off_at<at.in_bytes || at.shred_off_at-at.in_bytes>=8UL ) FAIL( "the device-only tail at %lu behind %lu", (unsigned long)at.shred_off_at, (unsigned long)at.in_bytes );
    if( at.total!=at.shred_off_at+tail ) FAIL( "total %lu, the tail holds %lu from %lu", (unsigned long)at.total, (unsigned long)tail, (unsigned long)at.shred_off_at );
    if( ( at.shreds_at & 15UL ) || at.shreds_at<ps.bytes || at.shreds_at-ps.bytes>=16UL ) FAIL( "shreds at %lu behind %lu bytes", (unsigned long)at.shreds_at, (unsigned long)ps.bytes );
    if( at.shred_bytes!=1228UL*ps.m || at.item_bytes!=at.shreds_at+at.shred_bytes ) FAIL( "item bytes %lu", (unsigned long)at.item_bytes );

    uint8_t * items  = malloc( at.item_bytes );
    void *    in_mem = NULL;
    if( !items || posix_memalign( &in_mem, 16UL, at.total ) ) return 2;
    uint8_t * in = in_mem;
    memset( items, FILL, at.item_bytes );
    memset( in, FILL, at.total );
    uint64_t skip = fd_shredder_pass_stage( batches, batch_off, batch_sz, desc, has_keys ? privs : NULL, gs, gh, &ps, &at, items, in );
    if( skip!=ps.q*31840UL ) FAIL( "skip %lu", (unsigned long)skip );

    uint64_t const * h_off = (uint64_t const *)( in + at.off_at );
    uint32_t const * h_sz  = (uint32_t const *)( in + at.sz_at );
    uint64_t pos = 0UL, k = k0;
    for( uint64_t c=ps.b; c<=ps.b1; c++ ) {
      /* [from, to) of batch c: what the pass's sets of it take */
      uint64_t from = 0UL, len = 0UL;
      if( k<k1 && set[k].batch==c ) from = 31840UL*set[k].q;
      for( ; k<k1 && set[k].batch==c; k++ ) len += set[k].bytes;
      uint64_t s = c-ps.b;
      if( !len && batch_sz[c] ) FAIL( "batch %lu is touched and gives no byte", (unsigned long)c );
      if( h_off[s]!=pos ) FAIL( "batch %lu at %lu, not %lu", (unsigned long)c, (unsigned long)h_off[s], (unsigned long)pos );
      if( h_sz[s]!=batch_sz[c] ) FAIL( "batch %lu: sz %u", (unsigned long)c, h_sz[s] );
      if( memcmp( in + at.desc_at + 24UL*s, desc + c, 24UL ) ) FAIL( "batch %lu: descriptor differs", (unsigned long)c );
      if( has_keys && memcmp( in + at.keys_at + 32UL*s, privs + 32UL*c, 32UL ) ) FAIL( "batch %lu: key differs", (unsigned long)c );
      if( pos+len>ps.bytes ) FAIL( "batch %lu ends at %lu", (unsigned long)c, (unsigned long)( pos+len ) );
      if( len && memcmp( items + pos, batches + batch_off[c] + from, len ) ) FAIL( "batch %lu: staged bytes are not [%lu, %lu)", (unsigned long)c, (unsigned long)from, (unsigned long)( from+len ) );
      pos += len;
    }
    if( k!=k1 || pos!=ps.bytes ) FAIL( "%lu bytes staged of %lu", (unsigned long)pos, (unsigned long)ps.bytes );
    if( memcmp( in + at.sfb_at, want_gs + ps.b, 4UL*( nbp+1UL ) ) || memcmp( in + at.hfb_at, want_gh + ps.b, 4UL*( nbp+1UL ) ) ) FAIL( "the prefix slices differ" );
    for( uint64_t i=ps.bytes; i<at.item_bytes; i++ ) if( items[i]!=FILL ) FAIL( "item byte %lu behind the batch bytes written", (unsigned long)i );
    for( uint64_t i=at.in_bytes; i<at.total; i++ ) if( in[i]!=FILL ) FAIL( "in byte %lu of the device-only tail written", (unsigned long)i );

    /* ---- the out block ---- */
    fd_shredder_pass_out_t ot = fd_shredder_pass_out( ps.ms );
    if( ot.roots_at!=0UL || ot.sigs_at!=32UL*ps.ms || ot.codes_at!=96UL*ps.ms || ot.pcodes_at!=97UL*ps.ms || ot.out_bytes!=98UL*ps.ms )
      FAIL( "the out block" );

    /* ---- the copy back, from slots filled as the kernels would: a type byte, and no byte like the caller's ---- */
    uint8_t * slots = items + at.shreds_at;
    uint64_t  last_sz = 0UL;
    for( uint64_t i=0UL; i<ps.m; i++ ) {
      for( uint64_t j=0UL; j<1228UL; j++ ) slots[ 1228UL*i+j ] = (uint8_t)( hash32( (uint32_t)( 1228UL*i+j ) ^ 0x51075U ) & 0x7fU );
      slots[ 1228UL*i+0x40UL ] = (uint8_t)( ( hash32( (uint32_t)( h0+i ) ) & 1U ) ? 0x86U : 0x46U );
      last_sz = ( slots[ 1228UL*i+0x40UL ] & 0xf0 )==0x80 ? 1203UL : 1228UL;
    }
    uint64_t       out_bytes    = STRIDE*( ps.m-1UL ) + last_sz;
    unsigned char * shreds_out  = malloc( out_bytes );
    unsigned int * shred_sz_out = malloc( 4UL*ps.m );
    if( !shreds_out || !shred_sz_out ) return 2;
    memset( shreds_out, FILL, out_bytes );
    fd_shredder_pass_copy_back( slots, ps.m, shreds_out, STRIDE, shred_sz_out );
    for( uint64_t i=0UL; i<ps.m; i++ ) {
      uint64_t sz = ( slots[ 1228UL*i+0x40UL ] & 0xf0 )==0x80 ? 1203UL : 1228UL;
      if( shred_sz_out[i]!=sz ) FAIL( "shred %lu: size %u, not %lu", (unsigned long)i, shred_sz_out[i], (unsigned long)sz );
      if( memcmp( shreds_out + STRIDE*i, slots + 1228UL*i, sz ) ) FAIL( "shred %lu: bytes differ", (unsigned long)i );
      for( uint64_t j=STRIDE*i+sz; j<STRIDE*( i+1UL ) && j<out_bytes; j++ ) if( shreds_out[j]!=FILL ) FAIL( "shred %lu: byte %lu behind it written", (unsigned long)i, (unsigned long)( j-STRIDE*i ) );
    }
    free( shreds_out ); free( shred_sz_out ); free( items ); free( in_mem );
    passes++; sets_cut += ps.ms; shreds_cut += ps.m;
    k0 = k1; h0 += want_m;
  }
  if( k0!=N || h0!=M ) { printf( "%s: the passes end at set %lu of %lu, shred %lu of %lu\n", name, (unsigned long)k0, (unsigned long)N, (unsigned long)h0, (unsigned long)M ); return 1; }
  if( set_first_out[N]!=M ) { printf( "%s: set_first_out ends at %u, not %lu\n", name, set_first_out[N], (unsigned long)M ); return 1; }
  free( batch_off ); free( batches ); free( desc ); free( privs ); free( batch_out ); free( gs ); free( gh ); free( want_gs ); free( want_gh );
  free( set ); free( set_first_out );
  return 0;
}

int
main( void ) {
  static unsigned int sz[ 16384 ];
  uint64_t nb;
#define BOTH( name ) do { if( run( name, nb, sz, 0 ) || run( name, nb, sz, 1 ) ) return 1; } while(0)

  nb = 0UL;
  for( int i=0; i<112; i++ ) sz[ nb++ ] = 63679U;
  sz[ nb++ ] = 700000U;
  sz[ nb++ ] = 63679U; sz[ nb++ ] = 63679U;
  BOTH( "inside" );

  nb = 0UL;
  for( int i=0; i<123; i++ ) sz[ nb++ ] = 63679U;
  BOTH( "front" );

  nb = 0UL;
  sz[ nb++ ] = 0U; sz[ nb++ ] = 0U;
  for( int i=0; i<122; i++ ) sz[ nb++ ] = 63679U;
  sz[ nb++ ] = 0U; sz[ nb++ ] = 0U;
  sz[ nb++ ] = 63679U;
  sz[ nb++ ] = 0U;
  BOTH( "zeros" );

  nb = 0UL;
  for( int i=0; i<911; i++ ) sz[ nb++ ] = 1U;
  BOTH( "tiny" );

  nb = 3UL;
  sz[ 0 ] = 0U; sz[ 1 ] = 0U; sz[ 2 ] = 0U;
  BOTH( "none" );

  /* sizes only: 16,384 x 134,892 sets leave INT32_MAX behind */
  nb = 16384UL;
  for( uint64_t b=0UL; b<nb; b++ ) sz[b] = 0xFFFFFFFFU;
  uint32_t *    gs        = malloc( 4UL*( nb+1UL ) );
  uint32_t *    gh        = malloc( 4UL*( nb+1UL ) );
  signed char * batch_out = malloc( nb );
  uint64_t N, M;
  if( !gs || !gh || !batch_out ) return 2;
  if( !fd_shredder_pass_reserve( sz, nb, gs, gh, batch_out, &N, &M ) ) { printf( "the reservation of 16,384 batches of 0xFFFFFFFF bytes went through\n" ); return 1; }
  free( gs ); free( gh ); free( batch_out );

  printf( "%lu passes, %lu sets, %lu shreds\n", (unsigned long)passes, (unsigned long)sets_cut, (unsigned long)shreds_cut );
  return 0;
}
