/* A pass of fd_ed25519_hip_poh_host (firedancer_amd/csrc/fd_poh_pass.h): the
   judgement and the order, the cut, the blocks' layout, the staging and the
   scatter, on buffers of exactly the sizes the header states -- n elements of
   order, item_bytes of item staging, in_bytes of in block, out_bytes of out
   block -- so that ASan sees any access past them.  Stand-alone, built under
   ASan and UBSan by tests/test_poh_pass.py.

   Every microblock has a 48-byte header and a 32-byte in state of its own at
   odd addresses of one buffer that ends with its last byte; the signatures
   all point at four places of 64 bytes.  The calls:
     order    48 microblocks of 0 to 3 signatures whose k ties, with headers
              and signature places that leave the buffer and hash counts over
              the bound among them, the in state of every third in `extra`;
              once more without `extra`, where the marked offsets leave the
              buffer, and once without out_hash
     blocks   16,385 microblocks without signatures: the microblock bound
     close    2^18 - 1, 1 and 1 signatures: the signature bound closes the
              pass between the last two
     exact    1, 2^18 and 1 signatures in this order of k
     over     1, 2^18 + 1 and 1: the large one travels alone
   What should travel, in what order and in which pass is worked out here
   from the public header's words.

   Prints the passes checked, the microblocks that travelled and the
   signatures staged; exit 1 with the first failure. */
#define _POSIX_C_SOURCE 200112L   /* posix_memalign */
#define FD_POH_CORE_NO_HOST 1     /* the judge alone */
#include "fd_ed25519_hip.h"
#include "fd_poh_pass.h"

#include <stdio.h>

#define FAIL( ... ) do { printf( "%s extra %d pass at %lu: ", name, with_extra, (unsigned long)a ); \
                         printf( __VA_ARGS__ ); printf( "\n" ); fflush( stdout ); return 1; } while(0)

#define FILL    0xA5
#define HDR_OUT 1U   /* the header leaves the buffer */
#define SIG_OUT 2U   /* the microblock's last signature leaves the buffer */
#define EXTRA   4U   /* the in state stands in `extra` */

typedef struct { uint64_t hash_cnt; uint32_t sigs, flags; } spec_t;

static uint32_t
hash32( uint32_t x ) { x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16; return x; }

static void
put64( unsigned char * p, uint64_t v ) { for( int i=0; i<8; i++ ) p[i] = (unsigned char)( v >> ( 8*i ) ); }

/* what the scatter should bring to microblock i */
static signed char   want_code ( uint64_t i )             { return (signed char)( 1U + ( hash32( (uint32_t)i ) & 63U ) ); }
static unsigned char want_state( uint64_t i, uint64_t j ) { return (unsigned char)hash32( (uint32_t)( 32UL*i+j ) ^ 0x57a7eU ); }

static uint64_t passes, travelled, staged;

static int
run( char const * name, uint64_t n, spec_t const * spec, unsigned long hash_cnt_max, int with_extra, int with_hash ) {
  uint64_t a = 0UL;

  /* ---- the caller's arrays ---- */
  uint64_t n_sig = 0UL;
  for( uint64_t i=0UL; i<n; i++ ) n_sig += spec[i].sigs;
  uint64_t hdr_at = 5UL, in_at = hdr_at + 48UL*n, pool_at = in_at + 32UL*n + 3UL, buf_sz = pool_at + 4UL*64UL;
  unsigned char * buf       = malloc( buf_sz );
  unsigned char * extra     = malloc( 32UL*n );
  unsigned long * hdr_off   = malloc( 8UL*n );
  unsigned long * in_off    = malloc( 8UL*n );
  unsigned int *  sig_first = malloc( 4UL*( n+1UL ) );
  unsigned long * sig_off   = malloc( 8UL*( n_sig ? n_sig : 1UL ) );
  signed char *   out       = malloc( n );
  unsigned char * out_hash  = malloc( 32UL*n );
  signed char *   want      = malloc( n );      /* ERR_PARSE, or 0: it travels */
  uint64_t *      want_k    = malloc( 8UL*n );
  fd_poh_pass_ord_t * ord   = malloc( sizeof(fd_poh_pass_ord_t)*n );
  fd_poh_pass_ord_t * wantord   = malloc( sizeof(fd_poh_pass_ord_t)*n );
  if( !buf || !extra || !hdr_off || !in_off || !sig_first || !sig_off || !out || !out_hash || !want || !want_k || !ord || !wantord ) return 2;
  for( uint64_t i=0UL; i<buf_sz; i++ ) buf[i] = (unsigned char)( hash32( (uint32_t)i ) | 1U );
  for( uint64_t i=0UL; i<32UL*n; i++ ) extra[i] = (unsigned char)( hash32( (uint32_t)i ^ 0xe87aU ) & 0xfeU );
  memset( out, FILL, n ); memset( out_hash, FILL, 32UL*n );
  uint64_t s = 0UL, go_want = 0UL;
  for( uint64_t i=0UL; i<n; i++ ) {
    int in_extra = ( spec[i].flags & EXTRA )!=0U;
    uint64_t txn_cnt = spec[i].sigs ? 2UL : 0UL;
    put64( buf + hdr_at + 48UL*i,         spec[i].hash_cnt );
    put64( buf + hdr_at + 48UL*i + 40UL,  txn_cnt );
    hdr_off[i]   = ( spec[i].flags & HDR_OUT ) ? buf_sz-47UL : hdr_at + 48UL*i;
    in_off[i]    = in_extra ? FD_POH_PASS_IN_EXTRA | ( 32UL*i ) : in_at + 32UL*i;
    sig_first[i] = (unsigned int)s;
    for( uint64_t j=0UL; j<spec[i].sigs; j++, s++ ) sig_off[s] = pool_at + 64UL*( s&3UL );
    if( ( spec[i].flags & SIG_OUT ) && spec[i].sigs ) sig_off[ s-1UL ] = buf_sz-63UL;
    /* the public header's rule 6, and the k of rules 1 and 2; over the bound it travels and is not hashed */
    int parse = ( spec[i].flags & HDR_OUT ) || ( ( spec[i].flags & SIG_OUT ) && spec[i].sigs ) || ( in_extra && !with_extra );
    uint64_t k = txn_cnt ? ( spec[i].hash_cnt ? spec[i].hash_cnt-1UL : 0UL ) : spec[i].hash_cnt;
    want[i]   = (signed char)( parse ? FD_ED25519_HIP_POH_ERR_PARSE : 0 );
    want_k[i] = k>hash_cnt_max ? 0UL : k;
    if( !parse ) go_want++;
  }
  sig_first[n] = (unsigned int)s;

  /* ---- the judgement and the order: descending k, then the index (a selection sort of what travels) ---- */
  uint64_t go = fd_poh_pass_order( buf, buf_sz, n, hdr_off, in_off, sig_first, n_sig, sig_off, with_extra ? extra : NULL, hash_cnt_max,
                                   out, with_hash ? out_hash : NULL, ord );
  if( go!=go_want ) FAIL( "%lu travel, not %lu", (unsigned long)go, (unsigned long)go_want );
  for( uint64_t i=0UL; i<n; i++ ) {
    if( out[i]!=( want[i] ? want[i] : (signed char)FILL ) ) FAIL( "microblock %lu judged %d", (unsigned long)i, out[i] );
    for( uint64_t j=0UL; j<32UL; j++ )
      if( out_hash[ 32UL*i+j ]!=( want[i] && with_hash ? 0 : FILL ) ) FAIL( "microblock %lu: state byte %lu after the judgement", (unsigned long)i, (unsigned long)j );
  }
  uint64_t ne = 0UL;
  for( uint64_t i=0UL; i<n; i++ ) if( !want[i] ) { wantord[ne].k = want_k[i]; wantord[ne].idx = (uint32_t)i; ne++; }
  if( n<=64UL ) {
    for( uint64_t x=0UL; x<ne; x++ ) {
      uint64_t best = x;
      for( uint64_t y=x+1UL; y<ne; y++ ) if( wantord[y].k>wantord[best].k || ( wantord[y].k==wantord[best].k && wantord[y].idx<wantord[best].idx ) ) best = y;
      fd_poh_pass_ord_t t = wantord[x]; wantord[x] = wantord[best]; wantord[best] = t;
    }
    for( uint64_t x=0UL; x<go; x++ ) if( ord[x].k!=wantord[x].k || ord[x].idx!=wantord[x].idx ) FAIL( "place %lu of the order holds %u", (unsigned long)x, ord[x].idx );
  } else {   /* a large call: it is ordered, and every traveller is in it once (below: every one gets its own code) */
    for( uint64_t x=0UL; x<go; x++ ) {
      if( ord[x].idx>=n || want[ ord[x].idx ] || ord[x].k!=want_k[ ord[x].idx ] ) FAIL( "place %lu of the order holds %u", (unsigned long)x, ord[x].idx );
      if( x && ( ord[x-1UL].k<ord[x].k || ( ord[x-1UL].k==ord[x].k && ord[x-1UL].idx>=ord[x].idx ) ) ) FAIL( "places %lu and %lu out of order", (unsigned long)( x-1UL ), (unsigned long)x );
    }
  }

  while( a<go ) {
    /* ---- the cut: it advances, keeps both bounds and is greedy ---- */
    uint64_t ns = ~0UL, b = fd_poh_pass_cut( ord, go, sig_first, a, &ns ), m = b-a, want_ns = 0UL;
    if( b<=a || b>go ) FAIL( "the pass ends at %lu", (unsigned long)b );
    for( uint64_t x=a; x<b; x++ ) want_ns += spec[ ord[x].idx ].sigs;
    if( ns!=want_ns ) FAIL( "%lu signatures, its microblocks have %lu", (unsigned long)ns, (unsigned long)want_ns );
    if( m>16384UL ) FAIL( "%lu microblocks", (unsigned long)m );
    if( ns>( 1UL<<18 ) && m!=1UL ) FAIL( "%lu signatures in %lu microblocks", (unsigned long)ns, (unsigned long)m );
    if( b<go && m<16384UL && ns+spec[ ord[b].idx ].sigs<=( 1UL<<18 ) ) FAIL( "the microblock at %lu would have fit", (unsigned long)b );

    /* ---- the blocks ---- */
    fd_poh_pass_blocks_t at = fd_poh_pass_blocks( m, ns );
    struct { char const * name; uint64_t at, elem, cnt; } arr[ 4 ] = {
      { "hdr_off",   at.hdr_at,   8UL, m      },
      { "in_off",    at.in_at,    8UL, m      },
      { "sig_off",   at.sig_at,   8UL, ns     },
      { "sig_first", at.first_at, 4UL, m+1UL  },
    };
    uint64_t covered = 0UL;
    for( int i=0; i<4; i++ ) {
      uint64_t len = arr[i].elem*arr[i].cnt;
      if( arr[i].at % arr[i].elem ) FAIL( "%s at %lu not aligned", arr[i].name, (unsigned long)arr[i].at );
      if( arr[i].at+len>at.in_bytes ) FAIL( "%s ends past in_bytes", arr[i].name );
      for( int j=0; j<i; j++ )
        if( len && arr[j].cnt && arr[i].at<arr[j].at+arr[j].elem*arr[j].cnt && arr[j].at<arr[i].at+len ) FAIL( "%s overlaps %s", arr[i].name, arr[j].name );
      covered += len;
    }
    if( covered!=at.in_bytes ) FAIL( "in_bytes %lu, the arrays hold %lu", (unsigned long)at.in_bytes, (unsigned long)covered );
    if( at.item_bytes!=80UL*m + 64UL*ns ) FAIL( "item bytes %lu", (unsigned long)at.item_bytes );
    if( at.states_at!=0UL || at.codes_at!=32UL*m || at.out_bytes!=33UL*m ) FAIL( "the out block" );

    /* ---- the staging: every byte ---- */
    uint8_t * items  = malloc( at.item_bytes );
    void *    in_mem = NULL;
    if( !items || posix_memalign( &in_mem, 16UL, at.in_bytes ) ) return 2;
    uint8_t * in = in_mem;
    memset( items, FILL, at.item_bytes ); memset( in, FILL, at.in_bytes );
    fd_poh_pass_stage( buf, hdr_off, in_off, sig_first, sig_off, with_extra ? extra : NULL, ord+a, m, &at, items, in );
    uint64_t const * h_hdr   = (uint64_t const *)( in + at.hdr_at );
    uint64_t const * h_in    = (uint64_t const *)( in + at.in_at );
    uint64_t const * h_so    = (uint64_t const *)( in + at.sig_at );
    uint32_t const * h_first = (uint32_t const *)( in + at.first_at );
    uint64_t pos = 0UL, t = 0UL;
    for( uint64_t q=0UL; q<m; q++ ) {
      uint64_t i = ord[ a+q ].idx;
      unsigned char const * state = ( spec[i].flags & EXTRA ) ? extra + 32UL*i : buf + in_at + 32UL*i;
      if( h_hdr[q]!=pos || h_in[q]!=pos+48UL || h_first[q]!=t ) FAIL( "microblock %lu: header at %lu, state at %lu, signatures from %u", (unsigned long)i, (unsigned long)h_hdr[q], (unsigned long)h_in[q], h_first[q] );
      if( pos+80UL+64UL*spec[i].sigs>at.item_bytes ) FAIL( "microblock %lu ends past the item bytes", (unsigned long)i );
      if( memcmp( items+pos, buf + hdr_at + 48UL*i, 48UL ) ) FAIL( "microblock %lu: header bytes differ", (unsigned long)i );
      if( memcmp( items+pos+48UL, state, 32UL ) ) FAIL( "microblock %lu: in state differs", (unsigned long)i );
      pos += 80UL;
      for( uint64_t j=sig_first[i]; j<sig_first[i+1UL]; j++, t++, pos+=64UL ) {
        if( h_so[t]!=pos ) FAIL( "microblock %lu: signature %lu at %lu", (unsigned long)i, (unsigned long)j, (unsigned long)h_so[t] );
        if( memcmp( items+pos, buf + sig_off[j], 64UL ) ) FAIL( "microblock %lu: signature %lu differs", (unsigned long)i, (unsigned long)j );
      }
    }
    if( pos!=at.item_bytes || t!=ns || h_first[m]!=ns ) FAIL( "%lu bytes and %lu signatures staged, sig_first ends at %u", (unsigned long)pos, (unsigned long)t, h_first[m] );

    /* ---- the scatter, from an out block filled as the kernels would ---- */
    uint8_t * ob = malloc( at.out_bytes );
    if( !ob ) return 2;
    for( uint64_t q=0UL; q<m; q++ ) {
      uint64_t i = ord[ a+q ].idx;
      ob[ at.codes_at+q ] = (uint8_t)want_code( i );
      for( uint64_t j=0UL; j<32UL; j++ ) ob[ at.states_at+32UL*q+j ] = want_state( i, j );
    }
    fd_poh_pass_scatter( ord+a, m, &at, ob, out, with_hash ? out_hash : NULL );
    free( ob ); free( items ); free( in_mem );
    passes++; travelled += m; staged += ns;
    a = b;
  }

  /* ---- codes and states at the caller's indices ---- */
  for( uint64_t i=0UL; i<n; i++ ) {
    if( out[i]!=( want[i] ? want[i] : want_code( i ) ) ) FAIL( "microblock %lu came back with %d", (unsigned long)i, out[i] );
    for( uint64_t j=0UL; j<32UL; j++ )
      if( out_hash[ 32UL*i+j ]!=( !with_hash ? FILL : want[i] ? 0 : want_state( i, j ) ) ) FAIL( "microblock %lu: state byte %lu came back wrong", (unsigned long)i, (unsigned long)j );
  }
  free( buf ); free( extra ); free( hdr_off ); free( in_off ); free( sig_first ); free( sig_off ); free( out ); free( out_hash );
  free( want ); free( want_k ); free( ord ); free( wantord );
  return 0;
}

int
main( void ) {
  static spec_t spec[ 16385 ];

  /* order: tests/test_poh_pass.py has the same table */
  static uint32_t const SIGS[ 5 ] = { 0U, 1U, 3U, 0U, 2U };
  static uint64_t const CNT [ 6 ] = { 7UL, 3UL, 7UL, 0UL, 12UL, 3UL };
  for( uint64_t i=0UL; i<48UL; i++ ) {
    spec[i].sigs     = SIGS[ i%5UL ];
    spec[i].hash_cnt = i%7UL==2UL ? 1000UL : CNT[ i%6UL ];   /* over the bound of 100 */
    spec[i].flags    = ( i%11UL==4UL ? HDR_OUT : 0U ) | ( i%13UL==6UL ? SIG_OUT : 0U ) | ( i%3UL==0UL ? EXTRA : 0U );
  }
  if( run( "order", 48UL, spec, 100UL, 1, 1 ) || run( "order", 48UL, spec, 100UL, 0, 1 ) || run( "order", 48UL, spec, 100UL, 1, 0 ) ) return 1;

  for( uint64_t i=0UL; i<16385UL; i++ ) { spec[i].sigs = 0U; spec[i].hash_cnt = i%3UL; spec[i].flags = ( i&1UL ) ? EXTRA : 0U; }
  if( run( "blocks", 16385UL, spec, 100UL, 1, 1 ) ) return 1;

  for( uint64_t i=0UL; i<3UL; i++ ) { spec[i].hash_cnt = 9UL-i; spec[i].flags = 0U; }   /* k falls: the order is the index */
  spec[0].sigs = ( 1U<<18 )-1U; spec[1].sigs = 1U; spec[2].sigs = 1U;
  if( run( "close", 3UL, spec, 100UL, 0, 1 ) ) return 1;
  spec[0].sigs = 1U; spec[1].sigs = 1U<<18; spec[2].sigs = 1U;
  if( run( "exact", 3UL, spec, 100UL, 0, 1 ) ) return 1;
  spec[0].sigs = 1U; spec[1].sigs = ( 1U<<18 )+1U; spec[2].sigs = 1U;
  if( run( "over", 3UL, spec, 100UL, 0, 1 ) ) return 1;

  printf( "%lu passes, %lu microblocks, %lu signatures\n", (unsigned long)passes, (unsigned long)travelled, (unsigned long)staged );
  return 0;
}
