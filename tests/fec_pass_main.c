/* A pass of the FEC-set host wrappers (firedancer_amd/csrc/fd_fec_pass.h): the
   cut, the in block's layout and the staging, on buffers of exactly the sizes
   the header states -- fd_fec_pass_item_bytes of item staging and in_bytes of
   in block -- so that ASan sees any write past them.  Stand-alone, built under
   ASan and UBSan by tests/test_fec_pass.py.

   Three batches, each in the seal's mode without and with keys, the parity's
   and the recovery's:
     mix      sets of 1, 2, .. 134 shreds, then an empty range, a range of 135,
              one that runs backwards, one that leaves [0, n), one that comes
              back from there, and a good set over shreds other sets hold too
     sets     16,385 empty ranges, then one good set of 3: the first pass is
              cut by the set bound
     shreds   130 sets of 134: the shred total crosses 16,384 inside set 122
   Shred j has SIZES[ j % 9 ] bytes and a type byte (0x40) that walks through
   data, code and neither as j / 9 does; slot j is erased as a hash says.

   Prints the passes checked and the shreds staged; exit 1 with the first
   failure. */
#define _POSIX_C_SOURCE 200112L   /* posix_memalign */
#include "fd_ed25519_hip.h"
#include "fd_fec_pass.h"

#include <stdio.h>
#include <stdlib.h>

#define FAIL( ... ) do { printf( "%s mode %d keys %d pass at set %lu: ", name, front, has_keys, (unsigned long)k0 ); \
                         printf( __VA_ARGS__ ); printf( "\n" ); fflush( stdout ); return 1; } while(0)

#define ROOM_BEHIND 64UL   /* what the engine's staging keeps behind the bytes a pass asks for */
#define FILL        0xA5

static unsigned const SIZES[ 9 ] = { 0U, 0x40U, 0x41U, 0x58U, 0x59U, 1203U, 1228U, 1229U, 4000U };

static uint32_t
hash32( uint32_t x ) { x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16; return x; }

typedef struct {
  char const *    name;
  uint64_t        n, n_set;
  unsigned char * shreds;
  unsigned long * off;
  unsigned int *  sz;
  unsigned char * erased;
  unsigned int *  set_first;   /* n_set + 1 */
} batch_t;

/* n shreds packed back to back, their set_first left to the caller */
static int
batch_new( batch_t * b, char const * name, uint64_t n, uint64_t n_set ) {
  b->name = name; b->n = n; b->n_set = n_set;
  uint64_t bytes = 0UL;
  for( uint64_t j=0UL; j<n; j++ ) bytes += SIZES[ j%9UL ];
  b->shreds    = malloc( bytes ? bytes : 1UL );
  b->off       = malloc( sizeof(unsigned long)*( n ? n : 1UL ) );
  b->sz        = malloc( sizeof(unsigned int)*( n ? n : 1UL ) );
  b->erased    = malloc( n ? n : 1UL );
  b->set_first = malloc( sizeof(unsigned int)*( n_set+1UL ) );
  if( !b->shreds || !b->off || !b->sz || !b->erased || !b->set_first ) return 1;
  uint64_t pos = 0UL;
  for( uint64_t j=0UL; j<n; j++ ) {
    static unsigned char const type[ 3 ] = { 0x86, 0x46, 0x66 };
    b->off[j] = pos; b->sz[j] = SIZES[ j%9UL ];
    for( uint64_t q=0UL; q<b->sz[j]; q++ ) b->shreds[ pos+q ] = (unsigned char)( hash32( (uint32_t)( pos+q ) ) | 1U );   /* no zero byte */
    if( b->sz[j]>0x40U ) b->shreds[ pos+0x40UL ] = type[ ( j/9UL )%3UL ];
    b->erased[j] = (unsigned char)( ( hash32( (uint32_t)j ^ 0x5eedU ) & 3U ) ? 0U : 1U + ( j & 1U ) );   /* 0, 1 or 2 */
    pos += b->sz[j];
  }
  return 0;
}

static void
batch_free( batch_t * b ) { free( b->shreds ); free( b->off ); free( b->sz ); free( b->erased ); free( b->set_first ); }

/* the count of a set as it travels, from the public header's words */
static uint64_t
want_cnt( batch_t const * b, uint64_t k ) {
  uint64_t first = b->set_first[k], last = b->set_first[k+1UL];
  if( first>last || last>b->n ) return 0UL;
  return last-first>FD_ED25519_HIP_FEC_SET_MAX ? 0UL : last-first;
}

static uint64_t passes, staged;

static int
run( batch_t const * b, int front, int has_keys ) {
  char const * name = b->name;
  uint64_t k0 = 0UL;
  while( k0<b->n_set ) {
    uint64_t k1 = ~0UL, m = fd_fec_pass_cut( b->set_first, b->n_set, b->n, k0, &k1 ), ms = k1-k0;
    if( k1<=k0 || k1>b->n_set ) FAIL( "the pass ends at set %lu", (unsigned long)k1 );
    if( m>16384UL || ms>16384UL ) FAIL( "%lu shreds, %lu sets", (unsigned long)m, (unsigned long)ms );
    uint64_t want_m = 0UL;
    for( uint64_t k=k0; k<k1; k++ ) want_m += want_cnt( b, k );
    if( m!=want_m ) FAIL( "%lu shreds, its sets have %lu", (unsigned long)m, (unsigned long)want_m );
    /* the cut is greedy: the next set, if any, would break a bound */
    if( k1<b->n_set && ms<16384UL && m+want_cnt( b, k1 )<=16384UL ) FAIL( "set %lu would have fit", (unsigned long)k1 );

    /* ---- the in block ---- */
    fd_fec_pass_in_t at = fd_fec_pass_in( m, ms, has_keys, front==FD_FEC_PASS_RECOVER );
    struct { char const * name; uint64_t at, elem, cnt, align; } arr[ 5 ] = {
      { "keys",      at.keys_at,  32UL, has_keys ? ms : 0UL,                     16UL },
      { "off",       at.off_at,    8UL, m,                                        8UL },
      { "set_first", at.first_at,  4UL, ms+1UL,                                   4UL },
      { "sz",        at.sz_at,     4UL, m,                                        4UL },
      { "flags",     at.flags_at,  1UL, front==FD_FEC_PASS_RECOVER ? m : 0UL,     1UL },
    };
    uint64_t covered = 0UL;
    for( int i=0; i<5; i++ ) {
      uint64_t len = arr[i].elem*arr[i].cnt;
      if( arr[i].at % arr[i].align ) FAIL( "%s at %lu not aligned to %lu", arr[i].name, (unsigned long)arr[i].at, (unsigned long)arr[i].align );
      if( arr[i].at+len>at.in_bytes ) FAIL( "%s ends at %lu past in_bytes %lu", arr[i].name, (unsigned long)( arr[i].at+len ), (unsigned long)at.in_bytes );
      for( int j=0; j<i; j++ )
        if( len && arr[j].cnt && arr[i].at<arr[j].at+arr[j].elem*arr[j].cnt && arr[j].at<arr[i].at+len ) FAIL( "%s overlaps %s", arr[i].name, arr[j].name );
      covered += len;
    }
    if( covered!=at.in_bytes ) FAIL( "in_bytes %lu, the arrays hold %lu", (unsigned long)at.in_bytes, (unsigned long)covered );

    /* ---- the staging, into buffers of exactly the stated sizes ---- */
    uint64_t item_bytes = fd_fec_pass_item_bytes( front, m );
    if( item_bytes!=m*1228UL + ( front==FD_FEC_PASS_SEAL ? 0UL : 16UL ) ) FAIL( "item bytes %lu", (unsigned long)item_bytes );
    uint8_t * items = malloc( item_bytes ? item_bytes : 1UL );
    void *    in_mem = NULL;
    if( !items || posix_memalign( &in_mem, 16UL, at.in_bytes ) ) return 2;
    uint8_t * in = in_mem;
    memset( items, FILL, item_bytes );
    memset( in, FILL, at.in_bytes );
    fd_fec_pass_staged_t sg = fd_fec_pass_stage( front, b->shreds, b->off, b->sz, b->erased, b->n, b->set_first, k0, k1, items, in, &at );

    uint64_t const * h_off   = (uint64_t const *)( in + at.off_at );
    uint32_t const * h_first = (uint32_t const *)( in + at.first_at );
    uint32_t const * h_sz    = (uint32_t const *)( in + at.sz_at );
    uint8_t const *  h_flags = in + at.flags_at;
    for( uint64_t q=0UL; q<32UL*( has_keys ? ms : 0UL ); q++ ) if( in[ at.keys_at+q ]!=FILL ) FAIL( "the keys were written" );
    if( sg.aside_at!=( ( sg.whole+15UL ) & ~15UL ) ) FAIL( "aside slots at %lu behind %lu whole bytes", (unsigned long)sg.aside_at, (unsigned long)sg.whole );
    if( sg.aside_at + 1228UL*sg.n_aside>item_bytes ) FAIL( "the aside slots end past the item bytes" );
    uint64_t pos = 0UL, n_aside = 0UL, i = 0UL;
    for( uint64_t k=k0; k<k1; k++ ) {
      uint64_t first = b->set_first[k], cnt = want_cnt( b, k );
      if( h_first[ k-k0 ]!=i ) FAIL( "set_first[%lu] is %u, not %lu", (unsigned long)( k-k0 ), h_first[ k-k0 ], (unsigned long)i );
      for( uint64_t j=first; j<first+cnt; j++, i++ ) {
        unsigned char const * s = b->shreds + b->off[j];
        uint64_t sz = b->sz[j];
        int aside = front==FD_FEC_PASS_PARITY ? ( sz>0x40UL && ( s[ 0x40 ] & 0xf0 )==0x40 ) : front==FD_FEC_PASS_RECOVER ? b->erased[j]!=0 : 0;
        if( h_sz[i]!=sz ) FAIL( "shred %lu: sz %u, not %lu", (unsigned long)j, h_sz[i], (unsigned long)sz );
        if( front==FD_FEC_PASS_RECOVER && h_flags[i]!=( b->erased[j]!=0 ) ) FAIL( "shred %lu: flag %u", (unsigned long)j, h_flags[i] );
        if( fd_fec_pass_at( in, &at, k-k0, j-first )!=h_off[i] ) FAIL( "shred %lu: fd_fec_pass_at", (unsigned long)j );
        if( !aside ) {
          uint64_t cp = sz<=1228UL ? sz : 1228UL;
          if( h_off[i]!=pos ) FAIL( "whole shred %lu at %lu, not %lu", (unsigned long)j, (unsigned long)h_off[i], (unsigned long)pos );
          if( pos+cp>sg.whole || pos+cp>item_bytes || pos+cp+16UL>item_bytes+ROOM_BEHIND ) FAIL( "whole shred %lu ends at %lu", (unsigned long)j, (unsigned long)( pos+cp ) );
          if( cp && memcmp( items+pos, s, cp ) ) FAIL( "whole shred %lu: staged bytes differ", (unsigned long)j );
          pos += cp;
        } else {
          uint64_t slot = sg.aside_at + 1228UL*n_aside, head = front==FD_FEC_PASS_PARITY ? 0x59UL : 0UL, cp = sz<head ? sz : head;
          if( h_off[i]!=slot || ( sg.aside_at & 15UL ) || sg.aside_at<sg.whole ) FAIL( "aside shred %lu at %lu, not %lu", (unsigned long)j, (unsigned long)h_off[i], (unsigned long)slot );
          if( slot+1228UL>item_bytes || slot+1228UL+16UL>item_bytes+ROOM_BEHIND ) FAIL( "aside shred %lu ends at %lu", (unsigned long)j, (unsigned long)( slot+1228UL ) );
          if( cp && memcmp( items+slot, s, cp ) ) FAIL( "aside shred %lu: head bytes differ", (unsigned long)j );
          for( uint64_t q=cp; q<head; q++ ) if( items[ slot+q ] ) FAIL( "aside shred %lu: byte %lu of the head not zero", (unsigned long)j, (unsigned long)q );
          for( uint64_t q=head; q<1228UL; q++ ) if( items[ slot+q ]!=FILL ) FAIL( "aside shred %lu: byte %lu written", (unsigned long)j, (unsigned long)q );
          n_aside++;
        }
      }
    }
    if( i!=m || h_first[ ms ]!=m ) FAIL( "%lu shreds staged, set_first ends at %u, m %lu", (unsigned long)i, h_first[ ms ], (unsigned long)m );
    if( pos!=sg.whole || n_aside!=sg.n_aside ) FAIL( "whole %lu (%lu), aside %lu (%lu)", (unsigned long)sg.whole, (unsigned long)pos, (unsigned long)sg.n_aside, (unsigned long)n_aside );
    for( uint64_t q=sg.whole; q<sg.aside_at && q<item_bytes; q++ ) if( items[q]!=FILL ) FAIL( "byte %lu between the regions written", (unsigned long)q );
    for( uint64_t q=sg.aside_at + 1228UL*sg.n_aside; q<item_bytes; q++ ) if( items[q]!=FILL ) FAIL( "byte %lu behind the slots written", (unsigned long)q );
    free( items ); free( in_mem );
    passes++; staged += m;
    k0 = k1;
  }
  if( k0!=b->n_set ) { printf( "%s: the passes end at set %lu of %lu\n", name, (unsigned long)k0, (unsigned long)b->n_set ); return 1; }
  return 0;
}

int
main( void ) {
  batch_t b[ 3 ];
  uint64_t k;

  /* mix: 134 good sets, six odd ranges, one more good set */
  uint64_t n_mix = 134UL*135UL/2UL + 140UL;
  if( batch_new( &b[0], "mix", n_mix, 134UL+6UL ) ) return 2;
  unsigned int * f = b[0].set_first;
  f[0] = 0U;
  for( k=1UL; k<=134UL; k++ ) f[k] = f[k-1UL] + (unsigned)k;   /* 1 .. 134 shreds; f[134] = 9045 */
  f[135] = f[134];                  /* empty */
  f[136] = f[135] + 135U;           /* 135 shreds: inside [0, n), one too many */
  f[137] = f[136] - 200U;           /* runs backwards */
  f[138] = (unsigned)n_mix + 7U;    /* leaves [0, n) */
  f[139] = 10U;                     /* comes back: backwards */
  f[140] = 10U + 134U;              /* a good set over shreds 10 .. 143 */

  /* sets: the set bound cuts the first pass */
  if( batch_new( &b[1], "sets", 3UL, 16386UL ) ) return 2;
  for( k=0UL; k<=16385UL; k++ ) b[1].set_first[k] = 0U;
  b[1].set_first[ 16386 ] = 3U;

  /* shreds: the shred bound cuts inside a set */
  if( batch_new( &b[2], "shreds", 134UL*130UL, 130UL ) ) return 2;
  for( k=0UL; k<=130UL; k++ ) b[2].set_first[k] = (unsigned)( 134UL*k );

  for( int i=0; i<3; i++ ) {
    if( run( &b[i], FD_FEC_PASS_SEAL, 0 ) || run( &b[i], FD_FEC_PASS_SEAL, 1 ) ) return 1;
    if( run( &b[i], FD_FEC_PASS_PARITY, 0 ) || run( &b[i], FD_FEC_PASS_RECOVER, 0 ) ) return 1;
  }
  for( int i=0; i<3; i++ ) batch_free( &b[i] );
  printf( "%lu passes, %lu shreds\n", (unsigned long)passes, (unsigned long)staged );
  return 0;
}
