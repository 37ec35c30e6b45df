/* The workspace layout of the FEC seal (front_work_fec,
   firedancer_amd/csrc/fd_front_work.h) against the public
   FD_ED25519_HIP_FEC_WORK_BYTES macro a caller sizes the buffer with.
   Stand-alone, built under ASan and UBSan by tests/test_fec_work.py; only
   pointers are formed, no array is touched.

   Prints the number of layouts checked; exit 1 with the first failure. */
#include "fd_ed25519_hip.h"
#include "fd_front_work.h"

#include <stdio.h>
#include <stdlib.h>

#define BUF_BYTES ( 32UL<<20 )

typedef struct {
  char const * name;
  void const * p;
  uint64_t     elem;     /* bytes an element */
  uint64_t     cnt;
  uint64_t     align;    /* elem, or 16 for the arrays read and written as uint4 */
  uint64_t     want;     /* the offset the public header's description gives */
} arr_t;

static uint8_t * buf;

static int
fec( uint64_t n, uint64_t n_set ) {
# define FAIL( ... ) do { printf( "fec(%lu,%lu): ", (unsigned long)n, (unsigned long)n_set ); printf( __VA_ARGS__ ); \
                          printf( "\n" ); return 1; } while(0)
  front_work_t w;
  uint64_t end = front_work_fec( buf, n, n_set, &w ), public_bytes = FD_ED25519_HIP_FEC_WORK_BYTES( n, n_set );
  arr_t arr[] = {
    { "sigs",    w.sigs,    64UL, n_set, 16UL, 0UL         },
    { "pubs",    w.pubs,    32UL, n_set, 16UL,  64UL*n_set },
    { "roots",   w.roots,   32UL, n_set, 16UL,  96UL*n_set },
    { "msg_off", w.msg_off,  8UL, n_set,  8UL, 128UL*n_set },
    { "msg_sz",  w.msg_sz,   4UL, n_set,  4UL, 136UL*n_set },
    { "set_of",  w.set_of,   4UL, n,      4UL, 140UL*n_set },
  };
  int arr_cnt = (int)( sizeof(arr)/sizeof(arr[0]) );
  if( end>public_bytes ) FAIL( "end %lu past the public %lu", (unsigned long)end, (unsigned long)public_bytes );
  if( public_bytes>BUF_BYTES ) FAIL( "test buffer too small" );
  if( w.msgs || w.codes || w.pre || w.ent_instr || w.status || w.hdr_instr || w.hdr_pos || w.val_sz ) FAIL( "an array of another front" );
  uint64_t last = 0UL;
  for( int i=0; i<arr_cnt; i++ ) {
    uint64_t off = (uint64_t)( (uint8_t const *)arr[i].p - buf ), len = arr[i].elem*arr[i].cnt;
    if( off!=arr[i].want ) FAIL( "%s at %lu, not at %lu", arr[i].name, (unsigned long)off, (unsigned long)arr[i].want );
    if( (uintptr_t)arr[i].p % arr[i].align ) FAIL( "%s at %lu not aligned to %lu", arr[i].name, (unsigned long)off, (unsigned long)arr[i].align );
    if( off+len>end ) FAIL( "%s ends at %lu past the end %lu", arr[i].name, (unsigned long)( off+len ), (unsigned long)end );
    if( off+len>last ) last = off+len;
    for( int j=0; j<i; j++ ) {
      uint64_t o2 = (uint64_t)( (uint8_t const *)arr[j].p - buf ), l2 = arr[j].elem*arr[j].cnt;
      if( off<o2+l2 && o2<off+len ) FAIL( "%s overlaps %s", arr[i].name, arr[j].name );
    }
  }
  if( last!=end ) FAIL( "end %lu, the last array ends at %lu", (unsigned long)end, (unsigned long)last );
  return 0;
# undef FAIL
}

int
main( void ) {
  buf = aligned_alloc( 16UL, BUF_BYTES );
  if( !buf ) return 2;
  uint64_t ns[ 72 ], cases = 0UL;
  for( uint64_t i=0UL; i<68UL; i++ ) ns[i] = i;
  ns[68] = 255UL; ns[69] = 256UL; ns[70] = 257UL; ns[71] = 16384UL;
  for( int i=0; i<72; i++ ) {
    uint64_t n_set = ns[i];
    uint64_t n[ 5 ] = { 0UL, 1UL, n_set, 64UL*n_set + 1UL, FD_ED25519_HIP_FEC_SET_MAX*n_set };
    for( int k=0; k<5; k++, cases++ ) if( fec( n[k], n_set ) ) return 1;
  }
  free( buf );
  printf( "%lu layouts\n", (unsigned long)cases );
  return 0;
}
