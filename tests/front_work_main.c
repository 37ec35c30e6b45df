/* The workspace layouts of the fronts (firedancer_amd/csrc/fd_front_work.h)
   against the public FD_ED25519_HIP_*_WORK_BYTES macros a caller sizes the
   buffer with, and against the byte offsets the engine used before the
   layouts had a header of their own (written out below as they stood in
   fd_ed25519_hip_engine.c, the fronts' file then).  Stand-alone, built under ASan and UBSan by
   tests/test_front_work.py; only pointers are formed, no array is touched.

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
  uint64_t     want;     /* the offset of before */
} arr_t;

static uint8_t * buf;

static int
check( char const * front, uint64_t a, uint64_t b, arr_t const * arr, int arr_cnt, uint64_t end, uint64_t public_bytes ) {
# define FAIL( ... ) do { printf( "%s(%lu,%lu): ", front, (unsigned long)a, (unsigned long)b ); printf( __VA_ARGS__ ); \
                          printf( "\n" ); return 1; } while(0)
  if( end>public_bytes ) FAIL( "end %lu past the public %lu", (unsigned long)end, (unsigned long)public_bytes );
  if( public_bytes>BUF_BYTES ) FAIL( "test buffer too small" );
  uint64_t last = 0UL;
  for( int i=0; i<arr_cnt; i++ ) {
    uint64_t off = (uint64_t)( (uint8_t const *)arr[i].p - buf ), len = arr[i].elem*arr[i].cnt;
    if( off!=arr[i].want ) FAIL( "%s at %lu, was at %lu", arr[i].name, (unsigned long)off, (unsigned long)arr[i].want );
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

static int
precompile( uint64_t ntxn, uint64_t n_ent ) {
  front_work_t w;
  uint64_t end = front_work_precompile( buf, ntxn, n_ent, &w );
  arr_t arr[] = {
    { "sigs",      w.sigs,      64UL, n_ent, 16UL, 0UL                      },
    { "pubs",      w.pubs,      32UL, n_ent, 16UL,  64UL*n_ent              },
    { "msg_off",   w.msg_off,    8UL, n_ent,  8UL,  96UL*n_ent              },
    { "msg_sz",    w.msg_sz,     4UL, n_ent,  4UL, 104UL*n_ent              },
    { "codes",     w.codes,      1UL, n_ent,  1UL, 108UL*n_ent              },
    { "pre",       w.pre,        1UL, n_ent,  1UL, 109UL*n_ent              },
    { "ent_instr", w.ent_instr,  1UL, n_ent,  1UL, 110UL*n_ent              },
    { "status",    w.status,     1UL, ntxn,   1UL, 111UL*n_ent              },
    { "hdr_instr", w.hdr_instr,  1UL, ntxn,   1UL, 111UL*n_ent + ntxn       },
    { "hdr_pos",   w.hdr_pos,    1UL, ntxn,   1UL, 111UL*n_ent + 2UL*ntxn   },
  };
  return check( "precompile", ntxn, n_ent, arr, 10, end, FD_ED25519_HIP_PRECOMPILE_WORK_BYTES( ntxn, n_ent ) );
}

static int
shred( uint64_t n ) {
  front_work_t w;
  uint64_t end = front_work_shred( buf, n, &w );
  arr_t arr[] = {
    { "sigs",    w.sigs,    64UL, n, 16UL, 0UL      },
    { "roots",   w.pubs,   32UL, n, 16UL,  64UL*n  },
    { "msg_off", w.msg_off,  8UL, n,  8UL,  96UL*n  },
    { "msg_sz",  w.msg_sz,   4UL, n,  4UL, 104UL*n  },
    { "codes",   w.codes,    1UL, n,  1UL, 108UL*n  },
    { "pre",     w.pre,      1UL, n,  1UL, 109UL*n  },
  };
  return check( "shred", n, 0UL, arr, 6, end, FD_ED25519_HIP_SHRED_WORK_BYTES( n ) );
}

static int
packet( uint64_t n, uint64_t pkt_bytes ) {
  front_work_t w;
  uint64_t end = front_work_packet( buf, n, pkt_bytes, &w );
  uint64_t mirror = ( pkt_bytes + 31UL ) & ~15UL;
  if( mirror<pkt_bytes+16UL ) { printf( "packet(%lu,%lu): mirror %lu\n", (unsigned long)n, (unsigned long)pkt_bytes, (unsigned long)mirror ); return 1; }
  arr_t arr[] = {
    { "sigs",    w.sigs,    64UL, n,      16UL, 0UL               },
    { "pubs",    w.pubs,    32UL, n,      16UL,  64UL*n           },
    { "msgs",    w.msgs,     1UL, mirror, 16UL,  96UL*n           },
    { "msg_off", w.msg_off,  8UL, n,       8UL,  96UL*n + mirror  },
    { "msg_sz",  w.msg_sz,   4UL, n,       4UL, 104UL*n + mirror  },
    { "codes",   w.codes,    1UL, n,       1UL, 108UL*n + mirror  },
    { "pre",     w.pre,      1UL, n,       1UL, 109UL*n + mirror  },
  };
  return check( "packet", n, pkt_bytes, arr, 7, end, FD_ED25519_HIP_PACKET_WORK_BYTES( n, pkt_bytes ) );
}

int
main( void ) {
  buf = aligned_alloc( 16UL, BUF_BYTES );
  if( !buf ) return 2;
  uint64_t ns[ 72 ], cases = 0UL;
  for( uint64_t i=0UL; i<68UL; i++ ) ns[i] = i;
  ns[68] = 255UL; ns[69] = 256UL; ns[70] = 257UL; ns[71] = 16384UL;
  for( int i=0; i<72; i++ ) {
    uint64_t n = ns[i];
    uint64_t n_ent[ 4 ] = { 0UL, 1UL, n, 8UL*n };
    for( int k=0; k<4; k++, cases++ ) if( precompile( n, n_ent[k] ) ) return 1;
    if( shred( n ) ) return 1;
    cases++;
    for( uint64_t b=0UL; b<=64UL; b++, cases++ ) if( packet( n, b ) ) return 1;
    if( packet( n, 1232UL*n ) ) return 1;
    cases++;
  }
  free( buf );
  printf( "%lu layouts\n", (unsigned long)cases );
  return 0;
}
