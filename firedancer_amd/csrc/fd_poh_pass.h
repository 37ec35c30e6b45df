/* fd_poh_pass.h -- a pass of fd_ed25519_hip_poh_host and, through it, of
   fd_ed25519_hip_poh_blocks_host (3a, "A pass by sets"): which
   microblocks travel and in what order, which of them a pass takes, how its
   in and out blocks are laid out, how headers, in states and signatures are
   packed into the item staging and how codes and states find their way back
   to the caller's order.  Plain C11, host only, no HIP, a sibling of
   fd_fec_pass.h and fd_shredder_pass.h: the engine
   (host/fd_ed25519_hip_fronts.c) stages in its pinned buffers through here,
   and tests/poh_pass_main.c runs the same code under ASan and UBSan on
   buffers of exactly the sizes stated here.  It includes fd_poh_core.h for
   the judge; an includer that wants the core's host side too includes what
   that asks for first.

   Judge on the host, order by descending k -- so that the lanes of a wave run
   alike --, then pass by pass: a microblock travels as its header (48), its
   in state (32) and its signatures (64 each), back to back in the item
   staging, 80 m + 64 ns bytes for m microblocks with ns signatures.

   The in block: hdr_off u64 [m], in_off u64 [m], sig_off u64 [ns], sig_first
   u32 [m+1], places in the item staging, without padding.  The out block:
   states [m][32], codes [m]. */
#ifndef FD_POH_PASS_H
#define FD_POH_PASS_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "fd_poh_core.h"

#define FD_POH_PASS_CHUNK 16384UL     /* microblocks a pass */
#define FD_POH_PASS_SIGS  (1UL<<18)   /* signatures a pass: 16 MiB of them (a microblock of more travels alone) */

/* an in_off with this bit set is, when the caller has an `extra` array
   (poh_blocks_host's in_hash), an offset into it, not into buf */
#define FD_POH_PASS_IN_EXTRA (1UL<<63)

typedef struct { uint64_t k; uint32_t idx; } fd_poh_pass_ord_t;

static inline int
fd_poh_pass_ord_cmp( void const * a, void const * b ) {
  fd_poh_pass_ord_t const * x = (fd_poh_pass_ord_t const *)a, * y = (fd_poh_pass_ord_t const *)b;
  if( x->k!=y->k ) return x->k>y->k ? -1 : 1;   /* descending k */
  return x->idx<y->idx ? -1 : x->idx>y->idx;
}

/* where microblock i's in state stands */
static inline unsigned char const *
fd_poh_pass_in_state( unsigned char const * buf, unsigned long const * in_off, unsigned char const * extra, uint64_t i ) {
  return extra && ( in_off[ i ] & FD_POH_PASS_IN_EXTRA ) ? extra + ( in_off[ i ] & ~FD_POH_PASS_IN_EXTRA ) : buf + in_off[ i ];
}

/* The judgement and the order of n < 2^32 microblocks.  One with ERR_PARSE --
   the judge's, or a signature that leaves the buffer -- gets its code in out
   and, with out_hash, a zero state, and does not travel.  The others are
   listed in ord (room for n), an unsupported one with k = 0 (it travels and
   is not hashed), sorted by descending k, then by index.  Returns how many
   travel. */
static inline uint64_t
fd_poh_pass_order( unsigned char const * buf, unsigned long buf_sz, uint64_t n, unsigned long const * hdr_off,
                   unsigned long const * in_off, unsigned int const * sig_first, unsigned long n_sig,
                   unsigned long const * sig_off, unsigned char const * extra, unsigned long hash_cnt_max, signed char * out,
                   unsigned char * out_hash, fd_poh_pass_ord_t * ord ) {
  uint64_t go = 0UL;
  for( uint64_t i=0UL; i<n; i++ ) {
    unsigned long k;
    int mixin, in_extra = extra && ( in_off[ i ] & FD_POH_PASS_IN_EXTRA );
    /* an in state in `extra` is the caller's own: judged as if it stood at the buffer's start */
    int code = fd_poh_core_judge( buf, buf_sz, hdr_off[ i ], in_extra ? 0UL : in_off[ i ], sig_first[ i ], sig_first[ i+1UL ],
                                  n_sig, hash_cnt_max, &k, &mixin );
    if( code!=FD_POH_CORE_ERR_PARSE )
      for( uint64_t j=sig_first[ i ]; j<sig_first[ i+1UL ]; j++ )
        if( !fd_poh_core_inside( sig_off[ j ], 64UL, buf_sz ) ) { code = FD_POH_CORE_ERR_PARSE; break; }
    if( code==FD_POH_CORE_ERR_PARSE ) {
      out[ i ] = (signed char)code;
      if( out_hash ) memset( out_hash + 32UL*i, 0, 32UL );
      continue;
    }
    ord[ go ].k = code ? 0UL : k;
    ord[ go ].idx = (uint32_t)i;
    go++;
  }
  qsort( ord, go, sizeof(fd_poh_pass_ord_t), fd_poh_pass_ord_cmp );
  return go;
}

/* The pass that starts at position a < go of the order: the positions
   [a, returned), at most FD_POH_PASS_CHUNK of them, with *ns signatures.  It
   stops before a microblock that would take it past FD_POH_PASS_SIGS
   signatures, but its first microblock always goes: a pass always advances. */
static inline uint64_t
fd_poh_pass_cut( fd_poh_pass_ord_t const * ord, uint64_t go, unsigned int const * sig_first, uint64_t a, uint64_t * ns ) {
  uint64_t b = a, s = 0UL;
  for( ; b<go && b-a<FD_POH_PASS_CHUNK; b++ ) {
    uint64_t cnt = (uint64_t)sig_first[ ord[ b ].idx+1UL ] - sig_first[ ord[ b ].idx ];
    if( b>a && s+cnt>FD_POH_PASS_SIGS ) break;
    s += cnt;
  }
  *ns = s;
  return b;
}

/* the in and out blocks of a pass of m microblocks with ns signatures, as offsets from their bases */
typedef struct {
  uint64_t hdr_at;       /* u64 [m] */
  uint64_t in_at;        /* u64 [m] */
  uint64_t sig_at;       /* u64 [ns] */
  uint64_t first_at;     /* u32 [m+1]: the pass's own sig_first, a prefix sum that ends at ns */
  uint64_t in_bytes;
  uint64_t item_bytes;   /* 80 m + 64 ns */
  uint64_t states_at;    /* out: [m][32] */
  uint64_t codes_at;     /* out: [m] */
  uint64_t out_bytes;
} fd_poh_pass_blocks_t;

static inline fd_poh_pass_blocks_t
fd_poh_pass_blocks( uint64_t m, uint64_t ns ) {
  fd_poh_pass_blocks_t at;
  at.hdr_at     = 0UL;
  at.in_at      = 8UL*m;
  at.sig_at     = 16UL*m;
  at.first_at   = at.sig_at   + 8UL*ns;
  at.in_bytes   = at.first_at + 4UL*( m+1UL );
  at.item_bytes = ( FD_POH_CORE_HDR_SZ+32UL )*m + 64UL*ns;
  at.states_at  = 0UL;
  at.codes_at   = 32UL*m;
  at.out_bytes  = 33UL*m;
  return at;
}

/* Packs the m microblocks ord[ 0 .. m ) of a pass (the caller passes ord + a)
   into items, at->item_bytes bytes, and fills the in block in, laid out as
   at says (fd_poh_pass_blocks of m and the cut's ns). */
static inline void
fd_poh_pass_stage( unsigned char const * buf, unsigned long const * hdr_off, unsigned long const * in_off,
                   unsigned int const * sig_first, unsigned long const * sig_off, unsigned char const * extra,
                   fd_poh_pass_ord_t const * ord, uint64_t m, fd_poh_pass_blocks_t const * at, uint8_t * items, uint8_t * in ) {
  uint64_t * h_hdr   = (uint64_t *)( in + at->hdr_at );
  uint64_t * h_in    = (uint64_t *)( in + at->in_at );
  uint64_t * h_so    = (uint64_t *)( in + at->sig_at );
  uint32_t * h_first = (uint32_t *)( in + at->first_at );
  uint64_t pos = 0UL, s = 0UL;
  for( uint64_t q=0UL; q<m; q++ ) {
    uint64_t i = ord[ q ].idx;
    memcpy( items + pos, buf + hdr_off[ i ], FD_POH_CORE_HDR_SZ );
    memcpy( items + pos + FD_POH_CORE_HDR_SZ, fd_poh_pass_in_state( buf, in_off, extra, i ), 32UL );
    h_hdr[ q ] = pos; h_in[ q ] = pos + FD_POH_CORE_HDR_SZ; h_first[ q ] = (uint32_t)s;
    pos += FD_POH_CORE_HDR_SZ + 32UL;
    for( uint64_t j=sig_first[ i ]; j<sig_first[ i+1UL ]; j++, s++, pos+=64UL ) {
      memcpy( items + pos, buf + sig_off[ j ], 64UL );
      h_so[ s ] = pos;
    }
  }
  h_first[ m ] = (uint32_t)s;
}

/* the out block's codes and, with out_hash, states to the caller's indices */
static inline void
fd_poh_pass_scatter( fd_poh_pass_ord_t const * ord, uint64_t m, fd_poh_pass_blocks_t const * at, uint8_t const * out_block,
                     signed char * out, unsigned char * out_hash ) {
  for( uint64_t q=0UL; q<m; q++ ) {
    uint64_t i = ord[ q ].idx;
    out[ i ] = (signed char)out_block[ at->codes_at + q ];
    if( out_hash ) memcpy( out_hash + 32UL*i, out_block + at->states_at + 32UL*q, 32UL );
  }
}

#endif /* FD_POH_PASS_H */
