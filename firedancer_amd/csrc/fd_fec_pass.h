/* fd_fec_pass.h -- a pass of the host wrappers that work on whole FEC sets
   (fd_ed25519_hip_fec_seal_host, _fec_parity_host, _fec_recover_host;
   DESIGN.md 3a, "A pass by sets"): which sets it takes, how its in block is
   laid out and how its shreds are packed into the item staging.  Plain C11,
   host only, no HIP: the engine (host/fd_ed25519_hip_fronts.c) stages in its
   pinned buffers through here, and tests/fec_pass_main.c runs the same code
   under ASan and UBSan on buffers of exactly the sizes stated here.  Its
   siblings: fd_shredder_pass.h (fd_ed25519_hip_shredder_host) and
   fd_poh_pass.h (fd_ed25519_hip_poh_host, _poh_blocks_host).

   A pass takes whole sets, up to FD_FEC_PASS_CHUNK shreds and as many sets.
   A set whose range runs backwards, leaves [0, n) or holds more than
   FEC_SET_MAX shreds travels as an empty set (fd_fec_core_set_cnt), which is
   the same code.  No rule reads and no kernel writes a byte at or past
   FD_SHRED_MAX_SZ, so a longer shred travels as its head and its true size.

   The item staging, the same on the host and on the device: the shreds that
   travel whole back to back from 0; then, from the next 16-byte boundary,
   the shreds that stand aside in slots FD_SHRED_MAX_SZ bytes apart, of which
   only the first head bytes go up (zero-filled when the shred is shorter).
   The aside slots are what the kernel fills, so that region alone comes down.

     seal      none stands aside
     parity    a code shred (type 0x4?, longer than 0x40 bytes) stands aside
               and sends its first 0x59 bytes: no rule reads a byte at or past
               0x59, and the kernel fills the rest
     recovery  an erased slot stands aside and sends nothing: the kernel reads
               its size alone

   The in block: keys [ms][32] (the seal's private keys, when it has them),
   off u64 [m], set_first u32 [ms+1], sz u32 [m], flags u8 [m] (the
   recovery's erased flags), without padding: from a 16-byte-aligned base
   every array is aligned to what front_begin asks of it. */
#ifndef FD_FEC_PASS_H
#define FD_FEC_PASS_H

#include <stdint.h>
#include <string.h>
#include "fd_fec_core.h"

#define FD_FEC_PASS_CHUNK 16384UL   /* shreds a pass, and sets a pass */

#define FD_FEC_PASS_SEAL    0
#define FD_FEC_PASS_PARITY  1
#define FD_FEC_PASS_RECOVER 2

/* The pass that starts at set k0 < n_set: the sets [k0, *k1) and, returned,
   their shreds as they travel, m <= FD_FEC_PASS_CHUNK, with *k1 - k0 <=
   FD_FEC_PASS_CHUNK.  A set travels as at most FEC_SET_MAX = 134 shreds,
   which always fit, so a pass always advances: *k1 > k0. */
static inline uint64_t
fd_fec_pass_cut( unsigned int const * set_first, uint64_t n_set, uint64_t n, uint64_t k0, uint64_t * k1 ) {
  uint64_t k = k0, m = 0UL;
  for( ; k<n_set && k-k0<FD_FEC_PASS_CHUNK; k++ ) {
    uint64_t cnt = fd_fec_core_set_cnt( set_first[k], set_first[k+1UL], n );
    if( m+cnt>FD_FEC_PASS_CHUNK ) break;
    m += cnt;
  }
  *k1 = k;
  return m;
}

/* the item bytes a pass of m shreds needs at most: m slots, and what the
   16-byte boundary in front of the aside slots may skip */
static inline uint64_t
fd_fec_pass_item_bytes( int front, uint64_t m ) {
  return m*FD_SHRED_CORE_MAX_SZ + ( front==FD_FEC_PASS_SEAL ? 0UL : 16UL );
}

/* the in block of a pass of m shreds in ms sets, as offsets from its base */
typedef struct {
  uint64_t keys_at;    /* [ms][32] when has_keys, else empty */
  uint64_t off_at;     /* u64 [m]: where a shred stands in the item staging */
  uint64_t first_at;   /* u32 [ms+1]: the pass's own set_first, a prefix sum that ends at m */
  uint64_t sz_at;      /* u32 [m]: the true sizes */
  uint64_t flags_at;   /* u8 [m] when has_flags, else empty */
  uint64_t in_bytes;
} fd_fec_pass_in_t;

static inline fd_fec_pass_in_t
fd_fec_pass_in( uint64_t m, uint64_t ms, int has_keys, int has_flags ) {
  fd_fec_pass_in_t at;
  at.keys_at  = 0UL;
  at.off_at   = has_keys ? 32UL*ms : 0UL;
  at.first_at = at.off_at   + 8UL*m;
  at.sz_at    = at.first_at + 4UL*( ms+1UL );
  at.flags_at = at.sz_at    + 4UL*m;
  at.in_bytes = at.flags_at + ( has_flags ? m : 0UL );
  return at;
}

/* where shred j of the pass's set q (set k0 + q of the batch) stands in the item staging */
static inline uint64_t
fd_fec_pass_at( uint8_t const * in, fd_fec_pass_in_t const * at, uint64_t q, uint64_t j ) {
  uint32_t const * first = (uint32_t const *)( in + at->first_at );
  return ( (uint64_t const *)( in + at->off_at ) )[ first[q]+j ];
}

/* whether shred j of the batch, s of sz bytes, stands aside */
static inline int
fd_fec_pass_aside( int front, unsigned char const * s, uint64_t sz, unsigned char const * erased, uint64_t j ) {
  return front==FD_FEC_PASS_PARITY ? ( sz>0x40UL && ( s[ 0x40 ] & 0xf0 )==0x40 ) : front==FD_FEC_PASS_RECOVER ? erased[j]!=0U : 0;
}

typedef struct {
  uint64_t whole;      /* the bytes of the shreds that travel whole: [0, whole) of the staging */
  uint64_t aside_at;   /* whole rounded up to 16: where the aside slots start */
  uint64_t n_aside;    /* slot i is [aside_at + FD_SHRED_MAX_SZ i, + FD_SHRED_MAX_SZ) */
} fd_fec_pass_staged_t;

/* Packs the shreds of the sets [k0, k1) of a pass of m shreds (fd_fec_pass_cut)
   into items, fd_fec_pass_item_bytes( front, m ) bytes, and fills off,
   set_first, sz and, for the recovery, the flags of the in block in, laid out
   as at says (fd_fec_pass_in of m and k1 - k0).  erased is read by the
   recovery alone.  The keys are the caller's to copy. */
static inline fd_fec_pass_staged_t
fd_fec_pass_stage( int front, unsigned char const * shreds, unsigned long const * shred_off, unsigned int const * shred_sz,
                   unsigned char const * erased, uint64_t n, unsigned int const * set_first, uint64_t k0, uint64_t k1,
                   uint8_t * items, uint8_t * in, fd_fec_pass_in_t const * at ) {
  uint64_t * h_off   = (uint64_t *)( in + at->off_at );
  uint32_t * h_first = (uint32_t *)( in + at->first_at );
  uint32_t * h_sz    = (uint32_t *)( in + at->sz_at );
  uint8_t *  h_flags = in + at->flags_at;
  fd_fec_pass_staged_t st = { 0UL, 0UL, 0UL };
  /* the whole shreds first: where they end, the aside slots begin (the seal has none) */
  uint64_t whole = 0UL;
  if( front!=FD_FEC_PASS_SEAL ) {
    for( uint64_t k=k0; k<k1; k++ ) {
      uint64_t first = set_first[k], cnt = fd_fec_core_set_cnt( first, set_first[k+1UL], n );
      for( uint64_t j=first; j<first+cnt; j++ )
        if( !fd_fec_pass_aside( front, shreds + shred_off[j], shred_sz[j], erased, j ) )
          whole += shred_sz[j]<=FD_SHRED_CORE_MAX_SZ ? shred_sz[j] : FD_SHRED_CORE_MAX_SZ;
    }
  }
  uint64_t aside_at = ( whole+15UL ) & ~15UL, pos = 0UL, i = 0UL;
  for( uint64_t k=k0; k<k1; k++ ) {
    uint64_t first = set_first[k], cnt = fd_fec_core_set_cnt( first, set_first[k+1UL], n );
    h_first[ k-k0 ] = (uint32_t)i;
    for( uint64_t j=first; j<first+cnt; j++, i++ ) {
      unsigned char const * s = shreds + shred_off[j];
      uint64_t sz = shred_sz[j];
      h_sz[i] = shred_sz[j];
      if( front==FD_FEC_PASS_RECOVER ) h_flags[i] = erased[j]!=0U;
      if( fd_fec_pass_aside( front, s, sz, erased, j ) ) {
        h_off[i] = aside_at + FD_SHRED_CORE_MAX_SZ*st.n_aside++;
        if( front==FD_FEC_PASS_PARITY ) {   /* the head, zero-filled behind a shred that ends inside it */
          memset( items + h_off[i], 0, FD_SHRED_CORE_CODE_HDR_SZ );
          memcpy( items + h_off[i], s, sz<FD_SHRED_CORE_CODE_HDR_SZ ? sz : FD_SHRED_CORE_CODE_HDR_SZ );
        }
      } else {
        uint64_t cp = sz<=FD_SHRED_CORE_MAX_SZ ? sz : FD_SHRED_CORE_MAX_SZ;
        if( cp ) memcpy( items + pos, s, cp );
        h_off[i] = pos;
        pos += cp;
      }
    }
  }
  st.whole    = pos;
  st.aside_at = ( pos+15UL ) & ~15UL;
  h_first[ k1-k0 ] = (uint32_t)i;
  return st;
}

#endif /* FD_FEC_PASS_H */
