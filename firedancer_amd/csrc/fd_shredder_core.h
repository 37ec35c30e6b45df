/* fd_shredder_core.h -- the front of the leader's shred path: how an entry
   batch is cut into FEC sets and what stands in every data shred and every
   parity header before the parity is computed (fd_shredder_init_batch and
   lines 145-221 of fd_shredder_next_fec_set, src/disco/shred/fd_shredder.c,
   with the fd_shredder_count_* arithmetic of fd_shredder.h:116-145),
   restated once and compiled three ways: into the device kernel
   (fd_ed25519_shredder.hip, hipcc), into the host library
   (host/fd_ed25519_hip_fronts.c, gcc: fd_ed25519_hip_shredder_count,
   fd_ed25519_hip_shredder) and into the hostile input test's stand-alone
   program (tests/shredder_walk_main.c, gcc with sanitizers).  The includer
   may define FD_SHRED_FN (the function qualifiers).

   Rules:

     1  a batch of sz > 0 bytes is max( sz, 63679 ) / 31840 sets; every set
        but the last takes 31,840 bytes as 32 data and 32 parity shreds, the
        last the r bytes that remain, 1 <= r <= 63679
     2  the last set's d data shreds:  r <=  9135  max( 1, ceil( r/1015 ) )
                                       r <= 31840  ceil( r/995 )
                                       r <= 62400  ceil( r/975 )
                                       else        ceil( r/955 )
        and its p parity shreds: T[ d ] in the first two branches (the
        protocol's table of 33 numbers below), d in the last two
     3  depth = fd_fec_core_depth( d + p ); a data shred carries up to
        payload = 1115 - 20 depth batch bytes, and for every r the branch
        taken gives ( d-1 ) payload < r <= d payload: only a batch's last data
        shred is short
     4  with D the slot index of the set's first data shred and C that of its
        first parity shred (the batch's data_idx and parity_idx plus the d
        and p of the sets before it, mod 2^32):
        data shred i    [0x40] 0x80 | depth, [0x41] slot u64, [0x49] D + i u32,
                        [0x4d] version u16, [0x4f] D u32, [0x53] parent_off
                        u16, [0x55] flags, [0x56] 0x58 + n u16, n = min( the
                        bytes left, payload ); then the n bytes and zeros up
                        to 1203; flags = reference_tick & 0x3f, on the set's
                        last data shred | 0x40 when the set is the batch's
                        last, | 0x80 when besides block_complete & 1
        parity shred j  [0x40] 0x40 | depth, slot, [0x49] C + j, version, D,
                        [0x53] d u16, [0x55] p u16, [0x57] j u16
     5  a batch descriptor: sz == 0, or bytes that leave the buffer,
        ERR_BATCH; else a reservation of sets and shreds that runs backwards,
        leaves [0, n_set) or [0, n), or is not rule 1-2's counts,
        BAD_RESERVATION */
#ifndef FD_SHREDDER_CORE_H
#define FD_SHREDDER_CORE_H

#include "fd_fec_core.h"

#define FD_SHREDDER_CORE_OK              (  0)
#define FD_SHREDDER_CORE_ERR_BATCH       (-19)
#define FD_SHREDDER_CORE_BAD_RESERVATION (-17)

#define FD_SHREDDER_CORE_SET_BYTES 31840UL   /* a normal set: 32 x 995 */
#define FD_SHREDDER_CORE_SET_SHREDS   64U    /* ... 32 + 32 */

/* fd_ed25519_hip_shredder_batch_t */
typedef struct {
  unsigned long  slot;
  unsigned int   data_idx, parity_idx;
  unsigned short version, parent_off;
  unsigned char  reference_tick, block_complete, pad[ 2 ];
} fd_shredder_core_desc_t;

/* set q of a batch */
typedef struct {
  unsigned long off;         /* its first byte in the batch */
  unsigned      bytes;       /* 31840, or r */
  unsigned      d, p, depth, payload;
  unsigned long shred0;      /* its first shred among the batch's: 64 q */
  unsigned      data_idx;    /* D */
  unsigned      parity_idx;  /* C */
  int           last;        /* the batch's last set */
} fd_shredder_core_plan_t;

/* rule 2: 1 <= r <= 63679 */
FD_SHRED_FN void
fd_shredder_core_split( unsigned long r, unsigned * d_out, unsigned * p_out ) {
  /* parity shreds of a set of d <= 32 data shreds */
  const unsigned char T[ 33 ] = {  0, 17, 18, 19, 19, 20, 21, 21, 22, 23, 23, 24, 24, 25, 25, 26, 26,
                                      26, 27, 27, 28, 28, 29, 29, 29, 30, 30, 31, 31, 31, 32, 32, 32 };
  unsigned d, p;
  if(      r<= 9135UL ) { d = (unsigned)( ( r+1014UL )/1015UL ); if( !d ) d = 1U; p = T[ d ]; }
  else if( r<=31840UL ) { d = (unsigned)( ( r+ 994UL )/ 995UL ); p = T[ d ]; }
  else if( r<=62400UL ) { d = (unsigned)( ( r+ 974UL )/ 975UL ); p = d; }
  else                  { d = (unsigned)( ( r+ 954UL )/ 955UL ); p = d; }
  *d_out = d; *p_out = p;
}

/* rule 1: sz > 0 */
FD_SHRED_FN unsigned long
fd_shredder_core_sets( unsigned long sz ) {
  return ( sz>2UL*FD_SHREDDER_CORE_SET_BYTES-1UL ? sz : 2UL*FD_SHREDDER_CORE_SET_BYTES-1UL ) / FD_SHREDDER_CORE_SET_BYTES;
}

/* the sets, data shreds and parity shreds of a batch; zeros for sz == 0 */
FD_SHRED_FN void
fd_shredder_core_count( unsigned long sz, unsigned long * n_set, unsigned long * n_data, unsigned long * n_parity ) {
  *n_set = 0UL; *n_data = 0UL; *n_parity = 0UL;
  if( !sz ) return;
  unsigned long sets = fd_shredder_core_sets( sz );
  unsigned d, p;
  fd_shredder_core_split( sz - ( sets-1UL )*FD_SHREDDER_CORE_SET_BYTES, &d, &p );
  *n_set = sets; *n_data = 32UL*( sets-1UL ) + d; *n_parity = 32UL*( sets-1UL ) + p;
}

/* set q < fd_shredder_core_sets( sz ) of a batch of sz bytes whose first
   shreds have the slot indices data_idx and parity_idx */
FD_SHRED_FN void
fd_shredder_core_plan( unsigned long sz, unsigned long q, unsigned data_idx, unsigned parity_idx, fd_shredder_core_plan_t * o ) {
  unsigned long sets = fd_shredder_core_sets( sz );
  o->off        = q*FD_SHREDDER_CORE_SET_BYTES;
  o->shred0     = q*FD_SHREDDER_CORE_SET_SHREDS;
  o->data_idx   = data_idx   + (unsigned)( 32UL*q );
  o->parity_idx = parity_idx + (unsigned)( 32UL*q );
  o->last       = q+1UL==sets;
  if( o->last ) { o->bytes = (unsigned)( sz - o->off ); fd_shredder_core_split( o->bytes, &o->d, &o->p ); }
  else          { o->bytes = (unsigned)FD_SHREDDER_CORE_SET_BYTES; o->d = 32U; o->p = 32U; }
  o->depth   = fd_fec_core_depth( o->d + o->p );
  o->payload = 1115U - 20U*o->depth;
}

/* the batch bytes data shred i < d of a set carries */
FD_SHRED_FN unsigned
fd_shredder_core_payload( fd_shredder_core_plan_t const * pl, unsigned i ) {
  unsigned at = i*pl->payload;
  return at>=pl->bytes ? 0U : pl->bytes-at<pl->payload ? pl->bytes-at : pl->payload;
}

FD_SHRED_FN void
fd_shredder_core_put( unsigned char * h, unsigned long v, unsigned bytes ) {
  for( unsigned b=0U; b<bytes; b++ ) h[ b ] = (unsigned char)( v >> ( 8U*b ) );
}

/* what data shred i and parity shred j have in common: h is the shred's bytes from 0x40 on */
FD_SHRED_FN void
fd_shredder_core_common_hdr( unsigned char * h, fd_shredder_core_desc_t const * desc, fd_shredder_core_plan_t const * pl,
                             unsigned type, unsigned idx ) {
  h[ 0 ] = (unsigned char)( type | pl->depth );
  fd_shredder_core_put( h+0x01, desc->slot,     8U );
  fd_shredder_core_put( h+0x09, idx,            4U );
  fd_shredder_core_put( h+0x0d, desc->version,  2U );
  fd_shredder_core_put( h+0x0f, pl->data_idx,   4U );
}

/* rule 4: bytes [0x40, 0x58) of data shred i < d into h[0..0x18) */
FD_SHRED_FN void
fd_shredder_core_data_hdr( unsigned char * h, fd_shredder_core_desc_t const * desc, fd_shredder_core_plan_t const * pl, unsigned i ) {
  unsigned flags = desc->reference_tick & 0x3fU;
  if( ( i+1U==pl->d ) & ( pl->last!=0 ) ) flags |= 0x40U | ( ( desc->block_complete & 1U ) << 7 );
  fd_shredder_core_common_hdr( h, desc, pl, 0x80U, pl->data_idx + i );
  fd_shredder_core_put( h+0x13, desc->parent_off, 2U );
  h[ 0x15 ] = (unsigned char)flags;
  fd_shredder_core_put( h+0x16, FD_SHRED_CORE_DATA_HDR_SZ + fd_shredder_core_payload( pl, i ), 2U );
}

/* ... bytes [0x40, 0x59) of parity shred j < p into h[0..0x19) */
FD_SHRED_FN void
fd_shredder_core_code_hdr( unsigned char * h, fd_shredder_core_desc_t const * desc, fd_shredder_core_plan_t const * pl, unsigned j ) {
  fd_shredder_core_common_hdr( h, desc, pl, 0x40U, pl->parity_idx + j );
  fd_shredder_core_put( h+0x13, pl->d, 2U );
  fd_shredder_core_put( h+0x15, pl->p, 2U );
  fd_shredder_core_put( h+0x17, j,     2U );
}

/* rule 5 for a batch of sz bytes at off of a buffer of buf_sz, with the sets
   [s0, s1) of n_set and the shreds [h0, h1) of n reserved for it */
FD_SHRED_FN int
fd_shredder_core_judge( unsigned long off, unsigned long sz, unsigned long buf_sz, unsigned long s0, unsigned long s1,
                        unsigned long n_set, unsigned long h0, unsigned long h1, unsigned long n ) {
  if( ( sz==0UL ) | ( off>buf_sz ) ) return FD_SHREDDER_CORE_ERR_BATCH;
  if( sz>buf_sz-off ) return FD_SHREDDER_CORE_ERR_BATCH;
  if( ( s0>s1 ) | ( s1>n_set ) | ( h0>h1 ) | ( h1>n ) ) return FD_SHREDDER_CORE_BAD_RESERVATION;
  unsigned long sets, nd, np;
  fd_shredder_core_count( sz, &sets, &nd, &np );
  if( ( s1-s0!=sets ) | ( h1-h0!=nd+np ) ) return FD_SHREDDER_CORE_BAD_RESERVATION;
  return FD_SHREDDER_CORE_OK;
}

/* One batch on a CPU: shred i of the batch, in tree order set by set, is
   written at shreds + shred_off[ i ] -- a data shred's bytes [0, 1203), a
   parity shred's [0, 0x59) and its proof field, the signature and proof
   fields zero, the parity region untouched --, shred_sz[ i ] gets 1203 or
   1228 and set_first[ 0 .. sets ] the sets' first shreds.  ERR_BATCH for
   sz == 0, nothing written. */
FD_SHRED_FN int
fd_shredder_core_batch( unsigned char const * batch, unsigned long sz, fd_shredder_core_desc_t const * desc,
                        unsigned char * shreds, unsigned long const * shred_off, unsigned int * shred_sz,
                        unsigned int * set_first ) {
  if( !sz ) return FD_SHREDDER_CORE_ERR_BATCH;
  unsigned long sets = fd_shredder_core_sets( sz ), at = 0UL;
  for( unsigned long q=0UL; q<sets; q++ ) {
    fd_shredder_core_plan_t pl;
    fd_shredder_core_plan( sz, q, desc->data_idx, desc->parity_idx, &pl );
    set_first[ q ] = (unsigned int)at;
    for( unsigned i=0U; i<pl.d; i++ ) {
      unsigned char * s = shreds + shred_off[ at+i ];
      unsigned n = fd_shredder_core_payload( &pl, i );
      for( unsigned b=0U; b<0x40U; b++ ) s[ b ] = 0U;
      fd_shredder_core_data_hdr( s+0x40, desc, &pl, i );
      for( unsigned b=0U; b<n; b++ ) s[ FD_SHRED_CORE_DATA_HDR_SZ+b ] = batch[ pl.off + (unsigned long)i*pl.payload + b ];
      for( unsigned b=FD_SHRED_CORE_DATA_HDR_SZ+n; b<FD_SHRED_CORE_MIN_SZ; b++ ) s[ b ] = 0U;
      shred_sz[ at+i ] = FD_SHRED_CORE_MIN_SZ;
    }
    for( unsigned j=0U; j<pl.p; j++ ) {
      unsigned char * s = shreds + shred_off[ at+pl.d+j ];
      for( unsigned b=0U; b<0x40U; b++ ) s[ b ] = 0U;
      fd_shredder_core_code_hdr( s+0x40, desc, &pl, j );
      for( unsigned b=FD_SHRED_CORE_MAX_SZ-20U*pl.depth; b<FD_SHRED_CORE_MAX_SZ; b++ ) s[ b ] = 0U;
      shred_sz[ at+pl.d+j ] = FD_SHRED_CORE_MAX_SZ;
    }
    at += pl.d + pl.p;
  }
  set_first[ sets ] = (unsigned int)at;
  return FD_SHREDDER_CORE_OK;
}

#endif
