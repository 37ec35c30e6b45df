/* fd_shredder_pass.h -- a pass of fd_ed25519_hip_shredder_host (DESIGN.md 3a,
   "A pass by sets"; 3a10): the reservation the call makes, which sets a pass
   takes, how its in and out blocks are laid out, how the batch bytes are
   packed into the item staging and how the finished shreds go back to the
   caller.  Plain C11, host only, no HIP, a sibling of fd_fec_pass.h and
   fd_poh_pass.h: the engine (host/fd_ed25519_hip_fronts.c) stages in its
   pinned buffers through here, and tests/shredder_pass_main.c runs the same
   code under ASan and UBSan on buffers of exactly the sizes stated here.

   Pass by pass, cut at set boundaries as fd_fec_pass.h cuts (up to
   FD_FEC_PASS_CHUNK shreds and as many sets): a pass is a range of the
   call's sets, and the batches it touches go up as the bytes its sets take --
   the first from where the pass before stopped in it (the launch's skip), the
   last up to where this pass stops.  A batch of no bytes has no set; one that
   stands between two touched batches travels as its descriptor and size 0.

   The item staging, the same on the host and on the device: the batch bytes
   back to back from 0; then, from the next 16-byte boundary (shreds_at), the
   pass's m shreds in slots FD_SHRED_MAX_SZ apart, which the kernels fill and
   which alone come down.

   The in block: keys [nbp][32] (with privs), batch_off u64 [nbp], desc
   [nbp] (24 bytes each), set_first_b u32 [nbp+1], shred_first_b u32 [nbp+1],
   batch_sz u32 [nbp] -- in_bytes so far, which go up -- and, device only,
   from the next 8-byte boundary shred_off u64 [m], shred_sz u32 [m],
   set_first u32 [ms+1], which the kernel writes and the parity and the seal
   read.  From a 16-byte-aligned base every array is aligned to its elements
   and the keys to what the seal asks.  set_first_b and shred_first_b are the
   call's own prefix arrays from batch b on: the launch is told the call's
   totals and where in them the pass lies (set0, shred0).

   The out block: roots [ms][32], sigs [ms][64], the seal's codes [ms], the
   parity's codes [ms]. */
#ifndef FD_SHREDDER_PASS_H
#define FD_SHREDDER_PASS_H

#include <stdint.h>
#include <string.h>
#include "fd_shredder_core.h"
#include "fd_fec_pass.h"   /* FD_FEC_PASS_CHUNK */

/* The reservation: batch b's sets [set_first_b[b], set_first_b[b+1]) and
   shreds [shred_first_b[b], shred_first_b[b+1]) of the call (nb+1 elements
   each), the totals *n_set and *n, and batch_out[b]: OK, or ERR_BATCH for a
   batch of no bytes, which takes neither.  Returns 0, or -1 when the call
   has more than INT32_MAX sets or UINT32_MAX shreds. */
static inline int
fd_shredder_pass_reserve( unsigned int const * batch_sz, uint64_t nb, uint32_t * set_first_b, uint32_t * shred_first_b,
                          signed char * batch_out, uint64_t * n_set, uint64_t * n ) {
  uint64_t N = 0UL, M = 0UL;
  for( uint64_t b=0UL; b<nb; b++ ) {
    unsigned long sets, nd, np;
    fd_shredder_core_count( batch_sz[b], &sets, &nd, &np );
    batch_out[b] = (signed char)( batch_sz[b] ? FD_SHREDDER_CORE_OK : FD_SHREDDER_CORE_ERR_BATCH );
    set_first_b[b] = (uint32_t)N; shred_first_b[b] = (uint32_t)M;
    N += sets; M += nd + np;
    if( N>INT32_MAX || M>UINT32_MAX ) return -1;
  }
  set_first_b[nb] = (uint32_t)N; shred_first_b[nb] = (uint32_t)M;
  *n_set = N; *n = M;
  return 0;
}

/* the next set to shred: set q of batch b, which is set k and shred h of the call.  A call starts at all zeros */
typedef struct { uint64_t b, q, k, h; } fd_shredder_pass_cur_t;

typedef struct {
  uint64_t b, q, k, h;    /* where it starts: the cursor, behind the batches of no bytes in front of it */
  uint64_t b1, q1;        /* the last batch it takes a set of, and the sets of that batch taken when it ends: q1 >= 1 */
  uint64_t nbp;           /* the batches it touches, [b, b1]: b1 - b + 1 */
  uint64_t ms, m, bytes;  /* its sets, their shreds and the batch bytes they take */
} fd_shredder_pass_t;

/* The pass from *cur on, k < n_set: its sets [k, k+ms), ms <=
   FD_FEC_PASS_CHUNK, with m <= FD_FEC_PASS_CHUNK shreds, greedily.  Writes
   set_first_out[ k+1 .. k+ms ], the sets' ends among the call's shreds, and
   moves *cur behind the pass.  A set has at most FEC_SET_MAX = 134 shreds,
   which always fit, so a pass always advances; it has at least 18 (one data
   shred and T[1] = 17 parity shreds), so the bound on the sets, kept as
   fd_fec_pass_cut has it, is never the one that cuts here. */
static inline fd_shredder_pass_t
fd_shredder_pass_cut( unsigned int const * batch_sz, uint32_t const * set_first_b, uint64_t n_set, fd_shredder_pass_cur_t * cur,
                      unsigned int * set_first_out ) {
  fd_shredder_pass_t ps = { 0 };
  uint64_t b = cur->b, q = cur->q;
  while( !batch_sz[b] ) b++;   /* q is 0 in front of them */
  ps.b = b; ps.q = q; ps.k = cur->k; ps.h = cur->h;
  for( ; ps.k+ps.ms<n_set && ps.ms<FD_FEC_PASS_CHUNK; q++ ) {
    while( q==(uint64_t)set_first_b[b+1UL]-set_first_b[b] ) { b++; q = 0UL; }   /* the next batch that has a set left */
    fd_shredder_core_plan_t pl;
    fd_shredder_core_plan( batch_sz[b], q, 0U, 0U, &pl );
    if( ps.m+pl.d+pl.p>FD_FEC_PASS_CHUNK ) break;   /* before a batch too: the pass ends where it took its last set */
    ps.m += pl.d+pl.p; ps.bytes += pl.bytes; ps.ms++;
    ps.b1 = b; ps.q1 = q+1UL;
    set_first_out[ ps.k+ps.ms ] = (unsigned int)( ps.h+ps.m );
  }
  ps.nbp = ps.b1-ps.b+1UL;
  cur->k = ps.k+ps.ms; cur->h = ps.h+ps.m;
  if( ps.q1<(uint64_t)set_first_b[ps.b1+1UL]-set_first_b[ps.b1] ) { cur->b = ps.b1;     cur->q = ps.q1; }
  else                                                            { cur->b = ps.b1+1UL; cur->q = 0UL;   }
  return ps;
}

/* the in block of a pass, as offsets from its base, and its place in the item staging */
typedef struct {
  uint64_t keys_at;        /* [nbp][32] when has_keys, else empty */
  uint64_t off_at;         /* u64 [nbp]: where a batch's staged bytes stand in the item staging */
  uint64_t desc_at;        /* [nbp][24] */
  uint64_t sfb_at;         /* u32 [nbp+1]: set_first_b from batch b on */
  uint64_t hfb_at;         /* u32 [nbp+1]: shred_first_b from batch b on */
  uint64_t sz_at;          /* u32 [nbp]: the true sizes */
  uint64_t in_bytes;       /* what goes up: [0, in_bytes) */
  uint64_t shred_off_at;   /* device only, on the next 8-byte boundary: u64 [m] */
  uint64_t shred_sz_at;    /* u32 [m] */
  uint64_t set_first_at;   /* u32 [ms+1] */
  uint64_t total;          /* the in block's room, the device-only tail included */
  uint64_t shreds_at;      /* the item staging: the batch bytes [0, bytes), the shreds from here on */
  uint64_t shred_bytes;    /* FD_SHRED_MAX_SZ m: what comes down */
  uint64_t item_bytes;     /* shreds_at + shred_bytes */
} fd_shredder_pass_in_t;

static inline fd_shredder_pass_in_t
fd_shredder_pass_in( fd_shredder_pass_t const * ps, int has_keys ) {
  fd_shredder_pass_in_t at;
  uint64_t nbp = ps->nbp;
  at.keys_at      = 0UL;
  at.off_at       = has_keys ? 32UL*nbp : 0UL;
  at.desc_at      = at.off_at  + 8UL*nbp;
  at.sfb_at       = at.desc_at + sizeof(fd_shredder_core_desc_t)*nbp;
  at.hfb_at       = at.sfb_at  + 4UL*( nbp+1UL );
  at.sz_at        = at.hfb_at  + 4UL*( nbp+1UL );
  at.in_bytes     = at.sz_at   + 4UL*nbp;
  at.shred_off_at = ( at.in_bytes+7UL ) & ~7UL;
  at.shred_sz_at  = at.shred_off_at + 8UL*ps->m;
  at.set_first_at = at.shred_sz_at  + 4UL*ps->m;
  at.total        = at.set_first_at + 4UL*( ps->ms+1UL );
  at.shreds_at    = ( ps->bytes+15UL ) & ~15UL;
  at.shred_bytes  = FD_SHRED_CORE_MAX_SZ*ps->m;
  at.item_bytes   = at.shreds_at + at.shred_bytes;
  return at;
}

/* Packs the bytes the pass's sets take of the batches [b, b1] into items
   ([0, ps->bytes) of it) and fills the uploaded part of the in block in, laid
   out as at says: slot c - b has batch c's place, true size, descriptor and,
   with privs, key, and the two prefix arrays are the call's from b on.
   Returns the skip the launch is given (with skip_b 0): the bytes of batch b
   that passes before this one took, which the staged copy leaves out. */
static inline uint64_t
fd_shredder_pass_stage( unsigned char const * batches, unsigned long const * batch_off, unsigned int const * batch_sz,
                        fd_shredder_core_desc_t const * desc, unsigned char const * privs, uint32_t const * set_first_b,
                        uint32_t const * shred_first_b, fd_shredder_pass_t const * ps, fd_shredder_pass_in_t const * at,
                        uint8_t * items, uint8_t * in ) {
  uint64_t * h_off = (uint64_t *)( in + at->off_at );
  uint32_t * h_sz  = (uint32_t *)( in + at->sz_at );
  uint64_t   skip  = ps->q*FD_SHREDDER_CORE_SET_BYTES, pos = 0UL;
  for( uint64_t c=ps->b; c<=ps->b1; c++ ) {
    /* a batch's last set ends with the batch, every other after 31,840 bytes */
    uint64_t from = c==ps->b ? skip : 0UL;
    uint64_t to   = ( c==ps->b1 && ps->q1<(uint64_t)set_first_b[c+1UL]-set_first_b[c] ) ? ps->q1*FD_SHREDDER_CORE_SET_BYTES : batch_sz[c];
    h_off[ c-ps->b ] = pos;
    h_sz [ c-ps->b ] = batch_sz[c];
    memcpy( in + at->desc_at + sizeof(fd_shredder_core_desc_t)*( c-ps->b ), desc + c, sizeof(fd_shredder_core_desc_t) );
    if( privs ) memcpy( in + at->keys_at + 32UL*( c-ps->b ), privs + 32UL*c, 32UL );
    if( to>from ) { memcpy( items + pos, batches + batch_off[c] + from, to-from ); pos += to-from; }
  }
  memcpy( in + at->sfb_at, set_first_b   + ps->b, 4UL*( ps->nbp+1UL ) );
  memcpy( in + at->hfb_at, shred_first_b + ps->b, 4UL*( ps->nbp+1UL ) );
  return skip;
}

/* the out block of a pass of ms sets: 98 bytes a set */
typedef struct { uint64_t roots_at, sigs_at, codes_at, pcodes_at, out_bytes; } fd_shredder_pass_out_t;

static inline fd_shredder_pass_out_t
fd_shredder_pass_out( uint64_t ms ) {
  fd_shredder_pass_out_t o = { 0UL, 32UL*ms, 96UL*ms, 97UL*ms, 98UL*ms };
  return o;
}

/* The pass's m finished shreds, slots FD_SHRED_MAX_SZ apart from shreds (the
   item staging at shreds_at), to the caller: shred i as its 1203 or 1228
   bytes, as its type byte says, at shreds_out + stride i, with
   shred_sz_out[ i ]; the caller passes both from shred h of the call on. */
static inline void
fd_shredder_pass_copy_back( uint8_t const * shreds, uint64_t m, unsigned char * shreds_out, uint64_t stride,
                            unsigned int * shred_sz_out ) {
  for( uint64_t i=0UL; i<m; i++ ) {
    unsigned char const * s = shreds + FD_SHRED_CORE_MAX_SZ*i;
    unsigned sz = ( s[ 0x40 ] & 0xf0 )==0x80 ? FD_SHRED_CORE_MIN_SZ : FD_SHRED_CORE_MAX_SZ;
    memcpy( shreds_out + stride*i, s, sz );
    shred_sz_out[ i ] = sz;
  }
}

#endif /* FD_SHREDDER_PASS_H */
