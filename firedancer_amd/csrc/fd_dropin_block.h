/* fd_dropin_block.h -- the pinned block of one drop-in launch
   (host/fd_ed25519_hip_dropin.c).  A drop-in call is latency-bound (a
   handful of signatures per GPU round trip), so a launch moves one block
   each way instead of an array per field:
     in   [off | sz | tfirst | tcnt | sigs | pubs | dig | msgs]
          every array 16-byte aligned, 16 readable bytes past the last
          message for the SHA-512 loader
     out  [codes | per-transaction codes]
     then, for a host-scalar launch, the host-scalar block
          (fd_ed25519_hip_internal.h), 16-byte aligned
   Plain C11, host only, integer arithmetic and nothing else:
   tests/dropin_block_main.c holds every offset to the formulas the
   drop-in used before the layout had a header of its own. */
#ifndef FD_DROPIN_BLOCK_H
#define FD_DROPIN_BLOCK_H

#include <stdint.h>

#define DROPIN_ALIGN16( x ) (((x) + 15UL) & ~15UL)

typedef struct {          /* byte offsets into the block, in its order */
  uint64_t o_off;         /* u64 [nsig]  a signature's message, from o_msg */
  uint64_t o_sz;          /* u32 [nsig]                                    */
  uint64_t o_tf;          /* u32 [n]     a request's first signature       */
  uint64_t o_tc;          /* u32 [n]     ... and its count                 */
  uint64_t o_sig;         /* [nsig][64]                                    */
  uint64_t o_pub;         /* [nsig][32]                                    */
  uint64_t o_dig;         /* [ndig][64]  digests of R||A||M                */
  uint64_t o_msg;         /* the messages back to back (none staged for host scalars) */
  uint64_t in_sz;         /* what the device reads: [0, in_sz)             */
  uint64_t o_out;         /* i8 [nsig]   codes                             */
  uint64_t o_tout;        /* i8 [n]      per-request codes                 */
  uint64_t o_hsb;         /* the host-scalar block                         */
  uint64_t need;          /* bytes of the whole block                      */
} fd_dropin_block_t;

/* n requests of nsig signatures in all; the nsig_h signatures of requests
   hashed on the host go after the others and travel as digests, the rest
   as bytes message bytes -- or, with host scalars (hsmode; nsig_h is 0
   then), as no message at all and room for nsig digests (the launch's
   fallback), with hs_bytes of host-scalar block behind the codes. */
static inline void
fd_dropin_block( uint64_t n, uint64_t nsig, uint64_t nsig_h, uint64_t bytes, int hsmode, uint64_t hs_bytes,
                 fd_dropin_block_t * b ) {
  uint64_t ndig = hsmode ? nsig : nsig_h;
  b->o_off  = 0UL;
  b->o_sz   = DROPIN_ALIGN16( b->o_off  + 8UL*nsig );
  b->o_tf   = DROPIN_ALIGN16( b->o_sz   + 4UL*nsig );
  b->o_tc   = DROPIN_ALIGN16( b->o_tf   + 4UL*n );
  b->o_sig  = DROPIN_ALIGN16( b->o_tc   + 4UL*n );
  b->o_pub  = DROPIN_ALIGN16( b->o_sig  + 64UL*nsig );
  b->o_dig  = DROPIN_ALIGN16( b->o_pub  + 32UL*nsig );
  b->o_msg  = DROPIN_ALIGN16( b->o_dig  + 64UL*ndig );
  b->in_sz  = b->o_msg + ( hsmode ? 0UL : bytes );
  b->o_out  = DROPIN_ALIGN16( b->in_sz + 16UL );
  b->o_tout = b->o_out + nsig;
  b->need   = b->o_tout + n + 16UL;
  b->o_hsb  = DROPIN_ALIGN16( b->need );
  if( hsmode ) b->need = b->o_hsb + hs_bytes;
}

#endif
