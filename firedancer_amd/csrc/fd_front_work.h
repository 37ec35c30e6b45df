/* fd_front_work.h -- the device workspace of the fronts before the verify
   phases (fd_ed25519_hip_precompile_dev, _shreds_dev, _packets_dev, _crds_dev), carved
   out of the caller's 16-byte-aligned buffer.  Plain C11, host only, nothing
   but pointer arithmetic: the engine (host/fd_ed25519_hip_fronts.c) takes
   its kernels' arrays from here, and tests/front_work_main.c (the CRDS
   front's: tests/crds_work_main.c, the FEC seal's: tests/fec_work_main.c, the proof-of-history check's:
   tests/poh_work_main.c) holds every layout to the public
   FD_ED25519_HIP_*_WORK_BYTES macro a caller sizes the buffer with.  A layout has no padding: the elements only get smaller, so
   every array is aligned to its element at any count. */
#ifndef FD_FRONT_WORK_H
#define FD_FRONT_WORK_H

#include <stdint.h>

/* the next count elements of elem_size bytes */
static inline void *
front_carve( uint8_t ** cursor, uint64_t count, uint64_t elem_size ) {
  void * p = *cursor;
  *cursor += count*elem_size;
  return p;
}

typedef struct {      /* in the buffer's order; [n] slots */
  uint8_t *  sigs;
  uint8_t *  pubs;    /* the shred front's roots (its keys are the caller's leaders): the verify messages, with what lies behind
                         them and the macro's 16 spare bytes to be read past */
  uint8_t *  msgs;    /* the packet front's mirror of the packet buffer, pkt_bytes + 16 (to be read past) rounded up to 16 */
  uint64_t * msg_off;
  uint32_t * msg_sz;
  int8_t *   codes;   /* the verify phases' output */
  int8_t *   pre;
  uint8_t *  ent_instr;                       /* the precompile front's: [n_ent] as the above, */
  int8_t *   status;                          /* and [ntxn] from here                          */
  uint8_t *  hdr_instr;
  uint8_t *  hdr_pos;
  uint32_t * val_sz;                          /* the CRDS front's: [n_val], the size of a value's data */
  uint8_t *  roots;                           /* the FEC seal's: [n_set][32], the sign kernel's messages */
  uint32_t * set_of;                          /* ... and [n], the set that sealed a shred */
} front_work_t;

/* what every layout begins with */
static inline uint8_t *
front_work_slots( void * work, uint64_t n, uint64_t msgs_bytes, front_work_t * w ) {
  uint8_t * c = (uint8_t *)work;
  *w = (front_work_t){ 0 };
  w->sigs    = (uint8_t *) front_carve( &c, n, 64UL );
  w->pubs    = (uint8_t *) front_carve( &c, n, 32UL );
  w->msgs    = (uint8_t *) front_carve( &c, msgs_bytes, 1UL );
  w->msg_off = (uint64_t *)front_carve( &c, n, 8UL );
  w->msg_sz  = (uint32_t *)front_carve( &c, n, 4UL );
  w->codes   = (int8_t *)  front_carve( &c, n, 1UL );
  w->pre     = (int8_t *)  front_carve( &c, n, 1UL );
  return c;
}

/* Each returns the bytes of work it laid out, at most the front's public macro. */

static inline uint64_t
front_work_precompile( void * work, uint64_t ntxn, uint64_t n_ent, front_work_t * w ) {
  uint8_t * c = front_work_slots( work, n_ent, 0UL, w );
  w->ent_instr = (uint8_t *)front_carve( &c, n_ent, 1UL );
  w->status    = (int8_t *) front_carve( &c, ntxn,  1UL );
  w->hdr_instr = (uint8_t *)front_carve( &c, ntxn,  1UL );
  w->hdr_pos   = (uint8_t *)front_carve( &c, ntxn,  1UL );
  return (uint64_t)( c - (uint8_t *)work );
}

static inline uint64_t
front_work_shred( void * work, uint64_t n, front_work_t * w ) {
  return (uint64_t)( front_work_slots( work, n, 0UL, w ) - (uint8_t *)work );
}

static inline uint64_t
front_work_packet( void * work, uint64_t n, uint64_t pkt_bytes, front_work_t * w ) {
  return (uint64_t)( front_work_slots( work, n, ( pkt_bytes + 31UL ) & ~15UL, w ) - (uint8_t *)work );
}

/* The CRDS front keeps a 4-byte array more per slot (val_sz), which has to
   stand ahead of the 1-byte ones, so it carves its slots itself; its
   messages are read in place.  status: [n], the packets' codes. */
static inline uint64_t
front_work_crds( void * work, uint64_t n, uint64_t n_val, front_work_t * w ) {
  uint8_t * c = (uint8_t *)work;
  *w = (front_work_t){ 0 };
  w->sigs    = (uint8_t *) front_carve( &c, n_val, 64UL );
  w->pubs    = (uint8_t *) front_carve( &c, n_val, 32UL );
  w->msg_off = (uint64_t *)front_carve( &c, n_val, 8UL );
  w->msg_sz  = (uint32_t *)front_carve( &c, n_val, 4UL );
  w->val_sz  = (uint32_t *)front_carve( &c, n_val, 4UL );
  w->codes   = (int8_t *)  front_carve( &c, n_val, 1UL );
  w->pre     = (int8_t *)  front_carve( &c, n_val, 1UL );
  w->status  = (int8_t *)  front_carve( &c, n,     1UL );
  return (uint64_t)( c - (uint8_t *)work );
}

/* The FEC seal (fd_ed25519_hip_fec_seal_dev) has no verify phases: [n_set]
   slots of the sign kernel -- signature, public key, the root as the
   message, its offset and size -- and the set of each of the n shreds. */
static inline uint64_t
front_work_fec( void * work, uint64_t n, uint64_t n_set, front_work_t * w ) {
  uint8_t * c = (uint8_t *)work;
  *w = (front_work_t){ 0 };
  w->sigs    = (uint8_t *) front_carve( &c, n_set, 64UL );
  w->pubs    = (uint8_t *) front_carve( &c, n_set, 32UL );
  w->roots   = (uint8_t *) front_carve( &c, n_set, 32UL );
  w->msg_off = (uint64_t *)front_carve( &c, n_set, 8UL );
  w->msg_sz  = (uint32_t *)front_carve( &c, n_set, 4UL );
  w->set_of  = (uint32_t *)front_carve( &c, n,     4UL );
  return (uint64_t)( c - (uint8_t *)work );
}

/* The proof-of-history check (fd_ed25519_hip_poh_dev) has no verify phases
   either: the leaf hashes, which the tree kernel reduces in place, [n_sig]
   rows of eight words; the roots, [n] rows; and the tree's flag per
   microblock (a signature that leaves the buffer).  tools/poh_bench.py
   repeats this order (Batch.params): change both together. */
typedef struct {
  uint32_t * leaves;
  uint32_t * roots;
  int8_t *   pre;
} front_work_poh_t;

static inline uint64_t
front_work_poh( void * work, uint64_t n, uint64_t n_sig, front_work_poh_t * w ) {
  uint8_t * c = (uint8_t *)work;
  w->leaves = (uint32_t *)front_carve( &c, n_sig, 32UL );
  w->roots  = (uint32_t *)front_carve( &c, n,     32UL );
  w->pre    = (int8_t *)  front_carve( &c, n,     1UL );
  return (uint64_t)( c - (uint8_t *)work );
}

#endif /* FD_FRONT_WORK_H */
