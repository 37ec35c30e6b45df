/* fd_ed25519_hip_fronts.c -- the fronts before the verify phases
   (include/fd_ed25519_hip.h Parts 2b-2j): stage kernel, verify_common,
   finish kernel in a *_dev; pack, upload, *_dev, download, synchronise in a
   *_host ("The shape of a front"); and the rules the stage
   kernels run, on the host (*_count, *_plan, *_root, fec_parity, fec_recover, poh, poh_prepare, shredder).  Part of the engine:
   the *_host wrappers stage in its pinned buffers
   (fd_ed25519_hip_engine_fields.h).  The three wrappers over whole FEC sets
   (fec_seal_host, fec_parity_host, fec_recover_host) share one pass by sets
   -- cut, room, stage; upload; *_dev; download and the front's own copy-back
   -- whose cut, in-block layout and staging are plain C in ../fd_fec_pass.h,
   held to their buffers under ASan and UBSan by tests/fec_pass_main.c.  The
   two other wrappers that work pass by pass have the same shape over a header
   of their own: shredder_host over ../fd_shredder_pass.h
   (tests/shredder_pass_main.c), poh_host and poh_blocks_host over
   ../fd_poh_pass.h (tests/poh_pass_main.c). */

#define _GNU_SOURCE
#include "fd_ed25519_hip_engine_fields.h"
#include "../../../include/fd_ed25519_hip_tile.h"   /* fd_ed25519_hip_txn_t, for the parse core */
#include "../fd_txn_parse_core.h"
#include "../fd_precompile_core.h"
#include "../fd_shred_core.h"
#include "../fd_packet_core.h"
#include "../fd_crds_core.h"
#include "../fd_fec_core.h"
#include "../fd_reedsol_core.h"
#include "../fd_poh_core.h"
#include "../fd_front_work.h"
#include "../fd_fec_pass.h"
#include "../fd_shredder_core.h"
#include "../fd_shredder_pass.h"
#include "../fd_poh_pass.h"

#include <stddef.h>
#include <stdlib.h>
#include <string.h>

/* What an entry point does before any work.  Returns 1 to go on (the device
   set, *st the call's stream), else the call's result: OK for an empty
   batch, ERR_INVAL for a missing argument (args_ok: the caller's NULL and
   range checks) or when one of the pointers or-ed into aligned16 (names, for
   the message) is off a 16-byte boundary. */
static int
front_begin( fd_ed25519_hip_engine_t * e, unsigned long n, int args_ok, uintptr_t aligned16, char const * names,
             void * stream, hipStream_t * st ) {
  if( !e ) return FD_ED25519_HIP_ERR_INVAL;
  if( !n ) return FD_ED25519_HIP_OK;
  if( !args_ok ) return FD_ED25519_HIP_ERR_INVAL;
  if( aligned16 & 15UL ) {
    fd_ed25519_hip_private_set_errorf( "%s must be 16-byte aligned", names );
    return FD_ED25519_HIP_ERR_INVAL;
  }
  *st = stream ? (hipStream_t)stream : e->stream;
  HIPCHK( hipSetDevice( e->device ), "hipSetDevice" );
  return 1;
}

/* the layout the kernels are about to write against the size the caller was told to allocate */
static int
front_work_fits( uint64_t end, uint64_t public_bytes, char const * what ) {
  if( end<=public_bytes ) return FD_ED25519_HIP_OK;
  fd_ed25519_hip_private_set_errorf( "%s workspace: %lu bytes laid out, %lu public", what, (unsigned long)end,
                                     (unsigned long)public_bytes );
  return FD_ED25519_HIP_ERR_INVAL;
}

/* device-only buffer grown on demand, like grow_pair */
static int
grow_dev( uint8_t ** d, uint64_t * cap, uint64_t need ) {
  if( need<=*cap ) return FD_ED25519_HIP_OK;
  uint64_t ncap = *cap ? *cap : 4096UL;
  while( ncap<need ) ncap *= 2UL;
  hipFree( *d ); *d = NULL; *cap = 0UL;
  HIPCHK( hipMalloc( (void **)d, ncap ), "hipMalloc" );
  *cap = ncap;
  return FD_ED25519_HIP_OK;
}

/* a pass of a host wrapper: room for its item bytes (with 64 bytes behind the last) and its in and out blocks */
static int
front_room( fd_ed25519_hip_engine_t * e, uint64_t item_bytes, uint64_t in_bytes, uint64_t out_bytes ) {
  int err;
  if( (err = fd_ed25519_hip_private_stage_msgs( e, item_bytes )) ) return err;
  if( (err = fd_ed25519_hip_private_grow_pair( (void **)&e->h_fr_in, (void **)&e->d_fr_in, &e->fr_in_cap, in_bytes, 1UL )) ) return err;
  return fd_ed25519_hip_private_grow_pair( (void **)&e->h_fr_out, (void **)&e->d_fr_out, &e->fr_out_cap, out_bytes, 1UL );
}

/* ... the items [off[i], off[i]+sz[i]) back to back in the pinned item staging, their places and true sizes in
   h_off and h_sz; an item of more than cap bytes travels as its first over bytes.  Returns the bytes packed */
static uint64_t
front_pack( fd_ed25519_hip_engine_t * e, uint64_t m, unsigned char const * items, unsigned long const * off,
            unsigned int const * sz, uint64_t cap, uint64_t over, uint64_t * h_off, uint32_t * h_sz ) {
  uint64_t pos = 0UL;
  for( uint64_t i=0UL; i<m; i++ ) {
    uint64_t cp = sz[i]<=cap ? sz[i] : over;
    if( cp ) memcpy( e->h_msgs + pos, items + off[i], cp );
    h_off[i] = pos;
    h_sz [i] = sz[i];
    pos += cp;
  }
  return pos;
}

/* ... the items and the in block to the device; the out block back, with the stream drained */
static int
front_upload( fd_ed25519_hip_engine_t * e, uint64_t item_bytes, uint64_t in_bytes, hipStream_t st ) {
  HIPCHK( hipMemcpyAsync( e->d_msgs, e->h_msgs, item_bytes ? item_bytes : 1UL, hipMemcpyHostToDevice, st ), "H2D front items" );
  HIPCHK( hipMemcpyAsync( e->d_fr_in, e->h_fr_in, in_bytes, hipMemcpyHostToDevice, st ), "H2D front in" );
  return FD_ED25519_HIP_OK;
}

static int
front_download( fd_ed25519_hip_engine_t * e, uint64_t out_bytes, hipStream_t st ) {
  HIPCHK( hipMemcpyAsync( e->h_fr_out, e->d_fr_out, out_bytes, hipMemcpyDeviceToHost, st ), "D2H front out" );
  HIPCHK( hipStreamSynchronize( st ), "front" );
  return FD_ED25519_HIP_OK;
}

/* ---- Ed25519 precompile instructions (include/fd_ed25519_hip.h Part 2b) -- */

_Static_assert( FD_ED25519_HIP_PRECOMPILE_ENT_MAX==FD_PRECOMPILE_CORE_ENT_MAX, "entry bound" );
_Static_assert( FD_ED25519_HIP_PRECOMPILE_ERR_SIGNATURE==FD_PRECOMPILE_CORE_ERR_SIGNATURE &&
                FD_ED25519_HIP_PRECOMPILE_ERR_DATA_OFFSET==FD_PRECOMPILE_CORE_ERR_DATA_OFFSET &&
                FD_ED25519_HIP_PRECOMPILE_ERR_INSTR_DATA_SIZE==FD_PRECOMPILE_CORE_ERR_INSTR_DATA_SIZE,
                "public and core precompile codes differ" );
/* the plan's entries are the core's, copied as bytes */
_Static_assert( sizeof(fd_ed25519_hip_precompile_ent_t)==sizeof(fd_precompile_core_ent_t) &&
                offsetof(fd_ed25519_hip_precompile_ent_t,pre    )==offsetof(fd_precompile_core_ent_t,pre    ) &&
                offsetof(fd_ed25519_hip_precompile_ent_t,sig_off)==offsetof(fd_precompile_core_ent_t,sig_off) &&
                offsetof(fd_ed25519_hip_precompile_ent_t,pub_off)==offsetof(fd_precompile_core_ent_t,pub_off) &&
                offsetof(fd_ed25519_hip_precompile_ent_t,msg_off)==offsetof(fd_precompile_core_ent_t,msg_off) &&
                offsetof(fd_ed25519_hip_precompile_ent_t,msg_sz )==offsetof(fd_precompile_core_ent_t,msg_sz ),
                "plan entry layout" );

/* count and plan: the walk the stage kernel runs, on the host (no GPU) */
unsigned
fd_ed25519_hip_precompile_count( unsigned char const * payload, unsigned long payload_sz ) {
  fd_precompile_core_sum_t sum;
  int parsed;
  fd_precompile_core_plan( payload, payload_sz, NULL, 0UL, &sum, &parsed );
  return sum.ent_cnt;
}

int
fd_ed25519_hip_precompile_plan( unsigned char const * payload, unsigned long payload_sz,
                                fd_ed25519_hip_precompile_ent_t * ents, unsigned long cap,
                                signed char * parse_or_header_code, unsigned char * instr ) {
  fd_precompile_core_sum_t sum;
  int parsed;
  int n = fd_precompile_core_plan( payload, payload_sz, (fd_precompile_core_ent_t *)ents, ents ? cap : 0UL, &sum, &parsed );
  if( parse_or_header_code )
    *parse_or_header_code = (signed char)( !parsed ? FD_ED25519_HIP_PRECOMPILE_PARSE_FAILED
                                         : sum.hdr_instr!=0xFF ? FD_ED25519_HIP_PRECOMPILE_ERR_INSTR_DATA_SIZE : 0 );
  if( instr ) *instr = sum.hdr_instr;
  return n;
}

int
fd_ed25519_hip_precompile_dev( fd_ed25519_hip_engine_t * e, unsigned long ntxn, unsigned char const * payloads,
                               unsigned long const * pay_off, unsigned int const * pay_sz,
                               unsigned int const * ent_first, unsigned long n_ent, void * work,
                               signed char * txn_out, unsigned char * instr_out, signed char * ent_out,
                               void * stream ) {
  hipStream_t st;
  int err = front_begin( e, ntxn, payloads && pay_off && pay_sz && ent_first && work && txn_out && instr_out &&
                                  n_ent<=ntxn*FD_ED25519_HIP_PRECOMPILE_ENT_MAX,
                         (uintptr_t)work, "precompile work", stream, &st );
  if( err<=0 ) return err;
  front_work_t w;
  err = front_work_fits( front_work_precompile( work, ntxn, n_ent, &w ), FD_ED25519_HIP_PRECOMPILE_WORK_BYTES( ntxn, n_ent ),
                         "precompile" );
  if( err ) return err;
  fd_ed25519_precompile_stage_params_t sp = { 0 };
  sp.payloads = payloads; sp.pay_off = (uint64_t const *)pay_off; sp.pay_sz = pay_sz; sp.ent_first = ent_first;
  sp.ntxn = ntxn; sp.n_ent = n_ent;
  sp.sigs = w.sigs; sp.pubs = w.pubs; sp.msg_off = w.msg_off; sp.msg_sz = w.msg_sz; sp.pre = w.pre;
  sp.ent_instr = w.ent_instr; sp.status = w.status; sp.hdr_instr = w.hdr_instr; sp.hdr_pos = w.hdr_pos;
  HIPCHK( (hipError_t)fd_ed25519_hip_launch_precompile_stage( &sp, st ), "precompile_stage launch" );
  if( n_ent ) {
    err = fd_ed25519_hip_private_verify_common( e, n_ent, payloads, (unsigned long const *)w.msg_off, w.msg_sz, NULL, w.sigs, w.pubs,
                         (signed char *)w.codes, st );
    if( err ) return err;
  }
  fd_ed25519_precompile_finish_params_t fp = { 0 };
  fp.codes = w.codes; fp.pre = w.pre; fp.ent_instr = w.ent_instr; fp.status = w.status;
  fp.hdr_instr = w.hdr_instr; fp.hdr_pos = w.hdr_pos; fp.ent_first = ent_first; fp.ntxn = ntxn; fp.n_ent = n_ent;
  fp.txn_out = (int8_t *)txn_out; fp.instr_out = instr_out; fp.ent_out = (int8_t *)ent_out;
  HIPCHK( (hipError_t)fd_ed25519_hip_launch_precompile_finish( &fp, st ), "precompile_finish launch" );
  return FD_ED25519_HIP_OK;
}

/* one pass over ntxn: the entries are counted from the packed copies, the ones the device will read */
int
fd_ed25519_hip_precompile_host( fd_ed25519_hip_engine_t * e, unsigned long ntxn, unsigned char const * payloads,
                                unsigned long const * pay_off, unsigned int const * pay_sz, signed char * txn_out,
                                unsigned char * instr_out ) {
  hipStream_t st;
  int err = front_begin( e, ntxn, payloads && pay_off && pay_sz && txn_out && instr_out, 0UL, NULL, NULL, &st );
  if( err<=0 ) return err;
  uint64_t bytes = 0UL;
  for( uint64_t t=0UL; t<ntxn; t++ ) bytes += pay_sz[t];
  /* in: pay_off u64 [ntxn], ent_first u32 [ntxn+1], pay_sz u32 [ntxn]; out: txn_out, instr_out [ntxn] */
  uint64_t in_bytes = 16UL*ntxn + 4UL, first_at = 8UL*ntxn, sz_at = 12UL*ntxn + 4UL;
  if( (err = front_room( e, bytes, in_bytes, 2UL*ntxn )) ) return err;
  uint64_t * h_off   = (uint64_t *)e->h_fr_in;
  uint32_t * h_first = (uint32_t *)( e->h_fr_in + first_at );
  front_pack( e, ntxn, payloads, pay_off, pay_sz, UINT64_MAX, 0UL, h_off, (uint32_t *)( e->h_fr_in + sz_at ) );
  uint64_t n_ent = 0UL;
  for( uint64_t t=0UL; t<ntxn; t++ ) {
    h_first[t] = (uint32_t)n_ent;
    n_ent += fd_ed25519_hip_precompile_count( e->h_msgs + h_off[t], pay_sz[t] );
  }
  h_first[ntxn] = (uint32_t)n_ent;
  if( (err = grow_dev( &e->d_fr_work, &e->fr_work_cap, FD_ED25519_HIP_PRECOMPILE_WORK_BYTES( ntxn, n_ent ) )) ) return err;
  if( (err = front_upload( e, bytes, in_bytes, st )) ) return err;
  if( (err = fd_ed25519_hip_precompile_dev( e, ntxn, e->d_msgs, (unsigned long const *)e->d_fr_in,
                                            (unsigned int const *)( e->d_fr_in + sz_at ),
                                            (unsigned int const *)( e->d_fr_in + first_at ), n_ent, e->d_fr_work,
                                            (signed char *)e->d_fr_out, e->d_fr_out + ntxn, NULL, st )) ) return err;
  if( (err = front_download( e, 2UL*ntxn, st )) ) return err;
  memcpy( txn_out,   e->h_fr_out,        ntxn );
  memcpy( instr_out, e->h_fr_out + ntxn, ntxn );
  return FD_ED25519_HIP_OK;
}

/* ---- leader signatures of Merkle shreds (include/fd_ed25519_hip.h Part 2c) -- */

_Static_assert( FD_ED25519_HIP_SHRED_OK==FD_SHRED_CORE_OK && FD_ED25519_HIP_SHRED_ERR_PARSE==FD_SHRED_CORE_ERR_PARSE &&
                FD_ED25519_HIP_SHRED_UNSUPPORTED==FD_SHRED_CORE_UNSUPPORTED &&
                FD_ED25519_HIP_SHRED_ERR_HEADER==FD_SHRED_CORE_ERR_HEADER &&
                FD_ED25519_HIP_SHRED_ERR_SIGNATURE==FD_SHRED_CORE_ERR_SIGNATURE,
                "public and core shred codes differ" );

/* the rules and the hashes the stage kernel runs, on the host (no GPU) */
int
fd_ed25519_hip_shred_root( unsigned char const * shred, unsigned long sz, unsigned char * root ) {
  return fd_shred_core_root( shred, sz, root );
}

int
fd_ed25519_hip_shreds_dev( fd_ed25519_hip_engine_t * e, unsigned long n, unsigned char const * shreds,
                           unsigned long const * shred_off, unsigned int const * shred_sz,
                           unsigned char const * leaders, void * work, signed char * out, unsigned char * roots,
                           signed char * sig_out, void * stream ) {
  hipStream_t st;
  int err = front_begin( e, n, shreds && shred_off && shred_sz && leaders && work && out,
                         (uintptr_t)work | (uintptr_t)leaders | (uintptr_t)roots | (uintptr_t)shreds,
                         "shreds/leaders/work/roots", stream, &st );
  if( err<=0 ) return err;
  front_work_t w;
  if( (err = front_work_fits( front_work_shred( work, n, &w ), FD_ED25519_HIP_SHRED_WORK_BYTES( n ), "shred" )) ) return err;
  fd_ed25519_shred_stage_params_t sp = { 0 };
  sp.shreds = shreds; sp.shred_off = (uint64_t const *)shred_off; sp.shred_sz = shred_sz; sp.n = n;
  sp.sigs = w.sigs; sp.roots = w.pubs /* the keys are the leaders */; sp.msg_off = w.msg_off; sp.msg_sz = w.msg_sz; sp.pre = w.pre;
  HIPCHK( (hipError_t)fd_ed25519_hip_launch_shred_stage( &sp, st ), "shred_stage launch" );
  err = fd_ed25519_hip_private_verify_common( e, n, w.pubs, (unsigned long const *)w.msg_off, w.msg_sz, NULL, w.sigs, leaders,
                       (signed char *)w.codes, st );
  if( err ) return err;
  fd_ed25519_shred_finish_params_t fp = { 0 };
  fp.codes = w.codes; fp.pre = w.pre; fp.roots = w.pubs; fp.n = n;
  fp.out = (int8_t *)out; fp.roots_out = roots; fp.sig_out = (int8_t *)sig_out;
  HIPCHK( (hipError_t)fd_ed25519_hip_launch_shred_finish( &fp, st ), "shred_finish launch" );
  return FD_ED25519_HIP_OK;
}

/* ---- signed gossip and repair control packets (include/fd_ed25519_hip.h Part 2d) -- */

_Static_assert( FD_ED25519_HIP_PACKET_OK==FD_PACKET_CORE_OK && FD_ED25519_HIP_PACKET_ERR_PARSE==FD_PACKET_CORE_ERR_PARSE &&
                FD_ED25519_HIP_PACKET_UNSUPPORTED==FD_PACKET_CORE_UNSUPPORTED &&
                FD_ED25519_HIP_PACKET_ERR_SIGNATURE==FD_PACKET_CORE_ERR_SIGNATURE &&
                FD_ED25519_HIP_PACKET_NOT_FOR_SELF==FD_PACKET_CORE_NOT_FOR_SELF &&
                FD_ED25519_HIP_PROTO_GOSSIP==FD_PACKET_CORE_PROTO_GOSSIP &&
                FD_ED25519_HIP_PROTO_REPAIR_SERV==FD_PACKET_CORE_PROTO_REPAIR_SERV &&
                FD_ED25519_HIP_PACKET_MAX==FD_PACKET_CORE_MAX &&
                sizeof(fd_ed25519_hip_packet_plan_t)==sizeof(fd_packet_core_plan_t),
                "public and core packet constants differ" );

static int
packet_proto_ok( int proto ) {
  return ( proto==FD_ED25519_HIP_PROTO_GOSSIP ) | ( proto==FD_ED25519_HIP_PROTO_REPAIR_SERV );
}

/* the rules the stage kernel runs, on the host (no GPU) */
int
fd_ed25519_hip_packet_plan( int proto, unsigned char const * pkt, unsigned long sz, unsigned char const self_key[ 32 ],
                            fd_ed25519_hip_packet_plan_t * plan ) {
  if( !packet_proto_ok( proto ) || !self_key || !plan ) return FD_ED25519_HIP_ERR_INVAL;
  fd_packet_core_plan_t c;
  int code = fd_packet_core_plan( proto, pkt, sz, self_key, &c );
  memcpy( plan, &c, sizeof(c) );
  return code;
}

int
fd_ed25519_hip_packets_dev( fd_ed25519_hip_engine_t * e, int proto, unsigned long n, unsigned char const * pkts,
                            unsigned long const * pkt_off, unsigned int const * pkt_sz, unsigned long pkt_bytes,
                            unsigned char const self_key[ 32 ], void * work, signed char * out, signed char * sig_out,
                            void * stream ) {
  if( !packet_proto_ok( proto ) || !self_key ) return FD_ED25519_HIP_ERR_INVAL;   /* of an empty batch too */
  hipStream_t st;
  int err = front_begin( e, n, pkts && pkt_off && pkt_sz && work && out, (uintptr_t)work | (uintptr_t)pkts, "pkts/work",
                         stream, &st );
  if( err<=0 ) return err;
  front_work_t w;
  err = front_work_fits( front_work_packet( work, n, pkt_bytes, &w ), FD_ED25519_HIP_PACKET_WORK_BYTES( n, pkt_bytes ),
                         "packet" );
  if( err ) return err;
  fd_ed25519_packet_stage_params_t sp = { 0 };
  sp.pkts = pkts; sp.pkt_off = (uint64_t const *)pkt_off; sp.pkt_sz = pkt_sz; sp.n = n; sp.pkt_bytes = pkt_bytes;
  memcpy( sp.self_key, self_key, 32UL );
  sp.proto = proto;
  sp.sigs = w.sigs; sp.pubs = w.pubs; sp.msgs = w.msgs; sp.msg_off = w.msg_off; sp.msg_sz = w.msg_sz; sp.pre = w.pre;
  HIPCHK( (hipError_t)fd_ed25519_hip_launch_packet_stage( &sp, st ), "packet_stage launch" );
  err = fd_ed25519_hip_private_verify_common( e, n, w.msgs, (unsigned long const *)w.msg_off, w.msg_sz, NULL, w.sigs, w.pubs,
                       (signed char *)w.codes, st );
  if( err ) return err;
  fd_ed25519_packet_finish_params_t fp = { 0 };
  fp.codes = w.codes; fp.pre = w.pre; fp.n = n; fp.out = (int8_t *)out; fp.sig_out = (int8_t *)sig_out;
  HIPCHK( (hipError_t)fd_ed25519_hip_launch_packet_finish( &fp, st ), "packet_finish launch" );
  return FD_ED25519_HIP_OK;
}

/* ---- shreds_host and packets_host ---------------------------------------- */

/* items per pass: bounds the pinned staging (20 MiB of item bytes) whatever n is */
#define FRONT_HOST_CHUNK 16384UL

/* The round trip of shreds (leaders given) and of packets (leaders NULL),
   pass by pass.  A shred pass has the leaders, 32 bytes each, in front of
   its in block (off u64 [m], sz u32 [m]) and the roots, 32 bytes each, in
   front of its out block (codes [m]).  No shred rule reads a byte at or past
   FD_SHRED_MAX_SZ, so a longer shred travels as its head and its true size;
   no packet rule reads a packet of more than FD_ED25519_HIP_PACKET_MAX bytes
   at all: it travels as its true size alone, and leaves the packed range. */
static int
front_items_host( fd_ed25519_hip_engine_t * e, hipStream_t st, unsigned long n, unsigned char const * items,
                  unsigned long const * off, unsigned int const * sz, unsigned char const * leaders, int proto,
                  unsigned char const * self_key, signed char * out, unsigned char * roots ) {
  uint64_t cap  = leaders ? FD_SHRED_CORE_MAX_SZ : FD_PACKET_CORE_MAX, over = leaders ? cap : 0UL;
  uint64_t lead = leaders ? 32UL : 0UL;
  int err;
  for( uint64_t base=0UL; base<n; base+=FRONT_HOST_CHUNK ) {
    uint64_t m = n-base<FRONT_HOST_CHUNK ? n-base : FRONT_HOST_CHUNK;
    uint64_t off_at = lead*m, sz_at = off_at + 8UL*m, in_bytes = sz_at + 4UL*m, out_bytes = lead*m + m;
    if( (err = front_room( e, m*cap, in_bytes, out_bytes )) ) return err;
    if( leaders ) memcpy( e->h_fr_in, leaders + 32UL*base, 32UL*m );
    uint64_t pos = front_pack( e, m, items, off+base, sz+base, cap, over, (uint64_t *)( e->h_fr_in + off_at ),
                               (uint32_t *)( e->h_fr_in + sz_at ) );
    uint64_t work = leaders ? FD_ED25519_HIP_SHRED_WORK_BYTES( m ) : FD_ED25519_HIP_PACKET_WORK_BYTES( m, pos );
    if( (err = grow_dev( &e->d_fr_work, &e->fr_work_cap, work )) ) return err;
    if( (err = front_upload( e, pos, in_bytes, st )) ) return err;
    unsigned long const * d_off   = (unsigned long const *)( e->d_fr_in + off_at );
    unsigned int const *  d_sz    = (unsigned int const *)( e->d_fr_in + sz_at );
    signed char *         d_codes = (signed char *)( e->d_fr_out + lead*m );
    err = leaders ? fd_ed25519_hip_shreds_dev( e, m, e->d_msgs, d_off, d_sz, e->d_fr_in, e->d_fr_work, d_codes,
                                               roots ? e->d_fr_out : NULL, NULL, st )
                  : fd_ed25519_hip_packets_dev( e, proto, m, e->d_msgs, d_off, d_sz, pos, self_key, e->d_fr_work, d_codes,
                                                NULL, st );
    if( err ) return err;
    if( (err = front_download( e, out_bytes, st )) ) return err;
    memcpy( out + base, e->h_fr_out + lead*m, m );
    if( roots ) memcpy( roots + 32UL*base, e->h_fr_out, 32UL*m );
  }
  return FD_ED25519_HIP_OK;
}

int
fd_ed25519_hip_shreds_host( fd_ed25519_hip_engine_t * e, unsigned long n, unsigned char const * shreds,
                            unsigned long const * shred_off, unsigned int const * shred_sz,
                            unsigned char const * leaders, signed char * out, unsigned char * roots ) {
  hipStream_t st;
  int err = front_begin( e, n, shreds && shred_off && shred_sz && leaders && out, 0UL, NULL, NULL, &st );
  if( err<=0 ) return err;
  return front_items_host( e, st, n, shreds, shred_off, shred_sz, leaders, 0, NULL, out, roots );
}

int
fd_ed25519_hip_packets_host( fd_ed25519_hip_engine_t * e, int proto, unsigned long n, unsigned char const * pkts,
                             unsigned long const * pkt_off, unsigned int const * pkt_sz,
                             unsigned char const self_key[ 32 ], signed char * out ) {
  if( !packet_proto_ok( proto ) || !self_key ) return FD_ED25519_HIP_ERR_INVAL;
  hipStream_t st;
  int err = front_begin( e, n, pkts && pkt_off && pkt_sz && out, 0UL, NULL, NULL, &st );
  if( err<=0 ) return err;
  return front_items_host( e, st, n, pkts, pkt_off, pkt_sz, NULL, proto, self_key, out, NULL );
}

/* ---- CRDS values of gossip pull responses and push messages (include/fd_ed25519_hip.h Part 2e) -- */

_Static_assert( FD_ED25519_HIP_CRDS_OK==FD_CRDS_CORE_OK && FD_ED25519_HIP_CRDS_ERR_PARSE==FD_CRDS_CORE_ERR_PARSE &&
                FD_ED25519_HIP_CRDS_UNSUPPORTED==FD_CRDS_CORE_UNSUPPORTED &&
                FD_ED25519_HIP_CRDS_ERR_SIGNATURE==FD_CRDS_CORE_ERR_SIGNATURE &&
                FD_ED25519_HIP_CRDS_OWN==FD_CRDS_CORE_OWN && FD_ED25519_HIP_CRDS_VAL_MAX==FD_CRDS_CORE_VAL_MAX &&
                FD_ED25519_HIP_PACKET_MAX==FD_CRDS_CORE_MAX &&
                FD_CRDS_CORE_HDR_SZ + FD_CRDS_CORE_VAL_MAX*FD_CRDS_CORE_VAL_MIN<=FD_CRDS_CORE_MAX &&
                FD_CRDS_CORE_HDR_SZ + ( FD_CRDS_CORE_VAL_MAX+1UL )*FD_CRDS_CORE_VAL_MIN>FD_CRDS_CORE_MAX,
                "public and core CRDS constants differ" );
/* the plan's values are the core's, copied as bytes */
_Static_assert( sizeof(fd_ed25519_hip_crds_val_t)==sizeof(fd_crds_core_val_t) &&
                offsetof(fd_ed25519_hip_crds_val_t,disc   )==offsetof(fd_crds_core_val_t,disc   ) &&
                offsetof(fd_ed25519_hip_crds_val_t,sig_off)==offsetof(fd_crds_core_val_t,sig_off) &&
                offsetof(fd_ed25519_hip_crds_val_t,key_off)==offsetof(fd_crds_core_val_t,key_off) &&
                offsetof(fd_ed25519_hip_crds_val_t,msg_off)==offsetof(fd_crds_core_val_t,msg_off) &&
                offsetof(fd_ed25519_hip_crds_val_t,msg_sz )==offsetof(fd_crds_core_val_t,msg_sz ) &&
                offsetof(fd_ed25519_hip_crds_val_t,pre    )==offsetof(fd_crds_core_val_t,pre    ),
                "plan value layout" );

/* count and plan: the walk the stage kernel runs, on the host (no GPU) */
unsigned
fd_ed25519_hip_crds_count( unsigned char const * pkt, unsigned long sz ) {
  fd_crds_core_idx_t idx;
  fd_crds_core_walk( pkt, sz, &idx );
  return idx.cnt;
}

int
fd_ed25519_hip_crds_plan( unsigned char const * pkt, unsigned long sz, unsigned char const self_key[ 32 ],
                          fd_ed25519_hip_crds_val_t * vals, unsigned long cap, signed char * pkt_code ) {
  if( !self_key ) return FD_ED25519_HIP_ERR_INVAL;
  fd_crds_core_idx_t idx;
  int code = fd_crds_core_walk( pkt, sz, &idx );
  if( pkt_code ) *pkt_code = (signed char)code;
  unsigned k = 0U;
  for( ; vals && k<idx.cnt && k<cap; k++ ) {
    fd_crds_core_val_t v = { 0 };
    fd_crds_core_value( pkt, sz, &idx, k, self_key, &v );
    memcpy( vals + k, &v, sizeof(v) );
  }
  return (int)k;
}

int
fd_ed25519_hip_crds_dev( fd_ed25519_hip_engine_t * e, unsigned long n, unsigned char const * pkts,
                         unsigned long const * pkt_off, unsigned int const * pkt_sz, unsigned long pkt_bytes,
                         unsigned char const self_key[ 32 ], unsigned int const * val_first, unsigned long n_val,
                         void * work, signed char * pkt_out, signed char * val_out, signed char * sig_out,
                         unsigned char * hash_out, void * stream ) {
  if( !self_key ) return FD_ED25519_HIP_ERR_INVAL;   /* of an empty batch too */
  hipStream_t st;
  int err = front_begin( e, n, pkts && pkt_off && pkt_sz && val_first && work && pkt_out && ( val_out || !n_val ) &&
                               n_val<=n*FD_ED25519_HIP_CRDS_VAL_MAX && !( (uintptr_t)pkts & 3UL ) && !( (uintptr_t)hash_out & 3UL ),
                         (uintptr_t)work, "crds work", stream, &st );
  if( err<=0 ) return err;
  front_work_t w;
  err = front_work_fits( front_work_crds( work, n, n_val, &w ), FD_ED25519_HIP_CRDS_WORK_BYTES( n, n_val ), "crds" );
  if( err ) return err;
  fd_ed25519_crds_stage_params_t sp = { 0 };
  sp.pkts = pkts; sp.pkt_off = (uint64_t const *)pkt_off; sp.pkt_sz = pkt_sz; sp.val_first = val_first;
  sp.n = n; sp.n_val = n_val; sp.pkt_bytes = pkt_bytes;
  memcpy( sp.self_key, self_key, 32UL );
  sp.sigs = w.sigs; sp.pubs = w.pubs; sp.msg_off = w.msg_off; sp.msg_sz = w.msg_sz; sp.val_sz = w.val_sz; sp.pre = w.pre;
  sp.status = w.status;
  /* The stage fills the slots val_first reserves.  A val_first that is no prefix sum (it runs backwards, leaves n_val or
     skips slots) leaves slots no lane fills, and the verify phases read every slot's message offset: empty messages at
     offset 0 and BAD_RESERVATION for all, ahead of the stage (msg_off, msg_sz, val_sz and codes are adjacent). */
  if( n_val ) {
    HIPCHK( hipMemsetAsync( w.msg_off, 0, 17UL*n_val, st ), "crds slots memset" );
    HIPCHK( hipMemsetAsync( w.pre, FD_ED25519_HIP_CRDS_BAD_RESERVATION & 0xFF, n_val, st ), "crds slots memset" );
  }
  HIPCHK( (hipError_t)fd_ed25519_hip_launch_crds_stage( &sp, st ), "crds_stage launch" );
  if( n_val ) {
    err = fd_ed25519_hip_private_verify_common( e, n_val, pkts, (unsigned long const *)w.msg_off, w.msg_sz, NULL, w.sigs, w.pubs,
                         (signed char *)w.codes, st );
    if( err ) return err;
  }
  fd_ed25519_crds_finish_params_t fp = { 0 };
  fp.codes = w.codes; fp.pre = w.pre; fp.status = w.status; fp.n = n; fp.n_val = n_val;
  fp.pkt_out = (int8_t *)pkt_out; fp.val_out = (int8_t *)val_out; fp.sig_out = (int8_t *)sig_out;
  HIPCHK( (hipError_t)fd_ed25519_hip_launch_crds_finish( &fp, st ), "crds_finish launch" );
  if( hash_out ) {
    fd_ed25519_crds_hash_params_t hp = { 0 };
    hp.pkts = pkts; hp.msg_off = w.msg_off; hp.val_sz = w.val_sz; hp.n_val = n_val; hp.hash_out = hash_out;
    HIPCHK( (hipError_t)fd_ed25519_hip_launch_crds_hash( &hp, st ), "crds_hash launch" );
  }
  return FD_ED25519_HIP_OK;
}

/* pass by pass, as front_items_host; a pass counts the values from the packed copies, the ones the device will read.
   in: off u64 [m], val_first u32 [m+1], sz u32 [m]; out: hashes [nv][32], value codes [nv], packet codes [m] */
int
fd_ed25519_hip_crds_host( fd_ed25519_hip_engine_t * e, unsigned long n, unsigned char const * pkts,
                          unsigned long const * pkt_off, unsigned int const * pkt_sz, unsigned char const self_key[ 32 ],
                          unsigned int * val_first_out, signed char * pkt_out, signed char * val_out,
                          unsigned char * hash_out ) {
  if( !self_key ) return FD_ED25519_HIP_ERR_INVAL;
  if( e && val_first_out ) val_first_out[ 0 ] = 0U;
  hipStream_t st;
  int err = front_begin( e, n, pkts && pkt_off && pkt_sz && val_first_out && pkt_out && val_out, 0UL, NULL, NULL, &st );
  if( err<=0 ) return err;
  uint64_t total = 0UL;
  for( uint64_t base=0UL; base<n; base+=FRONT_HOST_CHUNK ) {
    uint64_t m = n-base<FRONT_HOST_CHUNK ? n-base : FRONT_HOST_CHUNK;
    uint64_t first_at = 8UL*m, sz_at = 12UL*m + 4UL, in_bytes = 16UL*m + 4UL;
    uint64_t out_max = 33UL*m*FD_ED25519_HIP_CRDS_VAL_MAX + m;
    if( (err = front_room( e, m*FD_CRDS_CORE_MAX, in_bytes, out_max )) ) return err;
    uint64_t * h_off   = (uint64_t *)e->h_fr_in;
    uint32_t * h_first = (uint32_t *)( e->h_fr_in + first_at );
    uint32_t * h_sz    = (uint32_t *)( e->h_fr_in + sz_at );
    uint64_t pos = front_pack( e, m, pkts, pkt_off+base, pkt_sz+base, FD_CRDS_CORE_MAX, 0UL, h_off, h_sz );
    uint64_t nv = 0UL;
    for( uint64_t i=0UL; i<m; i++ ) {
      h_first[i] = (uint32_t)nv;
      val_first_out[ base+i ] = (unsigned int)( total + nv );
      /* a packet of more than PACKET_MAX bytes travels as its size alone: the walk rejects the size unread */
      nv += fd_ed25519_hip_crds_count( e->h_msgs + h_off[i], h_sz[i] );
    }
    h_first[m] = (uint32_t)nv;
    val_first_out[ base+m ] = (unsigned int)( total + nv );
    uint64_t hash_bytes = hash_out ? 32UL*nv : 0UL, out_bytes = hash_bytes + nv + m;
    if( (err = grow_dev( &e->d_fr_work, &e->fr_work_cap, FD_ED25519_HIP_CRDS_WORK_BYTES( m, nv ) )) ) return err;
    if( (err = front_upload( e, pos, in_bytes, st )) ) return err;
    err = fd_ed25519_hip_crds_dev( e, m, e->d_msgs, (unsigned long const *)e->d_fr_in,
                                   (unsigned int const *)( e->d_fr_in + sz_at ), pos, self_key,
                                   (unsigned int const *)( e->d_fr_in + first_at ), nv, e->d_fr_work,
                                   (signed char *)( e->d_fr_out + hash_bytes + nv ), (signed char *)( e->d_fr_out + hash_bytes ),
                                   NULL, hash_out ? e->d_fr_out : NULL, st );
    if( err ) return err;
    if( (err = front_download( e, out_bytes, st )) ) return err;
    if( hash_out ) memcpy( hash_out + 32UL*total, e->h_fr_out, hash_bytes );
    memcpy( val_out + total, e->h_fr_out + hash_bytes, nv );
    memcpy( pkt_out + base, e->h_fr_out + hash_bytes + nv, m );
    total += nv;
  }
  return FD_ED25519_HIP_OK;
}

/* ---- sealing a leader's FEC sets (include/fd_ed25519_hip.h Part 2f) ------ */

_Static_assert( FD_ED25519_HIP_FEC_OK==FD_FEC_CORE_OK && FD_ED25519_HIP_FEC_ERR_PARSE==FD_FEC_CORE_ERR_PARSE &&
                FD_ED25519_HIP_FEC_UNSUPPORTED==FD_FEC_CORE_UNSUPPORTED && FD_ED25519_HIP_FEC_ERR_SET==FD_FEC_CORE_ERR_SET &&
                FD_ED25519_HIP_FEC_ERR_SET==FD_ED25519_HIP_SHRED_ERR_HEADER &&
                FD_ED25519_HIP_FEC_SET_MAX==FD_FEC_CORE_CNT_MAX,
                "public and core FEC constants differ" );

/* the rules and the tree the tree kernel runs, on the host (no GPU) */
int
fd_ed25519_hip_fec_root( unsigned char const * shreds, unsigned long const * shred_off, unsigned int const * shred_sz,
                         unsigned long cnt, unsigned char * root, unsigned char * proofs ) {
  if( !root ) return FD_ED25519_HIP_ERR_INVAL;
  return fd_fec_core_root( shreds, shred_off, shred_sz, cnt, root, proofs );
}

int
fd_ed25519_hip_fec_seal_dev( fd_ed25519_hip_engine_t * e, unsigned long n, unsigned char * shreds,
                             unsigned long const * shred_off, unsigned int const * shred_sz, unsigned long n_set,
                             unsigned int const * set_first, unsigned char const * privs, void * work,
                             signed char * set_out, unsigned char * roots, unsigned char * sigs, void * stream ) {
  hipStream_t st;
  /* the batch is its sets: none is a no-op whatever n is; a signature copy needs the keys */
  int err = front_begin( e, n_set, set_first && work && set_out && ( !n || ( shreds && shred_off && shred_sz ) ) &&
                                   n<=UINT32_MAX && n_set<=INT32_MAX && ( privs || !sigs ),
                         (uintptr_t)work | (uintptr_t)privs | (uintptr_t)roots | (uintptr_t)sigs | (uintptr_t)shreds,
                         "shreds/privs/work/roots/sigs", stream, &st );
  if( err<=0 ) return err;
  front_work_t w;
  if( (err = front_work_fits( front_work_fec( work, n, n_set, &w ), FD_ED25519_HIP_FEC_WORK_BYTES( n, n_set ), "fec" )) ) return err;
  /* no set has sealed a shred yet; the scatter reads every shred's entry */
  if( n ) HIPCHK( hipMemsetAsync( w.set_of, 0xFF, 4UL*n, st ), "fec set_of memset" );
  fd_ed25519_fec_tree_params_t tp = { 0 };
  tp.shreds = shreds; tp.shred_off = (uint64_t const *)shred_off; tp.shred_sz = shred_sz; tp.n = n;
  tp.set_first = set_first; tp.n_set = n_set;
  tp.roots = w.roots; tp.msg_off = w.msg_off; tp.msg_sz = w.msg_sz; tp.set_of = w.set_of;
  tp.set_out = (int8_t *)set_out; tp.roots_out = roots;
  HIPCHK( (hipError_t)fd_ed25519_hip_launch_fec_tree( &tp, st ), "fec_tree launch" );
  if( !privs ) return FD_ED25519_HIP_OK;   /* the keyguard split: the caller signs the roots elsewhere */
  fd_ed25519_sign_params_t gp = { 0 };
  gp.msgs = w.roots; gp.msg_off = w.msg_off; gp.msg_sz = w.msg_sz; gp.privs = privs;
  gp.sigs = w.sigs; gp.pubs = w.pubs; gp.n = n_set; gp.btab = e->d_btab;
  HIPCHK( (hipError_t)fd_ed25519_hip_launch_sign( &gp, st ), "fec sign launch" );
  fd_ed25519_fec_scatter_params_t cp = { 0 };
  cp.shreds = shreds; cp.shred_off = (uint64_t const *)shred_off; cp.n = n; cp.n_set = n_set;
  cp.set_of = w.set_of; cp.sigs = w.sigs; cp.set_out = (int8_t const *)set_out; cp.sigs_out = sigs;
  HIPCHK( (hipError_t)fd_ed25519_hip_launch_fec_scatter( &cp, st ), "fec_scatter launch" );
  return FD_ED25519_HIP_OK;
}

/* ---- a pass by sets: what the three FEC-set wrappers do alike (fd_fec_pass.h) -- */

_Static_assert( FD_FEC_PASS_CHUNK==FRONT_HOST_CHUNK, "a pass by sets is bounded as a pass by items" );

typedef struct {
  uint64_t             k1, m, ms;   /* the pass is the sets [k0, k1): ms sets, m shreds */
  fd_fec_pass_in_t     at;          /* its in block */
  fd_fec_pass_staged_t sg;          /* its item staging */
} fec_pass_t;

/* cut, room, stage: the pass from set k0 into the pinned staging, with room for out_per_set bytes a set to come back */
static int
fec_pass_begin( fd_ed25519_hip_engine_t * e, int front, unsigned long n, unsigned char const * shreds,
                unsigned long const * shred_off, unsigned int const * shred_sz, unsigned char const * erased,
                unsigned long n_set, unsigned int const * set_first, unsigned char const * privs, uint64_t k0,
                uint64_t out_per_set, fec_pass_t * ps ) {
  ps->m  = fd_fec_pass_cut( set_first, n_set, n, k0, &ps->k1 );
  ps->ms = ps->k1-k0;
  ps->at = fd_fec_pass_in( ps->m, ps->ms, privs!=NULL, front==FD_FEC_PASS_RECOVER );
  int err = front_room( e, fd_fec_pass_item_bytes( front, ps->m ), ps->at.in_bytes, out_per_set*ps->ms );
  if( err ) return err;
  if( privs ) memcpy( e->h_fr_in + ps->at.keys_at, privs + 32UL*k0, 32UL*ps->ms );
  ps->sg = fd_fec_pass_stage( front, shreds, shred_off, shred_sz, erased, n, set_first, k0, ps->k1, e->h_msgs, e->h_fr_in, &ps->at );
  return FD_ED25519_HIP_OK;
}

/* the pass's arrays on the device, as the *_dev take them */
#define FEC_PASS_D_OFF( e, ps )   ( (unsigned long const *)( (e)->d_fr_in + (ps).at.off_at ) )
#define FEC_PASS_D_FIRST( e, ps ) ( (unsigned int const *)( (e)->d_fr_in + (ps).at.first_at ) )
#define FEC_PASS_D_SZ( e, ps )    ( (unsigned int const *)( (e)->d_fr_in + (ps).at.sz_at ) )

/* the aside slots, which the kernel has filled, back into the pinned staging */
static int
fec_pass_aside_down( fd_ed25519_hip_engine_t * e, fec_pass_t const * ps, hipStream_t st ) {
  if( ps->sg.n_aside )
    HIPCHK( hipMemcpyAsync( e->h_msgs + ps->sg.aside_at, e->d_msgs + ps->sg.aside_at, FD_SHRED_CORE_MAX_SZ*ps->sg.n_aside,
                            hipMemcpyDeviceToHost, st ), "D2H aside shreds" );
  return FD_ED25519_HIP_OK;
}

/* Pass by pass (fd_fec_pass.h): no shred stands aside, all come down.  The
   keys, with privs, stand in front of the in block; out: roots [ms][32],
   sigs [ms][64], codes [ms].  Of a sealed set's shreds the signature (with
   privs) and the proof are copied back, nothing else. */
int
fd_ed25519_hip_fec_seal_host( fd_ed25519_hip_engine_t * e, unsigned long n, unsigned char * shreds,
                              unsigned long const * shred_off, unsigned int const * shred_sz, unsigned long n_set,
                              unsigned int const * set_first, unsigned char const * privs, signed char * set_out,
                              unsigned char * roots, unsigned char * sigs ) {
  hipStream_t st;
  int err = front_begin( e, n_set, set_first && set_out && ( !n || ( shreds && shred_off && shred_sz ) ) && n<=UINT32_MAX &&
                                   ( privs || !sigs ), 0UL, NULL, NULL, &st );
  if( err<=0 ) return err;
  fec_pass_t ps;
  for( uint64_t k0=0UL; k0<n_set; k0=ps.k1 ) {
    if( (err = fec_pass_begin( e, FD_FEC_PASS_SEAL, n, shreds, shred_off, shred_sz, NULL, n_set, set_first, privs, k0, 97UL, &ps )) )
      return err;
    uint64_t ms = ps.ms, sigs_at = 32UL*ms, codes_at = 96UL*ms;
    if( (err = grow_dev( &e->d_fr_work, &e->fr_work_cap, FD_ED25519_HIP_FEC_WORK_BYTES( ps.m, ms ) )) ) return err;
    if( (err = front_upload( e, ps.sg.whole, ps.at.in_bytes, st )) ) return err;
    err = fd_ed25519_hip_fec_seal_dev( e, ps.m, e->d_msgs, FEC_PASS_D_OFF( e, ps ), FEC_PASS_D_SZ( e, ps ), ms,
                                       FEC_PASS_D_FIRST( e, ps ), privs ? e->d_fr_in + ps.at.keys_at : NULL, e->d_fr_work,
                                       (signed char *)( e->d_fr_out + codes_at ), e->d_fr_out,
                                       privs ? e->d_fr_out + sigs_at : NULL, st );
    if( err ) return err;
    if( ps.sg.whole )
      HIPCHK( hipMemcpyAsync( e->h_msgs, e->d_msgs, ps.sg.whole, hipMemcpyDeviceToHost, st ), "D2H sealed shreds" );
    if( (err = front_download( e, 97UL*ms, st )) ) return err;
    memcpy( set_out + k0, e->h_fr_out + codes_at, ms );
    if( roots ) memcpy( roots + 32UL*k0, e->h_fr_out, 32UL*ms );
    if( sigs )  memcpy( sigs  + 64UL*k0, e->h_fr_out + sigs_at, 64UL*ms );
    for( uint64_t k=k0; k<ps.k1; k++ ) {
      if( set_out[k] ) continue;                      /* rule 6 */
      uint64_t first = set_first[k], cnt = set_first[k+1UL]-first, depth = fd_fec_core_depth( (unsigned)cnt );
      for( uint64_t j=0UL; j<cnt; j++ ) {
        unsigned char *       dst = shreds + shred_off[ first+j ];
        unsigned char const * src = e->h_msgs + fd_fec_pass_at( e->h_fr_in, &ps.at, k-k0, j );
        uint64_t proof_at = ( ( src[ 0x40 ] & 0xf0 )==0x80 ? FD_SHRED_CORE_MIN_SZ : FD_SHRED_CORE_MAX_SZ ) - 20UL*depth;
        if( privs ) memcpy( dst, src, 64UL );
        memcpy( dst + proof_at, src + proof_at, 20UL*depth );
      }
    }
  }
  return FD_ED25519_HIP_OK;
}

/* ---- the Reed-Solomon parity of a leader's FEC sets (include/fd_ed25519_hip.h Part 2g) -- */

unsigned long
fd_ed25519_hip_private_reedsol_tab_bytes( void ) { return FD_REEDSOL_CORE_TAB_BYTES; }

void
fd_ed25519_hip_private_reedsol_tables( unsigned char * tab ) { fd_reedsol_core_tables( tab ); }

/* the rules and the code the parity kernel runs, on the host (no GPU) */
int
fd_ed25519_hip_fec_parity( unsigned char * shreds, unsigned long const * shred_off, unsigned int const * shred_sz,
                           unsigned long cnt ) {
  return fd_reedsol_core_encode( shreds, shred_off, shred_sz, cnt );
}

int
fd_ed25519_hip_fec_parity_dev( fd_ed25519_hip_engine_t * e, unsigned long n, unsigned char * shreds,
                               unsigned long const * shred_off, unsigned int const * shred_sz, unsigned long n_set,
                               unsigned int const * set_first, signed char * set_out, void * stream ) {
  hipStream_t st;
  int err = front_begin( e, n_set, set_first && set_out && ( !n || ( shreds && shred_off && shred_sz ) ) &&
                                   n<=UINT32_MAX && n_set<=INT32_MAX, (uintptr_t)shreds, "shreds", stream, &st );
  if( err<=0 ) return err;
  fd_ed25519_fec_parity_params_t pp = { 0 };
  pp.shreds = shreds; pp.shred_off = (uint64_t const *)shred_off; pp.shred_sz = shred_sz; pp.n = n;
  pp.set_first = set_first; pp.n_set = n_set; pp.tab = e->d_rstab; pp.set_out = (int8_t *)set_out;
  HIPCHK( (hipError_t)fd_ed25519_hip_launch_fec_parity( &pp, st ), "fec_parity launch" );
  return FD_ED25519_HIP_OK;
}

/* Pass by pass (fd_fec_pass.h): the code shreds stand aside.  Up go the
   whole shreds as they are and bytes [0, 0x59) of every code shred (one
   strided copy); down come the code shreds.  out: codes [ms].  Of a set with
   code 0 the parity regions of its code shreds are copied back, nothing
   else. */
int
fd_ed25519_hip_fec_parity_host( fd_ed25519_hip_engine_t * e, unsigned long n, unsigned char * shreds,
                                unsigned long const * shred_off, unsigned int const * shred_sz, unsigned long n_set,
                                unsigned int const * set_first, signed char * set_out ) {
  hipStream_t st;
  int err = front_begin( e, n_set, set_first && set_out && ( !n || ( shreds && shred_off && shred_sz ) ) && n<=UINT32_MAX,
                         0UL, NULL, NULL, &st );
  if( err<=0 ) return err;
  fec_pass_t ps;
  for( uint64_t k0=0UL; k0<n_set; k0=ps.k1 ) {
    if( (err = fec_pass_begin( e, FD_FEC_PASS_PARITY, n, shreds, shred_off, shred_sz, NULL, n_set, set_first, NULL, k0, 1UL, &ps )) )
      return err;
    if( (err = front_upload( e, ps.sg.whole, ps.at.in_bytes, st )) ) return err;
    if( ps.sg.n_aside )
      HIPCHK( hipMemcpy2DAsync( e->d_msgs + ps.sg.aside_at, FD_SHRED_CORE_MAX_SZ, e->h_msgs + ps.sg.aside_at, FD_SHRED_CORE_MAX_SZ,
                                FD_SHRED_CORE_CODE_HDR_SZ, ps.sg.n_aside, hipMemcpyHostToDevice, st ), "H2D parity headers" );
    err = fd_ed25519_hip_fec_parity_dev( e, ps.m, e->d_msgs, FEC_PASS_D_OFF( e, ps ), FEC_PASS_D_SZ( e, ps ), ps.ms,
                                         FEC_PASS_D_FIRST( e, ps ), (signed char *)e->d_fr_out, st );
    if( err ) return err;
    if( (err = fec_pass_aside_down( e, &ps, st )) ) return err;
    if( (err = front_download( e, ps.ms, st )) ) return err;
    memcpy( set_out + k0, e->h_fr_out, ps.ms );
    for( uint64_t k=k0; k<ps.k1; k++ ) {
      if( set_out[k] ) continue;                      /* rule 8 */
      uint64_t first = set_first[k], cnt = set_first[k+1UL]-first;
      uint64_t region = FD_REEDSOL_CORE_REGION( fd_fec_core_depth( (unsigned)cnt ) );
      for( uint64_t j=0UL; j<cnt; j++ ) {
        uint64_t at = fd_fec_pass_at( e->h_fr_in, &ps.at, k-k0, j );
        if( at<ps.sg.aside_at ) continue;             /* a data shred: read only */
        memcpy( shreds + shred_off[ first+j ] + FD_SHRED_CORE_CODE_HDR_SZ, e->h_msgs + at + FD_SHRED_CORE_CODE_HDR_SZ, region );
      }
    }
  }
  return FD_ED25519_HIP_OK;
}

/* ---- recovering received FEC sets (include/fd_ed25519_hip.h Part 2h) -- */

_Static_assert( FD_ED25519_HIP_FEC_ERR_PARTIAL==FD_REEDSOL_CORE_ERR_PARTIAL &&
                FD_ED25519_HIP_FEC_ERR_CORRUPT==FD_REEDSOL_CORE_ERR_CORRUPT, "public and core recover codes differ" );

/* the rules and the code the recover kernel runs, on the host (no GPU) */
int
fd_ed25519_hip_fec_recover( unsigned char * shreds, unsigned long const * shred_off, unsigned int const * shred_sz,
                            unsigned char const * erased, unsigned long cnt ) {
  return fd_reedsol_core_recover( shreds, shred_off, shred_sz, erased, cnt );
}

int
fd_ed25519_hip_fec_recover_dev( fd_ed25519_hip_engine_t * e, unsigned long n, unsigned char * shreds,
                                unsigned long const * shred_off, unsigned int const * shred_sz, unsigned char const * erased,
                                unsigned long n_set, unsigned int const * set_first, signed char * set_out, void * stream ) {
  hipStream_t st;
  int err = front_begin( e, n_set, set_first && set_out && ( !n || ( shreds && shred_off && shred_sz && erased ) ) &&
                                   n<=UINT32_MAX && n_set<=INT32_MAX, (uintptr_t)shreds, "shreds", stream, &st );
  if( err<=0 ) return err;
  fd_ed25519_fec_recover_params_t rp = { 0 };
  rp.shreds = shreds; rp.shred_off = (uint64_t const *)shred_off; rp.shred_sz = shred_sz; rp.erased = erased; rp.n = n;
  rp.set_first = set_first; rp.n_set = n_set; rp.tab = e->d_rstab; rp.set_out = (int8_t *)set_out;
  HIPCHK( (hipError_t)fd_ed25519_hip_launch_fec_recover( &rp, st ), "fec_recover launch" );
  return FD_ED25519_HIP_OK;
}

/* Pass by pass (fd_fec_pass.h): the erased slots stand aside, nothing of
   them goes up and all of them come down; the erased flags stand behind the
   in block.  out: codes [ms].  Of a set with code 0 the bytes rule 12 names
   of its erased slots are copied back, nothing else. */
int
fd_ed25519_hip_fec_recover_host( fd_ed25519_hip_engine_t * e, unsigned long n, unsigned char * shreds,
                                 unsigned long const * shred_off, unsigned int const * shred_sz, unsigned char const * erased,
                                 unsigned long n_set, unsigned int const * set_first, signed char * set_out ) {
  hipStream_t st;
  int err = front_begin( e, n_set, set_first && set_out && ( !n || ( shreds && shred_off && shred_sz && erased ) ) &&
                                   n<=UINT32_MAX, 0UL, NULL, NULL, &st );
  if( err<=0 ) return err;
  fec_pass_t ps;
  for( uint64_t k0=0UL; k0<n_set; k0=ps.k1 ) {
    if( (err = fec_pass_begin( e, FD_FEC_PASS_RECOVER, n, shreds, shred_off, shred_sz, erased, n_set, set_first, NULL, k0, 1UL, &ps )) )
      return err;
    if( (err = front_upload( e, ps.sg.whole, ps.at.in_bytes, st )) ) return err;
    err = fd_ed25519_hip_fec_recover_dev( e, ps.m, e->d_msgs, FEC_PASS_D_OFF( e, ps ), FEC_PASS_D_SZ( e, ps ),
                                          e->d_fr_in + ps.at.flags_at, ps.ms, FEC_PASS_D_FIRST( e, ps ), (signed char *)e->d_fr_out, st );
    if( err ) return err;
    if( (err = fec_pass_aside_down( e, &ps, st )) ) return err;
    if( (err = front_download( e, ps.ms, st )) ) return err;
    memcpy( set_out + k0, e->h_fr_out, ps.ms );
    for( uint64_t k=k0; k<ps.k1; k++ ) {
      if( set_out[k] ) continue;                      /* rule 12 */
      uint64_t first = set_first[k], cnt = set_first[k+1UL]-first;
      uint64_t region = FD_REEDSOL_CORE_REGION( fd_fec_core_depth( (unsigned)cnt ) );
      /* code 0: a received code shred has passed the rules, and its data_cnt is the set's */
      uint64_t d = cnt;
      for( uint64_t j=0UL; j<cnt; j++ )
        if( !erased[ first+j ] && ( shreds[ shred_off[ first+j ] + 0x40UL ] & 0xf0 )==0x40 ) {
          d = fd_shred_core_u16( shreds + shred_off[ first+j ] + 0x53UL );
          break;
        }
      for( uint64_t j=0UL; j<cnt; j++ ) {
        if( !erased[ first+j ] ) continue;            /* a received slot: read only */
        unsigned char const * from = e->h_msgs + fd_fec_pass_at( e->h_fr_in, &ps.at, k-k0, j );
        unsigned char *       to   = shreds + shred_off[ first+j ];
        if( j<d ) { memcpy( to, from, 64UL ); memcpy( to + 0x40UL, from + 0x40UL, region ); }
        else      memcpy( to, from, FD_SHRED_CORE_CODE_HDR_SZ + region );
      }
    }
  }
  return FD_ED25519_HIP_OK;
}

/* ---- a block's proof-of-history hash chain (include/fd_ed25519_hip.h Part 2i) -- */

_Static_assert( FD_ED25519_HIP_POH_ERR_PARSE==FD_POH_CORE_ERR_PARSE && FD_ED25519_HIP_POH_UNSUPPORTED==FD_POH_CORE_UNSUPPORTED &&
                FD_ED25519_HIP_POH_ERR_HASH==FD_POH_CORE_ERR_HASH &&
                FD_ED25519_HIP_POH_HASH_CNT_CEIL==FD_POH_CORE_HASH_CNT_CEIL, "public and core PoH constants differ" );

/* the walk and the rules the kernels run, on the host (no GPU) */
int
fd_ed25519_hip_poh_prepare_count( unsigned char const * block, unsigned long block_sz, unsigned long * n,
                                  unsigned long * n_sig ) {
  unsigned long mb = 0UL, sg = 0UL;
  if( !n || !n_sig || ( !block && block_sz ) ) return FD_ED25519_HIP_ERR_INVAL;
  int code = fd_poh_core_walk( block, block_sz, 0UL, 0UL, NULL, NULL, NULL, 0UL, NULL, 0UL, &mb, &sg );
  *n = mb; *n_sig = sg;
  return code;
}

int
fd_ed25519_hip_poh_prepare( unsigned char const * block, unsigned long block_sz, unsigned long first_in_off, unsigned long n,
                            unsigned long n_sig, unsigned long * hdr_off, unsigned long * in_off, unsigned int * sig_first,
                            unsigned long * sig_off ) {
  unsigned long mb, sg;
  if( !sig_first || ( n && ( !hdr_off || !in_off ) ) || ( n_sig && !sig_off ) || ( !block && block_sz ) )
    return FD_ED25519_HIP_ERR_INVAL;
  int code = fd_poh_core_walk( block, block_sz, 0UL, 0UL, NULL, NULL, NULL, 0UL, NULL, 0UL, &mb, &sg );
  if( code ) return code;
  if( mb>n || sg>n_sig ) return FD_ED25519_HIP_ERR_INVAL;
  unsigned long spare_off = 0UL;   /* n == 0: the walk writes sig_first[ 0 ] alone */
  return fd_poh_core_walk( block, block_sz, 0UL, first_in_off, hdr_off ? hdr_off : &spare_off, in_off, sig_first, n, sig_off,
                           n_sig, &mb, &sg );
}

int
fd_ed25519_hip_poh( unsigned char const * buf, unsigned long buf_sz, unsigned long n, unsigned long const * hdr_off,
                    unsigned long const * in_off, unsigned int const * sig_first, unsigned long n_sig,
                    unsigned long const * sig_off, unsigned long hash_cnt_max, signed char * out, unsigned char * out_hash ) {
  if( hash_cnt_max>FD_ED25519_HIP_POH_HASH_CNT_CEIL ) return FD_ED25519_HIP_ERR_INVAL;
  if( !n ) return FD_ED25519_HIP_OK;
  if( !hdr_off || !in_off || !sig_first || !out || ( n_sig && !sig_off ) || ( !buf && buf_sz ) ) return FD_ED25519_HIP_ERR_INVAL;
  for( unsigned long i=0UL; i<n; i++ )
    out[ i ] = (signed char)fd_poh_core_verify( buf, buf_sz, hdr_off[ i ], in_off[ i ], sig_first[ i ], sig_first[ i+1UL ], n_sig,
                                                sig_off, hash_cnt_max, out_hash ? out_hash + 32UL*i : NULL );
  return FD_ED25519_HIP_OK;
}

int
fd_ed25519_hip_poh_dev( fd_ed25519_hip_engine_t * e, unsigned long n, unsigned char const * buf, unsigned long buf_sz,
                        unsigned long const * hdr_off, unsigned long const * in_off, unsigned int const * sig_first,
                        unsigned long n_sig, unsigned long const * sig_off, unsigned long hash_cnt_max, signed char * out,
                        unsigned char * out_hash, void * work, void * stream ) {
  if( hash_cnt_max>FD_ED25519_HIP_POH_HASH_CNT_CEIL ) return FD_ED25519_HIP_ERR_INVAL;   /* of an empty batch too */
  hipStream_t st;
  int err = front_begin( e, n, buf && hdr_off && in_off && sig_first && out && work && ( !n_sig || sig_off ) &&
                               n<=INT32_MAX && n_sig<=UINT32_MAX,
                         (uintptr_t)work | (uintptr_t)out_hash, "poh work/out_hash", stream, &st );
  if( err<=0 ) return err;
  front_work_poh_t w;
  if( (err = front_work_fits( front_work_poh( work, n, n_sig, &w ), FD_ED25519_HIP_POH_WORK_BYTES( n, n_sig ), "poh" )) ) return err;
  fd_ed25519_poh_params_t p = { 0 };
  p.buf = buf; p.buf_sz = buf_sz; p.hdr_off = (uint64_t const *)hdr_off; p.in_off = (uint64_t const *)in_off;
  p.sig_first = sig_first; p.sig_off = (uint64_t const *)sig_off; p.n = n; p.n_sig = n_sig; p.hash_cnt_max = hash_cnt_max;
  p.leaves = w.leaves; p.roots = w.roots; p.pre = w.pre; p.out = (int8_t *)out; p.out_hash = out_hash;
  if( n_sig ) {   /* without signatures no microblock has a tree, and the chain reads neither roots nor pre */
    HIPCHK( (hipError_t)fd_ed25519_hip_launch_poh_leaf( &p, st ), "poh_leaf launch" );
    HIPCHK( (hipError_t)fd_ed25519_hip_launch_poh_tree( &p, st ), "poh_tree launch" );
  }
  HIPCHK( (hipError_t)fd_ed25519_hip_launch_poh_chain( &p, st ), "poh_chain launch" );
  return FD_ED25519_HIP_OK;
}

_Static_assert( FD_POH_PASS_CHUNK==FRONT_HOST_CHUNK, "a pass by microblocks is bounded as a pass by items" );

/* Judge and order, then pass by pass (fd_poh_pass.h): cut, room, stage,
   upload, poh_dev, download, scatter.  extra: the in states an in_off with
   FD_POH_PASS_IN_EXTRA points into (poh_blocks_host's in_hash), or NULL. */
static int
poh_host_impl( fd_ed25519_hip_engine_t * e, hipStream_t st, unsigned long n, unsigned char const * buf, unsigned long buf_sz,
               unsigned long const * hdr_off, unsigned long const * in_off, unsigned int const * sig_first, unsigned long n_sig,
               unsigned long const * sig_off, unsigned char const * extra, unsigned long hash_cnt_max, signed char * out,
               unsigned char * out_hash ) {
  fd_poh_pass_ord_t * ord = (fd_poh_pass_ord_t *)malloc( n*sizeof(fd_poh_pass_ord_t) );
  if( !ord ) { fd_ed25519_hip_private_set_errorf( "malloc failed" ); return FD_ED25519_HIP_ERR_NOMEM; }
  uint64_t go = fd_poh_pass_order( buf, buf_sz, n, hdr_off, in_off, sig_first, n_sig, sig_off, extra, hash_cnt_max, out, out_hash, ord );
  int err = FD_ED25519_HIP_OK;
  for( uint64_t a=0UL, b; a<go; a=b ) {
    uint64_t ns;
    b = fd_poh_pass_cut( ord, go, sig_first, a, &ns );
    uint64_t m = b-a;
    fd_poh_pass_blocks_t at = fd_poh_pass_blocks( m, ns );
    if( (err = front_room( e, at.item_bytes, at.in_bytes, at.out_bytes )) ) break;
    if( (err = grow_dev( &e->d_fr_work, &e->fr_work_cap, FD_ED25519_HIP_POH_WORK_BYTES( m, ns ) )) ) break;
    fd_poh_pass_stage( buf, hdr_off, in_off, sig_first, sig_off, extra, ord+a, m, &at, e->h_msgs, e->h_fr_in );
    if( (err = front_upload( e, at.item_bytes, at.in_bytes, st )) ) break;
    err = fd_ed25519_hip_poh_dev( e, m, e->d_msgs, at.item_bytes, (unsigned long const *)( e->d_fr_in + at.hdr_at ),
                                  (unsigned long const *)( e->d_fr_in + at.in_at ), (unsigned int const *)( e->d_fr_in + at.first_at ),
                                  ns, (unsigned long const *)( e->d_fr_in + at.sig_at ), hash_cnt_max,
                                  (signed char *)( e->d_fr_out + at.codes_at ), e->d_fr_out + at.states_at, e->d_fr_work, st );
    if( err ) break;
    if( (err = front_download( e, at.out_bytes, st )) ) break;
    fd_poh_pass_scatter( ord+a, m, &at, e->h_fr_out, out, out_hash );
  }
  free( ord );
  return err;
}

int
fd_ed25519_hip_poh_host( fd_ed25519_hip_engine_t * e, unsigned long n, unsigned char const * buf, unsigned long buf_sz,
                         unsigned long const * hdr_off, unsigned long const * in_off, unsigned int const * sig_first,
                         unsigned long n_sig, unsigned long const * sig_off, unsigned long hash_cnt_max, signed char * out,
                         unsigned char * out_hash ) {
  if( hash_cnt_max>FD_ED25519_HIP_POH_HASH_CNT_CEIL ) return FD_ED25519_HIP_ERR_INVAL;
  hipStream_t st;
  int err = front_begin( e, n, buf && hdr_off && in_off && sig_first && out && ( !n_sig || sig_off ) && n<=INT32_MAX &&
                               n_sig<=UINT32_MAX, 0UL, NULL, NULL, &st );
  if( err<=0 ) return err;
  return poh_host_impl( e, st, n, buf, buf_sz, hdr_off, in_off, sig_first, n_sig, sig_off, NULL, hash_cnt_max, out, out_hash );
}

int
fd_ed25519_hip_poh_blocks_host( fd_ed25519_hip_engine_t * e, unsigned long nb, unsigned char const * blocks,
                                unsigned long const * block_off, unsigned long const * block_sz, unsigned char const * in_hash,
                                unsigned long hash_cnt_max, signed char * block_out, unsigned int * first_bad,
                                unsigned char * out_hash ) {
  if( hash_cnt_max>FD_ED25519_HIP_POH_HASH_CNT_CEIL ) return FD_ED25519_HIP_ERR_INVAL;
  hipStream_t st;
  int err = front_begin( e, nb, blocks && block_off && block_sz && in_hash && block_out && first_bad && out_hash, 0UL, NULL,
                         NULL, &st );
  if( err<=0 ) return err;
  err = FD_ED25519_HIP_OK;
  /* the walk, twice: the counts, then the arrays.  mb_at[ b ]: block b's first microblock; a block that did not walk
     has none */
  uint64_t * mb_at = (uint64_t *)malloc( ( nb+1UL )*sizeof(uint64_t) );
  if( !mb_at ) { fd_ed25519_hip_private_set_errorf( "malloc failed" ); return FD_ED25519_HIP_ERR_NOMEM; }
  uint64_t n = 0UL, n_sig = 0UL, end = 0UL;
  for( uint64_t b=0UL; b<nb; b++ ) {
    unsigned long mb = 0UL, sg = 0UL;
    int code = fd_poh_core_walk( blocks + block_off[ b ], block_sz[ b ], 0UL, 0UL, NULL, NULL, NULL, 0UL, NULL, 0UL, &mb, &sg );
    if( code || !mb ) { mb = 0UL; sg = 0UL; }
    mb_at[ b ] = n;
    n += mb; n_sig += sg;
    if( mb && block_off[ b ]+block_sz[ b ]>end ) end = block_off[ b ]+block_sz[ b ];
  }
  mb_at[ nb ] = n;
  if( n>INT32_MAX || n_sig>UINT32_MAX ) { free( mb_at ); return FD_ED25519_HIP_ERR_INVAL; }
  unsigned long * hdr_off   = (unsigned long *)malloc( ( n ? n : 1UL )*sizeof(unsigned long) );
  unsigned long * in_off    = (unsigned long *)malloc( ( n ? n : 1UL )*sizeof(unsigned long) );
  unsigned int *  sig_first = (unsigned int *) malloc( ( n+1UL )*sizeof(unsigned int) );
  unsigned long * sig_off   = (unsigned long *)malloc( ( n_sig ? n_sig : 1UL )*sizeof(unsigned long) );
  signed char *   out       = (signed char *)  malloc( n ? n : 1UL );
  if( !hdr_off || !in_off || !sig_first || !sig_off || !out ) {
    fd_ed25519_hip_private_set_errorf( "malloc failed" );
    err = FD_ED25519_HIP_ERR_NOMEM;
  }
  uint64_t sg_at = 0UL;
  for( uint64_t b=0UL; b<nb && !err; b++ ) {
    uint64_t m0 = mb_at[ b ], mb_cnt = mb_at[ b+1UL ]-m0;
    if( !mb_cnt ) continue;
    unsigned long mb, sg;
    /* sig_first comes back relative to the block's first signature; the block's last element is the next one's first */
    fd_poh_core_walk( blocks + block_off[ b ], block_sz[ b ], block_off[ b ], FD_POH_PASS_IN_EXTRA | ( 32UL*b ), hdr_off + m0, in_off + m0,
                      sig_first + m0, mb_cnt, sig_off + sg_at, n_sig-sg_at, &mb, &sg );
    for( uint64_t i=m0; i<m0+mb_cnt; i++ ) sig_first[ i ] += (unsigned int)sg_at;
    sg_at += sg;
  }
  if( !err ) {
    sig_first[ n ] = (unsigned int)n_sig;
    if( n ) err = poh_host_impl( e, st, n, blocks, end, hdr_off, in_off, sig_first, n_sig, sig_off, in_hash, hash_cnt_max, out,
                                 NULL );
  }
  /* fd_runtime_block_verify_tpool's reduction */
  for( uint64_t b=0UL; b<nb && !err; b++ ) {
    uint64_t m0 = mb_at[ b ], m1 = mb_at[ b+1UL ];
    first_bad[ b ] = 0xFFFFFFFFU;
    if( m0==m1 ) {
      block_out[ b ] = FD_ED25519_HIP_POH_ERR_PARSE;
      memset( out_hash + 32UL*b, 0, 32UL );
      continue;
    }
    int any_hash = 0, any_unsup = 0;
    for( uint64_t i=m1; i>m0; i-- )
      if( out[ i-1UL ] ) {
        first_bad[ b ] = (unsigned int)( i-1UL-m0 );
        any_hash  |= out[ i-1UL ]==FD_ED25519_HIP_POH_ERR_HASH;
        any_unsup |= out[ i-1UL ]==FD_ED25519_HIP_POH_UNSUPPORTED;
      }
    block_out[ b ] = (signed char)( any_hash ? FD_ED25519_HIP_POH_ERR_HASH : any_unsup ? FD_ED25519_HIP_POH_UNSUPPORTED : 0 );
    memcpy( out_hash + 32UL*b, blocks + hdr_off[ m1-1UL ] + 8UL, 32UL );
  }
  free( mb_at ); free( hdr_off ); free( in_off ); free( sig_first ); free( sig_off ); free( out );
  return err;
}


/* ---- shredding entry batches (include/fd_ed25519_hip.h Part 2j) -- */

_Static_assert( FD_ED25519_HIP_SHREDDER_OK==FD_SHREDDER_CORE_OK && FD_ED25519_HIP_SHREDDER_ERR_BATCH==FD_SHREDDER_CORE_ERR_BATCH &&
                FD_ED25519_HIP_SHREDDER_BAD_RESERVATION==FD_SHREDDER_CORE_BAD_RESERVATION,
                "public and core shredder codes differ" );
_Static_assert( sizeof(fd_ed25519_hip_shredder_batch_t)==24UL && sizeof(fd_shredder_core_desc_t)==24UL &&
                offsetof( fd_ed25519_hip_shredder_batch_t, data_idx      )==offsetof( fd_shredder_core_desc_t, data_idx       ) &&
                offsetof( fd_ed25519_hip_shredder_batch_t, parity_idx    )==offsetof( fd_shredder_core_desc_t, parity_idx     ) &&
                offsetof( fd_ed25519_hip_shredder_batch_t, version       )==offsetof( fd_shredder_core_desc_t, version        ) &&
                offsetof( fd_ed25519_hip_shredder_batch_t, parent_off    )==offsetof( fd_shredder_core_desc_t, parent_off     ) &&
                offsetof( fd_ed25519_hip_shredder_batch_t, reference_tick)==offsetof( fd_shredder_core_desc_t, reference_tick ) &&
                offsetof( fd_ed25519_hip_shredder_batch_t, block_complete)==offsetof( fd_shredder_core_desc_t, block_complete ),
                "public and core batch descriptors differ" );

/* the counts and the layout the kernel runs, on the host (no GPU) */
int
fd_ed25519_hip_shredder_count( unsigned long sz, unsigned long * n_set, unsigned long * n_data, unsigned long * n_parity ) {
  if( !n_set || !n_data || !n_parity ) return FD_ED25519_HIP_ERR_INVAL;
  fd_shredder_core_count( sz, n_set, n_data, n_parity );
  return FD_ED25519_HIP_OK;
}

int
fd_ed25519_hip_shredder( unsigned char const * batch, unsigned long sz, fd_ed25519_hip_shredder_batch_t const * desc,
                         unsigned char * shreds, unsigned long const * shred_off, unsigned int * shred_sz,
                         unsigned int * set_first ) {
  if( !sz ) return FD_ED25519_HIP_SHREDDER_ERR_BATCH;
  if( !batch || !desc || !shreds || !shred_off || !shred_sz || !set_first ) return FD_ED25519_HIP_ERR_INVAL;
  return fd_shredder_core_batch( batch, sz, (fd_shredder_core_desc_t const *)desc, shreds, shred_off, shred_sz, set_first );
}

/* The front's launch behind the memset of its shred_sz and, with work, the
   parity and the seal over the same arrays on the same stream.  work: the
   sets' keys [set_cnt][32], the seal's workspace, the parity's codes
   [set_cnt] -- FD_ED25519_HIP_SHREDDER_WORK_BYTES( m, set_cnt ).  With
   parity_out the parity's codes go there instead, for a caller who reads them. */
static int
shredder_run( fd_ed25519_hip_engine_t * e, fd_ed25519_shredder_params_t * sp, void * work, signed char * parity_out,
              signed char * set_out, unsigned char * roots, unsigned char * sigs, hipStream_t st ) {
  uint64_t m = sp->m, ms = sp->set_cnt;
  uint8_t * keys = (uint8_t *)work, * fec_work = work ? keys + 32UL*ms : NULL;
  uint8_t * pcodes = parity_out ? (uint8_t *)parity_out : work ? fec_work + FD_ED25519_HIP_FEC_WORK_BYTES( m, ms ) : NULL;
  int err;
  if( work && (err = front_work_fits( 32UL*ms + FD_ED25519_HIP_FEC_WORK_BYTES( m, ms ) + ms,
                                      FD_ED25519_HIP_SHREDDER_WORK_BYTES( m, ms ), "shredder" )) ) return err;
  /* a shred no set writes has size 0: the parity and the seal judge it without reading it */
  if( m ) HIPCHK( hipMemsetAsync( sp->shred_sz, 0, 4UL*m, st ), "shredder shred_sz memset" );
  sp->keys = sp->privs ? keys : NULL;
  HIPCHK( (hipError_t)fd_ed25519_hip_launch_shredder( sp, st ), "shredder launch" );
  if( !work ) return FD_ED25519_HIP_OK;
  if( (err = fd_ed25519_hip_fec_parity_dev( e, m, sp->shreds, (unsigned long const *)sp->shred_off, sp->shred_sz, ms, sp->set_first,
                                            (signed char *)pcodes, st )) ) return err;
  return fd_ed25519_hip_fec_seal_dev( e, m, sp->shreds, (unsigned long const *)sp->shred_off, sp->shred_sz, ms, sp->set_first,
                                      sp->privs ? keys : NULL, fec_work, set_out, roots, sigs, st );
}

static int
shredder_dev_impl( fd_ed25519_hip_engine_t * e, unsigned long nb, unsigned char const * buf, unsigned long buf_sz,
                   unsigned long const * batch_off, unsigned int const * batch_sz, fd_ed25519_hip_shredder_batch_t const * desc,
                   unsigned int const * set_first_b, unsigned int const * shred_first_b, unsigned long n_set, unsigned long n,
                   unsigned char * shreds, unsigned long base_off, unsigned long stride, unsigned long * shred_off,
                   unsigned int * shred_sz, unsigned int * set_first, signed char * batch_out, int seal,
                   unsigned char const * privs, void * work, signed char * set_out, unsigned char * roots, unsigned char * sigs,
                   void * stream ) {
  hipStream_t st;
  int args_ok = buf && batch_off && batch_sz && desc && set_first_b && shred_first_b && set_first && batch_out &&
                ( !n || ( shreds && shred_off && shred_sz ) ) && stride>=FD_SHRED_CORE_MAX_SZ && n<=UINT32_MAX && n_set<=INT32_MAX &&
                nb<=INT32_MAX && !( (uintptr_t)desc & 7UL ) && ( !seal || ( work && set_out && ( privs || !sigs ) ) );
  int err = front_begin( e, nb, args_ok, seal ? ( (uintptr_t)work | (uintptr_t)privs | (uintptr_t)roots | (uintptr_t)sigs |
                                                  (uintptr_t)shreds ) : 0UL, "shreds/privs/work/roots/sigs", stream, &st );
  if( err<=0 ) return err;
  fd_ed25519_shredder_params_t sp = { 0 };
  sp.buf = buf; sp.buf_sz = buf_sz; sp.batch_off = (uint64_t const *)batch_off; sp.batch_sz = batch_sz; sp.desc = desc;
  sp.set_first_b = set_first_b; sp.shred_first_b = shred_first_b; sp.nb = nb; sp.n_set = n_set; sp.n = n;
  sp.set0 = 0UL; sp.set_cnt = n_set; sp.shred0 = 0UL; sp.m = n; sp.skip_b = UINT64_MAX; sp.skip = 0UL;
  sp.shreds = shreds; sp.base_off = base_off; sp.stride = stride; sp.shred_off = (uint64_t *)shred_off; sp.shred_sz = shred_sz;
  sp.set_first = set_first; sp.batch_out = (int8_t *)batch_out; sp.privs = seal ? privs : NULL;
  return shredder_run( e, &sp, seal ? work : NULL, NULL, set_out, roots, sigs, st );
}

int
fd_ed25519_hip_shredder_front_dev( fd_ed25519_hip_engine_t * e, unsigned long nb, unsigned char const * buf, unsigned long buf_sz,
                                   unsigned long const * batch_off, unsigned int const * batch_sz,
                                   fd_ed25519_hip_shredder_batch_t const * desc, unsigned int const * set_first_b,
                                   unsigned int const * shred_first_b, unsigned long n_set, unsigned long n,
                                   unsigned char * shreds, unsigned long base_off, unsigned long stride,
                                   unsigned long * shred_off, unsigned int * shred_sz, unsigned int * set_first,
                                   signed char * batch_out, void * stream ) {
  return shredder_dev_impl( e, nb, buf, buf_sz, batch_off, batch_sz, desc, set_first_b, shred_first_b, n_set, n, shreds, base_off,
                            stride, shred_off, shred_sz, set_first, batch_out, 0, NULL, NULL, NULL, NULL, NULL, stream );
}

int
fd_ed25519_hip_shredder_dev( fd_ed25519_hip_engine_t * e, unsigned long nb, unsigned char const * buf, unsigned long buf_sz,
                             unsigned long const * batch_off, unsigned int const * batch_sz,
                             fd_ed25519_hip_shredder_batch_t const * desc, unsigned int const * set_first_b,
                             unsigned int const * shred_first_b, unsigned long n_set, unsigned long n, unsigned char * shreds,
                             unsigned long base_off, unsigned long stride, unsigned long * shred_off, unsigned int * shred_sz,
                             unsigned int * set_first, signed char * batch_out, unsigned char const * privs, void * work,
                             signed char * set_out, unsigned char * roots, unsigned char * sigs, void * stream ) {
  return shredder_dev_impl( e, nb, buf, buf_sz, batch_off, batch_sz, desc, set_first_b, shred_first_b, n_set, n, shreds, base_off,
                            stride, shred_off, shred_sz, set_first, batch_out, 1, privs, work, set_out, roots, sigs, stream );
}

/* The reservation, then pass by pass (fd_shredder_pass.h): cut, room, stage,
   upload, front, parity and seal, download, copy back.  The parity's and the
   seal's codes of every set come down with the shreds, and any of them fails
   the call. */
int
fd_ed25519_hip_shredder_host( fd_ed25519_hip_engine_t * e, unsigned long nb, unsigned char const * batches,
                              unsigned long const * batch_off, unsigned int const * batch_sz,
                              fd_ed25519_hip_shredder_batch_t const * desc, unsigned char const * privs,
                              unsigned char * shreds_out, unsigned long stride, unsigned int * shred_sz_out,
                              unsigned int * set_first_out, signed char * batch_out, unsigned char * roots, unsigned char * sigs ) {
  hipStream_t st;
  int err = front_begin( e, nb, batches && batch_off && batch_sz && desc && shreds_out && shred_sz_out && set_first_out &&
                                batch_out && stride>=FD_SHRED_CORE_MAX_SZ && nb<=INT32_MAX && ( privs || !sigs ),
                         0UL, NULL, NULL, &st );
  if( err<=0 ) return err;
  err = FD_ED25519_HIP_OK;   /* a call of zero-size batches alone has no pass to set it */
  uint32_t * gs = (uint32_t *)malloc( 2UL*sizeof(uint32_t)*( nb+1UL ) ), * gh = gs ? gs + nb + 1UL : NULL;
  if( !gs ) { fd_ed25519_hip_private_set_errorf( "malloc failed" ); return FD_ED25519_HIP_ERR_NOMEM; }
  uint64_t N, M;
  if( fd_shredder_pass_reserve( batch_sz, nb, gs, gh, batch_out, &N, &M ) ) { free( gs ); return FD_ED25519_HIP_ERR_INVAL; }
  set_first_out[0] = 0U;
  fd_shredder_pass_cur_t cur = { 0UL, 0UL, 0UL, 0UL };
  while( cur.k<N ) {
    fd_shredder_pass_t     ps = fd_shredder_pass_cut( batch_sz, gs, N, &cur, set_first_out );
    fd_shredder_pass_in_t  at = fd_shredder_pass_in( &ps, privs!=NULL );
    fd_shredder_pass_out_t ot = fd_shredder_pass_out( ps.ms );
    if( (err = front_room( e, at.item_bytes, at.total, ot.out_bytes )) ) break;
    if( (err = grow_dev( &e->d_fr_work, &e->fr_work_cap, FD_ED25519_HIP_SHREDDER_WORK_BYTES( ps.m, ps.ms ) )) ) break;
    uint64_t skip = fd_shredder_pass_stage( batches, batch_off, batch_sz, (fd_shredder_core_desc_t const *)desc, privs, gs, gh, &ps,
                                            &at, e->h_msgs, e->h_fr_in );
    if( (err = front_upload( e, ps.bytes, at.in_bytes, st )) ) break;
    fd_ed25519_shredder_params_t sp = { 0 };
    sp.buf = e->d_msgs; sp.buf_sz = UINT64_MAX; sp.batch_off = (uint64_t const *)( e->d_fr_in + at.off_at );
    sp.batch_sz = (uint32_t const *)( e->d_fr_in + at.sz_at ); sp.desc = e->d_fr_in + at.desc_at;
    sp.set_first_b = (uint32_t const *)( e->d_fr_in + at.sfb_at ); sp.shred_first_b = (uint32_t const *)( e->d_fr_in + at.hfb_at );
    sp.nb = ps.nbp; sp.n_set = N; sp.n = M; sp.set0 = ps.k; sp.set_cnt = ps.ms; sp.shred0 = ps.h; sp.m = ps.m;
    sp.skip_b = 0UL; sp.skip = skip;
    sp.shreds = e->d_msgs; sp.base_off = at.shreds_at; sp.stride = FD_SHRED_CORE_MAX_SZ;
    sp.shred_off = (uint64_t *)( e->d_fr_in + at.shred_off_at ); sp.shred_sz = (uint32_t *)( e->d_fr_in + at.shred_sz_at );
    sp.set_first = (uint32_t *)( e->d_fr_in + at.set_first_at ); sp.batch_out = NULL;
    sp.privs = privs ? e->d_fr_in + at.keys_at : NULL;
    if( (err = shredder_run( e, &sp, e->d_fr_work, (signed char *)( e->d_fr_out + ot.pcodes_at ),
                             (signed char *)( e->d_fr_out + ot.codes_at ), e->d_fr_out + ot.roots_at,
                             privs ? e->d_fr_out + ot.sigs_at : NULL, st )) ) break;
    HIPCHK( hipMemcpyAsync( e->h_msgs + at.shreds_at, e->d_msgs + at.shreds_at, at.shred_bytes, hipMemcpyDeviceToHost, st ),
            "D2H shreds" );
    if( (err = front_download( e, ot.out_bytes, st )) ) break;
    for( uint64_t i=0UL; i<ps.ms && !err; i++ )
      if( e->h_fr_out[ ot.pcodes_at+i ] || e->h_fr_out[ ot.codes_at+i ] ) {
        fd_ed25519_hip_private_set_errorf( "shredder: set %lu got parity code %d, seal code %d", (unsigned long)( ps.k+i ),
                                           (int)(int8_t)e->h_fr_out[ ot.pcodes_at+i ], (int)(int8_t)e->h_fr_out[ ot.codes_at+i ] );
        err = FD_ED25519_HIP_ERR_INVAL;
      }
    if( err ) break;
    if( roots ) memcpy( roots + 32UL*ps.k, e->h_fr_out + ot.roots_at, 32UL*ps.ms );
    if( sigs )  memcpy( sigs  + 64UL*ps.k, e->h_fr_out + ot.sigs_at,  64UL*ps.ms );
    fd_shredder_pass_copy_back( e->h_msgs + at.shreds_at, ps.m, shreds_out + stride*ps.h, stride, shred_sz_out + ps.h );
  }
  free( gs );
  return err;
}
