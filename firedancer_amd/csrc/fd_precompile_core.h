/* fd_precompile_core.h -- the offsets walk of the Ed25519 precompile
   (fd_precompile_ed25519_verify) restated once, compiled three ways: into
   the host library (host/fd_ed25519_hip_fronts.c, gcc), into the device
   staging kernel (fd_ed25519_txn.hip, hipcc) and into the hostile
   input test's stand-alone program (tests/precompile_walk_main.c, gcc with
   sanitizers), so all three lay out exactly the same entries.  Include
   after fd_txn_parse_core.h (FD_TXN_FN, fd_txn_core_cu16,
   fd_ed25519_hip_txn_t).

   Reference: src/flamenco/runtime/program/fd_precompiles.c:72-109 (the
   cross-instruction lookup) and :115-200 (the Ed25519 precompile); the
   dispatch by program account key, src/flamenco/runtime/fd_executor.c:64.
   Rules, for a payload fd_txn_core_parse accepted:

     an instruction counts iff the 32 bytes at acct_addr_off + 32 program_id
       equal the Ed25519 program id; every other instruction is ignored
     header (:130-146), data / data_sz the instruction's data:
       data_sz < 16: success with no entry iff data_sz==2 && data[0]==0,
                     else INSTR_DATA_SIZE
       cnt = data[0]; cnt==0 or data_sz < 2 + 14 cnt: INSTR_DATA_SIZE
       (data[1] is ignored)
     entry i < cnt (:148-197): seven little-endian u16 at data + 2 + 14 i:
       sig_offset, sig_instr_idx, pubkey_offset, pubkey_instr_idx,
       msg_offset, msg_data_sz, msg_instr_idx
     lookup of (idx, offset, size) (:72-109): idx 0xFFFF is this
       instruction's data, any other idx must be < instr_cnt and selects
       that instruction's data; offset + size <= that data_sz (no wrap: both
       are below 2^16); a failed lookup of the signature (64 B), the key
       (32 B) or the message (msg_data_sz B) is DATA_OFFSET

   The walk reads no byte the parser or a check above has not proved
   present: the instruction list is re-walked inside what the parser
   accepted, data[0] only once data_sz allows it, an entry's 14 bytes only
   below 2 + 14 cnt <= data_sz.

   The instruction table (data offset and size of every instruction, for
   the lookups by index) is built once per transaction into caller
   storage, entry j at tab[ j*stride ]: the host keeps 64 words on its
   stack (stride 1), the device kernel a column of LDS per lane (stride =
   the block size). */
#ifndef FD_PRECOMPILE_CORE_H
#define FD_PRECOMPILE_CORE_H

#define FD_PRECOMPILE_CORE_ERR_SIGNATURE       (-3)   /* fd_executor.h:93-95 */
#define FD_PRECOMPILE_CORE_ERR_DATA_OFFSET     (-4)
#define FD_PRECOMPILE_CORE_ERR_INSTR_DATA_SIZE (-5)

#define FD_PRECOMPILE_CORE_DATA_START 16UL   /* 2 + one 14-byte entry */
#define FD_PRECOMPILE_CORE_ENT_SZ     14UL
#define FD_PRECOMPILE_CORE_ENT_MAX    87UL   /* (1232-2)/14: the entries of one transaction's passing headers */
#define FD_PRECOMPILE_CORE_THIS_INSTR 0xFFFFU

/* tab word: data_off in the low half, data_sz in the high half (both at
   most the 1232-byte MTU) */
#define FD_PRECOMPILE_CORE_TAB_OFF( w ) ( (w) & 0xFFFFU )
#define FD_PRECOMPILE_CORE_TAB_SZ( w )  ( (w) >> 16 )

/* one entry of the walk; offsets are relative to the payload and 0 (with
   msg_sz 0) when pre is not 0 */
typedef struct {
  unsigned char  instr;     /* index of the precompile instruction that lists it */
  signed char    pre;       /* 0, or FD_PRECOMPILE_CORE_ERR_DATA_OFFSET */
  unsigned short sig_off;
  unsigned short pub_off;
  unsigned short msg_off;
  unsigned short msg_sz;
} fd_precompile_core_ent_t;

/* base58 Ed25519SigVerify111111111111111111111111111 */
FD_TXN_FN int
fd_precompile_core_is_ed25519( unsigned char const * key ) {
  /* compared byte by byte: an account key starts at any byte of the payload */
  const unsigned char id[ 32 ] = {
    0x03,0x7d,0x46,0xd6,0x7c,0x93,0xfb,0xbe, 0x12,0xf9,0x42,0x8f,0x83,0x8d,0x40,0xff,
    0x05,0x70,0x74,0x49,0x27,0xf4,0x8a,0x64, 0xfc,0xca,0x70,0x44,0x80,0x00,0x00,0x00 };
  unsigned diff = 0U;
  for( int i=0; i<32; i++ ) diff |= (unsigned)( key[ i ] ^ id[ i ] );
  return !diff;
}

/* Re-walks the instruction list of an accepted payload from
   recent_blockhash_off + 32 into tab; returns the mask of the Ed25519
   precompile instructions (bit j: instruction j; at most 64). */
FD_TXN_FN unsigned long
fd_precompile_core_table( unsigned char const * p, fd_ed25519_hip_txn_t const * tx, unsigned * tab,
                          unsigned long stride ) {
  unsigned long i = (unsigned long)tx->recent_blockhash_off + 32UL, mask = 0UL;
  unsigned v = 0U;
  /* the parser accepted every compact-u16 and length below, so `avail` only
     has to admit the longest encoding */
  i += fd_txn_core_cu16( p + i, 3UL, &v );                            /* instr_cnt */
  for( unsigned j=0U; j<(unsigned)tx->instr_cnt; j++ ) {
    unsigned prog = p[ i++ ];
    i += fd_txn_core_cu16( p + i, 3UL, &v );  i += v;                  /* account indices */
    i += fd_txn_core_cu16( p + i, 3UL, &v );                           /* data */
    tab[ j*stride ] = (unsigned)i | ( v << 16 );
    i += v;
    if( fd_precompile_core_is_ed25519( p + tx->acct_addr_off + 32UL*prog ) ) mask |= 1UL << j;
  }
  return mask;
}

/* The header of one precompile instruction: the entry count (1..255) when
   it passes with entries, 0 when it passes with none (the 2-byte form),
   FD_PRECOMPILE_CORE_ERR_INSTR_DATA_SIZE when it fails. */
FD_TXN_FN int
fd_precompile_core_header( unsigned char const * data, unsigned data_sz ) {
  if( data_sz<FD_PRECOMPILE_CORE_DATA_START )                                            /* :130-135 */
    return ( data_sz==2U && data[ 0 ]==0 ) ? 0 : FD_PRECOMPILE_CORE_ERR_INSTR_DATA_SIZE;
  unsigned cnt = data[ 0 ];
  if( !cnt ) return FD_PRECOMPILE_CORE_ERR_INSTR_DATA_SIZE;                              /* :138 */
  if( data_sz < 2U + (unsigned)FD_PRECOMPILE_CORE_ENT_SZ*cnt ) return FD_PRECOMPILE_CORE_ERR_INSTR_DATA_SIZE;  /* :144 */
  return (int)cnt;
}

/* One lookup: the payload offset of (idx, offset, size), or -1. */
FD_TXN_FN int
fd_precompile_core_lookup( unsigned const * tab, unsigned long stride, unsigned instr_cnt, unsigned self,
                           unsigned idx, unsigned offset, unsigned size ) {
  if( idx==FD_PRECOMPILE_CORE_THIS_INSTR ) idx = self;                                   /* :86 */
  else if( idx>=instr_cnt ) return -1;                                                   /* :95 */
  unsigned w = tab[ idx*stride ];
  if( offset + size > FD_PRECOMPILE_CORE_TAB_SZ( w ) ) return -1;                        /* :104 */
  return (int)( FD_PRECOMPILE_CORE_TAB_OFF( w ) + offset );
}

/* Entry i of precompile instruction j (whose header passed with more than
   i entries). */
FD_TXN_FN void
fd_precompile_core_entry( unsigned char const * p, unsigned const * tab, unsigned long stride, unsigned instr_cnt,
                          unsigned j, unsigned i, fd_precompile_core_ent_t * ent ) {
  unsigned char const * e = p + FD_PRECOMPILE_CORE_TAB_OFF( tab[ j*stride ] ) + 2UL + FD_PRECOMPILE_CORE_ENT_SZ*i;
  unsigned f[ 7 ];
  for( int q=0; q<7; q++ ) f[ q ] = (unsigned)e[ 2*q ] | ( (unsigned)e[ 2*q+1 ] << 8 );
  int s = fd_precompile_core_lookup( tab, stride, instr_cnt, j, f[ 1 ], f[ 0 ], 64U );
  int k = fd_precompile_core_lookup( tab, stride, instr_cnt, j, f[ 3 ], f[ 2 ], 32U );
  int m = fd_precompile_core_lookup( tab, stride, instr_cnt, j, f[ 6 ], f[ 4 ], f[ 5 ] );
  int ok = ( s>=0 ) & ( k>=0 ) & ( m>=0 );
  ent->instr   = (unsigned char)j;
  ent->pre     = (signed char)( ok ? 0 : FD_PRECOMPILE_CORE_ERR_DATA_OFFSET );
  ent->sig_off = (unsigned short)( ok ? s : 0 );
  ent->pub_off = (unsigned short)( ok ? k : 0 );
  ent->msg_off = (unsigned short)( ok ? m : 0 );
  ent->msg_sz  = (unsigned short)( ok ? f[ 5 ] : 0U );
}

/* The walk's summary: the reservation count (the sum of cnt over the
   precompile instructions whose header passes) and the first instruction
   whose header fails (0xFF: none) with the number of entries before it. */
typedef struct {
  unsigned      ent_cnt;
  unsigned char hdr_instr;
  unsigned char hdr_pos;
} fd_precompile_core_sum_t;

FD_TXN_FN void
fd_precompile_core_summary( unsigned char const * p, unsigned const * tab, unsigned long stride, unsigned instr_cnt,
                            unsigned long mask, fd_precompile_core_sum_t * s ) {
  s->ent_cnt = 0U; s->hdr_instr = 0xFF; s->hdr_pos = 0;
  for( unsigned j=0U; j<instr_cnt; j++ ) {
    if( !( ( mask >> j ) & 1UL ) ) continue;
    unsigned w = tab[ j*stride ];
    int h = fd_precompile_core_header( p + FD_PRECOMPILE_CORE_TAB_OFF( w ), FD_PRECOMPILE_CORE_TAB_SZ( w ) );
    if( h<0 ) {
      if( s->hdr_instr==0xFF ) { s->hdr_instr = (unsigned char)j; s->hdr_pos = (unsigned char)s->ent_cnt; }
    } else s->ent_cnt += (unsigned)h;
  }
}

/* The whole walk of one payload on a CPU (the library's precompile_count
   and precompile_plan, and the hostile-input program): parses, fills sum,
   writes the first cap entries in instruction then entry order and
   returns how many it wrote.  *parsed: the parser accepted the payload. */
FD_TXN_FN int
fd_precompile_core_plan( unsigned char const * payload, unsigned long payload_sz, fd_precompile_core_ent_t * ents,
                         unsigned long cap, fd_precompile_core_sum_t * sum, int * parsed ) {
  fd_ed25519_hip_txn_t tx;
  unsigned tab[ FD_TXN_CORE_INSTR_MAX ];
  sum->ent_cnt = 0U; sum->hdr_instr = 0xFF; sum->hdr_pos = 0;
  *parsed = payload && fd_txn_core_parse( payload, payload_sz, &tx, (unsigned char *)0, 0UL )!=0UL;
  if( !*parsed ) return 0;
  unsigned long mask = fd_precompile_core_table( payload, &tx, tab, 1UL );
  fd_precompile_core_summary( payload, tab, 1UL, tx.instr_cnt, mask, sum );
  unsigned long k = 0UL;
  for( unsigned j=0U; j<(unsigned)tx.instr_cnt && k<cap; j++ ) {
    if( !( ( mask >> j ) & 1UL ) ) continue;
    int h = fd_precompile_core_header( payload + FD_PRECOMPILE_CORE_TAB_OFF( tab[ j ] ), FD_PRECOMPILE_CORE_TAB_SZ( tab[ j ] ) );
    for( int i=0; i<h && k<cap; i++, k++ ) fd_precompile_core_entry( payload, tab, 1UL, tx.instr_cnt, j, (unsigned)i, ents+k );
  }
  return (int)k;
}

#endif
