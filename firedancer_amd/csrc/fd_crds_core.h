/* fd_crds_core.h -- what fd_gossip_recv_packet and fd_gossip_recv_crds_value
   decide for the CRDS values of a gossip pull response or push message
   before they call fd_ed25519_verify, restated once and compiled three ways:
   into the device stage kernel (fd_ed25519_crds.hip, hipcc), into the host
   library (host/fd_ed25519_hip_fronts.c, gcc: fd_ed25519_hip_crds_count,
   _crds_plan) and into the hostile input test's stand-alone program
   (tests/crds_walk_main.c, gcc with sanitizers).  Include after
   fd_txn_parse_core.h (fd_txn_core_cu16, fd_txn_core_parse_prefix).  The
   includer may define FD_CRDS_FN (the function qualifiers), the readers
   FD_CRDS_U32 / FD_CRDS_U64 (little-endian loads at any byte) and
   FD_CRDS_KEY_T / FD_CRDS_KEY_NE (the own identity and its comparison with
   32 packet bytes); the defaults read bytes.

   Reference: src/flamenco/gossip/fd_gossip.c:1858-1878 (decode, every byte
   consumed), :1420-1430 (every value of a pull response and of a push
   message goes to fd_gossip_recv_crds_value, with the message's pubkey),
   :1020-1091 (the key, the own-identity drop, the re-encode, the verify),
   :1093-1105 (the value hash); src/flamenco/types/fd_types.c,
   fd_bincode.h, fd_types_custom.c as cited at each rule.

   The walk is a cursor over the packet's sz bytes.  It never computes a
   size from a length field: a length either counts loop iterations, each of
   which consumes at least one byte or fails, or is compared with the bytes
   that remain (fd_bincode_bytes_decode_preflight, fd_bincode.h:168-177), so
   a length of 2^64-1 ends within the packet.

   Packet (bincode: fixed-width little-endian):
     NULL, sz < 4 or sz > 1232 (PACKET_DATA_SIZE, fd_gossip.c:17): ERR_PARSE
     disc = u32 at 0                                   (fd_types.c:22522-22556)
       0 pull_req, 3 prune, 4 ping, 5 pong: UNSUPPORTED with no further look
         (the packet front's, or the caller's)
       >= 6: ERR_PARSE                                            (:22555)
       1 pull_resp (:22229), 2 push_msg (:22337): pubkey [4,36), crds_len u64
         [36,44), crds_len values; the packet is judged as a whole
         (fd_gossip.c:1868-1877): a value that fails its decode, or a byte
         behind the last value, gives ERR_PARSE and no value a verdict
   Value (:22095): signature 64, then fd_crds_data (:21585): u32 data
     discriminant (>= 12: fails, :21521) and the variant's fields:
      0 contact_info_v1 (:19332) id 32, ten socket_addr (:19267: ip_addr
          :18883 = u32 0 with 4 bytes or 1 with 16, else fails; port u16),
          wallclock u64, shred_version u16
      1 vote (:19527) index u8, from 32, txn, wallclock u64; the txn is
          fd_flamenco_txn_decode_preflight (fd_types_custom.c:28-38):
          fd_txn_core_parse_prefix over all the bytes that remain
      2 lowest_slot (:19614) u8, from 32, root u64, lowest u64, slots_len u64
          with as many u64, u64, wallclock u64
      3, 4 slot_hashes (:19767) from 32, hashes_len u64 with as many
          slot_hash (:9255: u64, hash 32), wallclock u64
      5 epoch_slots (:20206) u8, from 32, slots_len u64 with as many
          slots_enum (:20094: u32 0 flate2 :19960 = first_slot u64, num u64,
          compressed_len u64 and as many bytes; 1 uncompressed :19885 =
          first_slot u64, num u64, bitvec_u8 :18478 = option tag, if 1
          vec_len u64 and as many bytes (:18399), then len u64; else
          fails), wallclock u64
      6 version_v1 (:20334) from 32, wallclock u64, three u16, option tag,
          if 1 commit u32
      7 version_v2 (:20474) the same, then feature_set u32
      8 node_instance (:20727) from 32, three u64
      9 duplicate_shred (:20812) version u16, from 32, wallclock u64, slot
          u64, u32, three u8, chunk_len u64 and as many bytes
     10 incremental_snapshot_hashes (:20973) from 32, slot_hash, hashes_len
          u64 with as many slot_hash, wallclock u64
     11 contact_info_v2 (:21176) from 32, wallclock varint, outset u64,
          shred_version u16, version_v3 (:20624: three compact-u16, two u32,
          compact-u16), compact-u16 addrs_len with as many ip_addr,
          compact-u16 sockets_len with as many socket_entry (:21103: u8, u8,
          compact-u16), compact-u16 extensions_len with as many u32
     An option tag is a bool: anything but 0 or 1 fails (fd_bincode.h:
     102-116).  compact-u16 (:204-232) and varint (:311-340) reject
     non-minimal and over-long forms.
   Key (fd_gossip.c:1023-1071): for data discriminants 0..10 the variant's
     own id / from, which lies 0 (0, 3, 4, 6, 7, 8, 10), 1 (1, 2, 5: a u8 in
     front) or 2 (9: a u16 in front) bytes into the fields; for 11 the
     switch falls to default and the key stays the message's pubkey [4,36).
     A value whose key is the own identity is dropped unverified (:1072):
     OWN.
   Message (:1075-1088): fd_crds_data_encode of the decoded value, not the
     received bytes.  For data discriminants 0..10 every encoding the
     decoders above accept is the one the encoders write -- the widths are
     fixed, bool / option tags are 0 or 1 and written as such
     (fd_bincode.h:140-151), a vector's bytes follow its own length, the
     transaction is written from the raw bytes the parser took
     (fd_types_custom.c:21-22) -- so the re-encode equals the received run
     [data discriminant, end of value), which is read in place.
     contact_info_v2 is the exception: the decoders read version_v3's major,
     minor, patch and client and every socket_entry's offset as compact-u16
     (:20626-20636, :21109), the encoders write them as plain u16
     (:20703-20713, :21162).  No compact-u16 is its value's u16 (one byte
     against two; three against two; of two bytes the first has bit 7 set
     where the u16's low byte has it only for an odd second byte, which
     would then have to equal its own half), and version_v3 is in every
     contact_info_v2, so the re-encode of a contact_info_v2 never equals the
     received run.  The rules here never give a verdict over bytes the
     reference would not have hashed: such a value is UNSUPPORTED (unless it
     is OWN, which the reference decides first) and stays with the caller.
     tests/golden/crds.npz records the reference's re-encoded bytes for every
     decoded value and tests/test_crds_core.py compares them with the
     planned run.
   Hash (:1093-1105): SHA-256 of fd_crds_value_encode's output, by the same
     argument the received run [signature, end of value) for data
     discriminants 0..10, and not taken for contact_info_v2.

   The smallest value is a version_v1 without commit: 64 + 4 + 32 + 8 + 6 + 1
   = 115 bytes, so a packet holds at most (1232 - 44) / 115 = 10 values
   (FD_CRDS_CORE_VAL_MAX).  The walk keeps the start of each as 12 bits of
   two 64-bit words, five each (every start is below 1232 < 4096), so a lane
   needs no array. */
#ifndef FD_CRDS_CORE_H
#define FD_CRDS_CORE_H

#ifndef FD_CRDS_FN
#define FD_CRDS_FN static inline
#endif

#define FD_CRDS_CORE_OK            (  0)
#define FD_CRDS_CORE_ERR_PARSE     (-16)
#define FD_CRDS_CORE_UNSUPPORTED   (-18)
#define FD_CRDS_CORE_ERR_SIGNATURE (-20)
#define FD_CRDS_CORE_OWN           (-21)

#define FD_CRDS_CORE_MAX      1232UL   /* PACKET_DATA_SIZE */
#define FD_CRDS_CORE_HDR_SZ     44UL   /* disc 4, pubkey 32, crds_len 8 */
#define FD_CRDS_CORE_VAL_MIN   115UL   /* signature 64, disc 4, version_v1: from 32, wallclock 8, three u16, tag 1 */
#define FD_CRDS_CORE_VAL_MAX    10UL   /* (1232 - 44) / 115 */
#define FD_CRDS_CORE_DISC_CNT   12U    /* fd_types.c:21521 */

/* the layout of fd_ed25519_hip_crds_val_t (include/fd_ed25519_hip.h);
   offsets are relative to the packet */
typedef struct {
  unsigned int   disc;      /* the data discriminant, 0..11 */
  unsigned short sig_off;
  unsigned short key_off;
  unsigned short msg_off;
  unsigned short msg_sz;
  signed char    pre;       /* 0, FD_CRDS_CORE_OWN or FD_CRDS_CORE_UNSUPPORTED */
} fd_crds_core_val_t;

/* what the walk of a decoded packet leaves: crds_len and the values' starts */
typedef struct {
  unsigned           cnt;
  unsigned long long starts[ 2 ];
} fd_crds_core_idx_t;

FD_CRDS_FN unsigned
fd_crds_core_u32( unsigned char const * p ) {
  return (unsigned)p[ 0 ] | ( (unsigned)p[ 1 ] << 8 ) | ( (unsigned)p[ 2 ] << 16 ) | ( (unsigned)p[ 3 ] << 24 );
}

FD_CRDS_FN unsigned long long
fd_crds_core_u64( unsigned char const * p ) {
  return (unsigned long long)fd_crds_core_u32( p ) | ( (unsigned long long)fd_crds_core_u32( p + 4 ) << 32 );
}

FD_CRDS_FN int
fd_crds_core_key_ne( unsigned char const * p, unsigned char const * key ) {
  unsigned d = 0U;
  for( int i=0; i<32; i++ ) d |= (unsigned)( p[ i ] ^ key[ i ] );
  return d!=0U;
}

#ifndef FD_CRDS_U32
#define FD_CRDS_U32( p ) fd_crds_core_u32( p )
#endif
#ifndef FD_CRDS_U64
#define FD_CRDS_U64( p ) fd_crds_core_u64( p )
#endif
#ifndef FD_CRDS_KEY_T
#define FD_CRDS_KEY_T unsigned char const *
#define FD_CRDS_KEY_NE( p, key ) fd_crds_core_key_ne( p, key )
#endif

/* The decoders: each takes the packet, its size and the cursor, and returns
   the cursor behind what it decoded, or 0 when the decode fails (no decoder
   is called at cursor 0, and every one consumes a byte at least). */
#define FD_CRDS_SKIP( k )      do { if( (unsigned long)(k) > sz - i ) return 0UL; i += (unsigned long)(k); } while(0)
#define FD_CRDS_GET_U32( dst ) do { if( 4UL > sz - i ) return 0UL; (dst) = FD_CRDS_U32( p + i ); i += 4UL; } while(0)
#define FD_CRDS_GET_U64( dst ) do { if( 8UL > sz - i ) return 0UL; (dst) = FD_CRDS_U64( p + i ); i += 8UL; } while(0)
#define FD_CRDS_GET_TAG( dst ) do { if( 1UL > sz - i ) return 0UL; (dst) = p[ i ]; if( (dst) & ~1U ) return 0UL; i += 1UL; } while(0)
#define FD_CRDS_GET_CU16( dst ) do { unsigned long n_ = fd_txn_core_cu16( p + i, sz - i, &(dst) ); if( !n_ ) return 0UL; i += n_; } while(0)
#define FD_CRDS_SUB( call )    do { i = (call); if( !i ) return 0UL; } while(0)

/* len bytes behind a u64 length: fd_bincode_bytes_decode_preflight compares, it does not add (fd_bincode.h:171) */
FD_CRDS_FN unsigned long
fd_crds_core_bytes( unsigned char const * p, unsigned long sz, unsigned long i ) {
  unsigned long long len;
  FD_CRDS_GET_U64( len );
  if( len > (unsigned long long)( sz - i ) ) return 0UL;
  return i + (unsigned long)len;
}

/* fd_bincode_varint_decode (fd_bincode.h:311-340): at most ten bytes, the
   last one at most 1 and the value's top bits not shifted out, no zero byte
   at the end of more than one */
FD_CRDS_FN unsigned long
fd_crds_core_varint( unsigned char const * p, unsigned long sz, unsigned long i ) {
  unsigned long long out = 0ULL;
  for( unsigned shift=0U; shift<64U; shift+=7U ) {
    if( 1UL > sz - i ) return 0UL;
    unsigned byte = p[ i++ ];
    out |= (unsigned long long)( byte & 0x7FU ) << shift;
    if( !( byte & 0x80U ) ) {
      if( ( out >> shift )!=(unsigned long long)byte ) return 0UL;                         /* :327 */
      if( byte==0U && ( shift!=0U || out!=0ULL ) ) return 0UL;                             /* :329 */
      return i;
    }
  }
  return 0UL;                                                                              /* :339 */
}

FD_CRDS_FN unsigned long
fd_crds_core_ip_addr( unsigned char const * p, unsigned long sz, unsigned long i ) {      /* fd_types.c:18846-18888 */
  unsigned d;
  FD_CRDS_GET_U32( d );
  if( d>1U ) return 0UL;
  FD_CRDS_SKIP( d ? 16UL : 4UL );
  return i;
}

FD_CRDS_FN unsigned long
fd_crds_core_slot_hashes( unsigned char const * p, unsigned long sz, unsigned long i ) {   /* hashes_len and its slot_hash */
  unsigned long long len;
  FD_CRDS_GET_U64( len );
  for( unsigned long long k=0ULL; k<len; k++ ) FD_CRDS_SKIP( 40UL );
  return i;
}

FD_CRDS_FN unsigned long
fd_crds_core_slots_enum( unsigned char const * p, unsigned long sz, unsigned long i ) {   /* fd_types.c:20057-20098 */
  unsigned d, tag;
  FD_CRDS_GET_U32( d );
  if( d>1U ) return 0UL;
  FD_CRDS_SKIP( 16UL );                                             /* first_slot, num */
  if( d==0U ) {                                                     /* flate2, :19960 */
    FD_CRDS_SUB( fd_crds_core_bytes( p, sz, i ) );
    return i;
  }
  FD_CRDS_GET_TAG( tag );                                           /* bitvec_u8, :18478 */
  if( tag ) FD_CRDS_SUB( fd_crds_core_bytes( p, sz, i ) );
  FD_CRDS_SKIP( 8UL );
  return i;
}

/* the fields of variant disc from cursor i (behind the data discriminant) */
FD_CRDS_FN unsigned long
fd_crds_core_fields( unsigned disc, unsigned char const * p, unsigned long sz, unsigned long i ) {
  unsigned long long len;
  unsigned tag, cnt;
  switch( disc ) {
  case 0U:                                                          /* contact_info_v1 */
    FD_CRDS_SKIP( 32UL );
    for( int k=0; k<10; k++ ) { FD_CRDS_SUB( fd_crds_core_ip_addr( p, sz, i ) ); FD_CRDS_SKIP( 2UL ); }
    FD_CRDS_SKIP( 10UL );
    return i;
  case 1U: {                                                        /* vote */
    FD_CRDS_SKIP( 33UL );
    unsigned long t = fd_txn_core_parse_prefix( p + i, sz - i );
    if( !t ) return 0UL;
    i += t;
    FD_CRDS_SKIP( 8UL );
    return i;
  }
  case 2U:                                                          /* lowest_slot */
    FD_CRDS_SKIP( 49UL );
    FD_CRDS_GET_U64( len );
    for( unsigned long long k=0ULL; k<len; k++ ) FD_CRDS_SKIP( 8UL );
    FD_CRDS_SKIP( 16UL );
    return i;
  case 3U: case 4U:                                                 /* snapshot_hashes, accounts_hashes */
    FD_CRDS_SKIP( 32UL );
    FD_CRDS_SUB( fd_crds_core_slot_hashes( p, sz, i ) );
    FD_CRDS_SKIP( 8UL );
    return i;
  case 5U:                                                          /* epoch_slots */
    FD_CRDS_SKIP( 33UL );
    FD_CRDS_GET_U64( len );
    for( unsigned long long k=0ULL; k<len; k++ ) FD_CRDS_SUB( fd_crds_core_slots_enum( p, sz, i ) );
    FD_CRDS_SKIP( 8UL );
    return i;
  case 6U: case 7U:                                                 /* version_v1, version_v2 */
    FD_CRDS_SKIP( 46UL );
    FD_CRDS_GET_TAG( tag );
    if( tag ) FD_CRDS_SKIP( 4UL );
    if( disc==7U ) FD_CRDS_SKIP( 4UL );
    return i;
  case 8U:                                                          /* node_instance */
    FD_CRDS_SKIP( 56UL );
    return i;
  case 9U:                                                          /* duplicate_shred */
    FD_CRDS_SKIP( 57UL );
    FD_CRDS_SUB( fd_crds_core_bytes( p, sz, i ) );
    return i;
  case 10U:                                                         /* incremental_snapshot_hashes */
    FD_CRDS_SKIP( 72UL );
    FD_CRDS_SUB( fd_crds_core_slot_hashes( p, sz, i ) );
    FD_CRDS_SKIP( 8UL );
    return i;
  case 11U:                                                         /* contact_info_v2 */
    FD_CRDS_SKIP( 32UL );
    FD_CRDS_SUB( fd_crds_core_varint( p, sz, i ) );
    FD_CRDS_SKIP( 10UL );
    FD_CRDS_GET_CU16( cnt ); FD_CRDS_GET_CU16( cnt ); FD_CRDS_GET_CU16( cnt );           /* version_v3 */
    FD_CRDS_SKIP( 8UL );
    FD_CRDS_GET_CU16( cnt );
    FD_CRDS_GET_CU16( cnt );
    for( unsigned k=0U; k<cnt; k++ ) FD_CRDS_SUB( fd_crds_core_ip_addr( p, sz, i ) );
    FD_CRDS_GET_CU16( cnt );
    for( unsigned k=0U; k<cnt; k++ ) { unsigned off; FD_CRDS_SKIP( 2UL ); FD_CRDS_GET_CU16( off ); (void)off; }
    FD_CRDS_GET_CU16( cnt );
    for( unsigned k=0U; k<cnt; k++ ) FD_CRDS_SKIP( 4UL );
    return i;
  default:
    return 0UL;                                                     /* fd_types.c:21521 */
  }
}

/* one value from cursor i: signature, data discriminant, fields */
FD_CRDS_FN unsigned long
fd_crds_core_value_end( unsigned char const * p, unsigned long sz, unsigned long i ) {
  unsigned disc;
  FD_CRDS_SKIP( 64UL );
  FD_CRDS_GET_U32( disc );
  return fd_crds_core_fields( disc, p, sz, i );
}

#undef FD_CRDS_SKIP
#undef FD_CRDS_GET_U32
#undef FD_CRDS_GET_U64
#undef FD_CRDS_GET_TAG
#undef FD_CRDS_GET_CU16
#undef FD_CRDS_SUB

/* where the key of a value of this data discriminant lies behind it; -1:
   the message's pubkey */
FD_CRDS_FN int
fd_crds_core_key_delta( unsigned disc ) {
  /* 2 bits per discriminant 0..10: 0 1 1 0 0 1 0 0 0 2 0 */
  return disc>=11U ? -1 : (int)( ( 0x80414U >> ( 2U*disc ) ) & 3U );
}

FD_CRDS_FN unsigned
fd_crds_core_start( fd_crds_core_idx_t const * idx, unsigned k ) {
  return (unsigned)( ( k<5U ? idx->starts[ 0 ] >> ( 12U*k ) : idx->starts[ 1 ] >> ( 12U*( k-5U ) ) ) & 0xFFFULL );
}

/* The code of one packet before any verify: OK with idx filled (crds_len
   values, 0..VAL_MAX), else ERR_PARSE or UNSUPPORTED with idx->cnt 0. */
FD_CRDS_FN int
fd_crds_core_walk( unsigned char const * p, unsigned long sz, fd_crds_core_idx_t * idx ) {
  idx->cnt = 0U; idx->starts[ 0 ] = idx->starts[ 1 ] = 0ULL;
  if( !p || sz<4UL || sz>FD_CRDS_CORE_MAX ) return FD_CRDS_CORE_ERR_PARSE;
  unsigned disc = FD_CRDS_U32( p );
  if( disc>=6U ) return FD_CRDS_CORE_ERR_PARSE;                                           /* fd_types.c:22555 */
  if( disc!=1U && disc!=2U ) return FD_CRDS_CORE_UNSUPPORTED;
  if( sz<FD_CRDS_CORE_HDR_SZ ) return FD_CRDS_CORE_ERR_PARSE;                             /* :22231-22235 */
  unsigned long long crds_len = FD_CRDS_U64( p + 36 );
  unsigned long i = FD_CRDS_CORE_HDR_SZ;
  unsigned long long s0 = 0ULL, s1 = 0ULL;
  for( unsigned long long k=0ULL; k<crds_len; k++ ) {                                     /* :22236-22241 */
    /* a value takes VAL_MIN bytes at least, so the eleventh does not fit; the bound keeps the starts inside their words */
    if( k>=FD_CRDS_CORE_VAL_MAX ) return FD_CRDS_CORE_ERR_PARSE;
    if( k<5ULL ) s0 |= (unsigned long long)i << ( 12U*(unsigned)k );
    else         s1 |= (unsigned long long)i << ( 12U*( (unsigned)k-5U ) );
    i = fd_crds_core_value_end( p, sz, i );
    if( !i ) return FD_CRDS_CORE_ERR_PARSE;
  }
  if( i!=sz ) return FD_CRDS_CORE_ERR_PARSE;                                              /* fd_gossip.c:1873 */
  idx->cnt = (unsigned)crds_len; idx->starts[ 0 ] = s0; idx->starts[ 1 ] = s1;
  return FD_CRDS_CORE_OK;
}

/* whether fd_crds_data_encode of a decoded value of this data discriminant
   writes the received run (above, "Message") */
FD_CRDS_FN int
fd_crds_core_reencodes( unsigned disc ) {
  return disc<11U;
}

/* Value k < idx->cnt of a packet fd_crds_core_walk gave OK: where its
   signature, key and received run lie, and pre: OWN for a value under the
   own identity, else UNSUPPORTED for one whose re-encode is not the
   received run, else 0 (the offsets are filled all the same).  A value
   ends where the next one starts, the last one with the packet. */
FD_CRDS_FN void
fd_crds_core_value( unsigned char const * p, unsigned long sz, fd_crds_core_idx_t const * idx, unsigned k, FD_CRDS_KEY_T self,
                    fd_crds_core_val_t * v ) {
  unsigned start = fd_crds_core_start( idx, k );
  unsigned end   = k+1U<idx->cnt ? fd_crds_core_start( idx, k+1U ) : (unsigned)sz;
  unsigned disc  = FD_CRDS_U32( p + start + 64U );
  int delta      = fd_crds_core_key_delta( disc );
  v->disc    = disc;
  v->sig_off = (unsigned short)start;
  v->msg_off = (unsigned short)( start + 64U );
  v->msg_sz  = (unsigned short)( end - start - 64U );
  v->key_off = (unsigned short)( delta<0 ? 4U : start + 68U + (unsigned)delta );         /* fd_gossip.c:1023-1071 */
  v->pre     = (signed char)( !FD_CRDS_KEY_NE( p + v->key_off, self ) ? FD_CRDS_CORE_OWN                 /* :1072 */
                            : !fd_crds_core_reencodes( disc )         ? FD_CRDS_CORE_UNSUPPORTED : 0 );  /* :1075-1082 */
}

#endif /* FD_CRDS_CORE_H */
