/* fd_packet_core.h -- what fd_gossip_recv_packet and
   fd_repair_recv_serv_packet decide for a signed control packet of fixed or
   nearly fixed layout before they call fd_ed25519_verify, restated once and
   compiled three ways: into the device stage kernel (fd_ed25519_packet.hip,
   hipcc), into the host library (host/fd_ed25519_hip_fronts.c, gcc:
   fd_ed25519_hip_packet_plan) and into the hostile input test's stand-alone
   program (tests/packet_walk_main.c, gcc with sanitizers).  The includer
   may define FD_PACKET_FN (the function qualifiers) and the readers
   FD_PACKET_U32 / FD_PACKET_U64 (little-endian loads at any byte) and
   FD_PACKET_KEY_T / FD_PACKET_KEY_NE (the own identity and its comparison
   with 32 packet bytes); the defaults read bytes.

   Reference: src/flamenco/gossip/fd_gossip.c:1858-1878 (decode, every byte
   consumed), :646-656 and :940-949 (ping and pong), :1201-1236 (prune),
   src/flamenco/repair/fd_repair.c:1012-1070 (decode, every byte consumed,
   the kinds, the recipient, the verify), src/flamenco/types/fd_types.c:
   fd_gossip_msg_decode_preflight (:22522-22599), fd_gossip_ping (:18769),
   fd_gossip_prune_msg / _prune_data (:22445, :18995),
   fd_gossip_prune_sign_data_encode (:19239), fd_repair_protocol_decode_
   preflight (:23540-23650), fd_repair_request_header (:23133: signature 64,
   sender 32, recipient 32, timestamp 8, nonce 4), fd_repair_window_index
   (:23232: header, slot 8, shred_index 8), _highest_window_index (:23307:
   the same), _orphan (:23382: header, slot 8), _ancestor_hashes (:23447).
   Rules, for a packet p of sz bytes (bincode: fixed-width little-endian):

     both protocols: NULL, sz < 4 (no discriminant: fd_bincode_uint32_decode
       fails) or sz > 1232 (PACKET_DATA_SIZE, fd_gossip.c:17: no larger UDP
       payload reaches the handlers; this library's cap) gives ERR_PARSE;
       disc = u32 at 0

     gossip (fd_gossip_msg, fd_types.c:22522-22556):
       disc 0 pull_req, 1 pull_resp, 2 push_msg: UNSUPPORTED with no further
         look (their CRDS values stay with the caller)
       disc 4 ping, 5 pong: sz != 132 gives ERR_PARSE (from 32, token 32,
         signature 64; fd_gossip.c:1873 wants every byte consumed); key
         [4,36), message [36,68), signature [68,132)   (fd_gossip.c:646-656,
         :940-949; the pong's table lookup and token comparison, :913-938,
         have no side effect and stay with the caller)
       disc 3 prune: pubkey [4,36), data.pubkey [36,68), m = u64 at [68,76),
         m prunes of 32, signature 64, destination 32, wallclock 8:
         sz < 180, m > (sz-180)/32 or sz != 180 + 32 m gives ERR_PARSE (the
         comparison comes before the product, so no m wraps; m <= 32
         follows from sz <= 1232)
         destination [140+32m, 172+32m) != own identity: NOT_FOR_SELF (:1205)
         key data.pubkey [36,68), not the outer pubkey       (:1216-1219)
         signature [76+32m, 140+32m)
         message [36, 76+32m) then [140+32m, 180+32m): pubkey, prunes_len,
           prunes, destination, wallclock as
           fd_gossip_prune_sign_data_encode writes them      (:1209-1233)
       disc >= 6: ERR_PARSE                              (fd_types.c:22555)

     repair serve (fd_repair_protocol, fd_types.c:23540-23590):
       disc 0..6 legacy: sz == 4 decodes and falls to "unknown type"
         (fd_repair.c:1048): UNSUPPORTED; else ERR_PARSE
       disc 7 pong: sz == 132 UNSUPPORTED (its signed message is a hash of
         the caller's own ping token, fd_repair.c:986-1006); else ERR_PARSE
       disc 11 ancestor_hashes: sz == 152 UNSUPPORTED (:1048); else ERR_PARSE
       disc 8 window_index, 9 highest_window_index: sz != 160 ERR_PARSE
       disc 10 orphan: sz != 152 ERR_PARSE
       disc >= 12: ERR_PARSE                             (fd_types.c:23589)
       for 8, 9, 10: recipient [100,132) != own identity: NOT_FOR_SELF
         (fd_repair.c:1053); key the sender [68,100), signature [4,68),
         message [0,4) then [68,sz) (:1060-1067: the reference copies the
         discriminant over the signature's tail and verifies from byte 64;
         the packet is const here and that is not imitated)

   A plan names the key, the signature and the message as two runs of packet
   bytes, the second possibly empty; every run lies inside [0,sz). */
#ifndef FD_PACKET_CORE_H
#define FD_PACKET_CORE_H

#ifndef FD_PACKET_FN
#define FD_PACKET_FN static inline
#endif

#define FD_PACKET_CORE_OK            (  0)
#define FD_PACKET_CORE_ERR_PARSE     (-16)
#define FD_PACKET_CORE_UNSUPPORTED   (-18)
#define FD_PACKET_CORE_ERR_SIGNATURE (-20)
#define FD_PACKET_CORE_NOT_FOR_SELF  (-21)

#define FD_PACKET_CORE_PROTO_GOSSIP      (0)
#define FD_PACKET_CORE_PROTO_REPAIR_SERV (1)

#define FD_PACKET_CORE_MAX       1232UL   /* PACKET_DATA_SIZE */
#define FD_PACKET_CORE_PING_SZ    132UL   /* disc 4, from 32, token 32, signature 64 */
#define FD_PACKET_CORE_PRUNE_SZ   180UL   /* disc 4, pubkey 32, data: pubkey 32, len 8, signature 64, destination 32, wallclock 8 */
#define FD_PACKET_CORE_WINDOW_SZ  160UL   /* disc 4, header 140, slot 8, shred_index 8 */
#define FD_PACKET_CORE_ORPHAN_SZ  152UL   /* disc 4, header 140, slot 8 */
#define FD_PACKET_CORE_ANCESTOR_SZ 152UL  /* the same fields as orphan */

/* the layout of fd_ed25519_hip_packet_plan_t (include/fd_ed25519_hip.h) */
typedef struct {
  unsigned short key_off, sig_off, msg0_off, msg0_sz, msg1_off, msg1_sz;
  unsigned int   disc;
} fd_packet_core_plan_t;

FD_PACKET_FN unsigned
fd_packet_core_u32( unsigned char const * p ) {
  return (unsigned)p[ 0 ] | ( (unsigned)p[ 1 ] << 8 ) | ( (unsigned)p[ 2 ] << 16 ) | ( (unsigned)p[ 3 ] << 24 );
}

FD_PACKET_FN unsigned long long
fd_packet_core_u64( unsigned char const * p ) {
  return (unsigned long long)fd_packet_core_u32( p ) | ( (unsigned long long)fd_packet_core_u32( p + 4 ) << 32 );
}

FD_PACKET_FN int
fd_packet_core_key_ne( unsigned char const * p, unsigned char const * key ) {
  unsigned d = 0U;
  for( int i=0; i<32; i++ ) d |= (unsigned)( p[ i ] ^ key[ i ] );
  return d!=0U;
}

#ifndef FD_PACKET_U32
#define FD_PACKET_U32( p ) fd_packet_core_u32( p )
#endif
#ifndef FD_PACKET_U64
#define FD_PACKET_U64( p ) fd_packet_core_u64( p )
#endif
#ifndef FD_PACKET_KEY_T
#define FD_PACKET_KEY_T unsigned char const *
#define FD_PACKET_KEY_NE( p, key ) fd_packet_core_key_ne( p, key )
#endif

/* The code of one packet before any verify: OK with the plan filled,
   else ERR_PARSE, UNSUPPORTED or NOT_FOR_SELF with every offset and size of
   the plan zero.  plan->disc is the discriminant wherever one was read. */
FD_PACKET_FN int
fd_packet_core_plan( int proto, unsigned char const * p, unsigned long sz, FD_PACKET_KEY_T self,
                     fd_packet_core_plan_t * plan ) {
  plan->key_off = plan->sig_off = plan->msg0_off = plan->msg0_sz = plan->msg1_off = plan->msg1_sz = (unsigned short)0;
  plan->disc = 0U;
  if( !p || sz<4UL || sz>FD_PACKET_CORE_MAX ) return FD_PACKET_CORE_ERR_PARSE;
  unsigned disc = FD_PACKET_U32( p );
  plan->disc = disc;

  if( proto==FD_PACKET_CORE_PROTO_GOSSIP ) {
    if( disc<=2U ) return FD_PACKET_CORE_UNSUPPORTED;                       /* fd_types.c:22525-22539 */
    if( disc>=6U ) return FD_PACKET_CORE_ERR_PARSE;                         /* fd_types.c:22555 */
    if( disc!=3U ) {                                                        /* ping, pong */
      if( sz!=FD_PACKET_CORE_PING_SZ ) return FD_PACKET_CORE_ERR_PARSE;     /* fd_types.c:18769, fd_gossip.c:1873 */
      plan->key_off  = (unsigned short) 4;                                  /* fd_gossip.c:653, :946 */
      plan->msg0_off = (unsigned short)36; plan->msg0_sz = (unsigned short)32;   /* :650, :943 */
      plan->sig_off  = (unsigned short)68;                                  /* :652, :945 */
      return FD_PACKET_CORE_OK;
    }
    if( sz<FD_PACKET_CORE_PRUNE_SZ ) return FD_PACKET_CORE_ERR_PARSE;       /* fd_types.c:22445, :18995 */
    unsigned long long m = FD_PACKET_U64( p + 68 );
    if( m>( sz-FD_PACKET_CORE_PRUNE_SZ )/32UL ) return FD_PACKET_CORE_ERR_PARSE;        /* :19003-19006 runs out of bytes */
    if( sz!=FD_PACKET_CORE_PRUNE_SZ+32UL*(unsigned long)m ) return FD_PACKET_CORE_ERR_PARSE;   /* fd_gossip.c:1873 */
    unsigned run = 32U*(unsigned)m;
    if( FD_PACKET_KEY_NE( p + 140U + run, self ) ) return FD_PACKET_CORE_NOT_FOR_SELF;   /* fd_gossip.c:1205 */
    plan->key_off  = (unsigned short)36;                                    /* :1232 */
    plan->sig_off  = (unsigned short)( 76U + run );                         /* :1231 */
    plan->msg0_off = (unsigned short)36;           plan->msg0_sz = (unsigned short)( 40U + run );   /* :1210-1212 */
    plan->msg1_off = (unsigned short)( 140U+run ); plan->msg1_sz = (unsigned short)40;              /* :1213-1214 */
    return FD_PACKET_CORE_OK;
  }

  if( proto==FD_PACKET_CORE_PROTO_REPAIR_SERV ) {
    if( disc>=12U ) return FD_PACKET_CORE_ERR_PARSE;                        /* fd_types.c:23589 */
    if( disc<=6U )                                                          /* fd_types.c:23543-23563, fd_repair.c:1048 */
      return sz==4UL ? FD_PACKET_CORE_UNSUPPORTED : FD_PACKET_CORE_ERR_PARSE;
    if( disc==7U )                                                          /* fd_repair.c:1027, :986-1006 */
      return sz==FD_PACKET_CORE_PING_SZ ? FD_PACKET_CORE_UNSUPPORTED : FD_PACKET_CORE_ERR_PARSE;
    if( disc==11U )                                                         /* fd_types.c:23447, fd_repair.c:1048 */
      return sz==FD_PACKET_CORE_ANCESTOR_SZ ? FD_PACKET_CORE_UNSUPPORTED : FD_PACKET_CORE_ERR_PARSE;
    if( sz!=( disc==10U ? FD_PACKET_CORE_ORPHAN_SZ : FD_PACKET_CORE_WINDOW_SZ ) )       /* fd_types.c:23232, :23307, :23382 */
      return FD_PACKET_CORE_ERR_PARSE;
    if( FD_PACKET_KEY_NE( p + 100, self ) ) return FD_PACKET_CORE_NOT_FOR_SELF;          /* fd_repair.c:1053 */
    plan->key_off  = (unsigned short)68;                                    /* :1066 */
    plan->sig_off  = (unsigned short) 4;                                    /* :1061 */
    plan->msg0_off = (unsigned short) 0; plan->msg0_sz = (unsigned short)4;                /* :1062 */
    plan->msg1_off = (unsigned short)68; plan->msg1_sz = (unsigned short)( sz-68UL );      /* :1063-1064 */
    return FD_PACKET_CORE_OK;
  }

  return FD_PACKET_CORE_ERR_PARSE;   /* an unknown protocol: the entry points reject it before any packet */
}

#endif /* FD_PACKET_CORE_H */
