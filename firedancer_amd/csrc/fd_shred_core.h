/* fd_shred_core.h -- what fd_fec_resolver_add_shred decides for a Merkle
   shred that opens a FEC set, up to the root its leader signed, restated
   once and compiled three ways: into the device stage kernel
   (fd_ed25519_shred.hip, hipcc: the rules; the kernel hashes with its own
   SHA-256), into the host library (host/fd_ed25519_hip_fronts.c, gcc:
   fd_ed25519_hip_shred_root) and into the hostile input test's stand-alone
   program (tests/shred_walk_main.c, gcc with sanitizers).  The includer may
   define FD_SHRED_FN (the function qualifiers).

   Reference: src/ballet/shred/fd_shred.c:3-72 (fd_shred_parse),
   src/ballet/shred/fd_shred.h:83-91, 97-112, 155-227, 269-299 (sizes, types,
   the packed header, header and proof sizes),
   src/disco/shred/fd_fec_resolver.c:311-359 (the resolver's header checks),
   :339-342 with src/ballet/bmtree/fd_bmtree.c:51-68 (the leaf),
   fd_bmtree.c:78-130 and :384-459 (the node hash and the walk of an
   inclusion proof on a fresh tree), fd_bmtree.c:147-153 (fd_bmtree_depth).
   Rules, for a shred s of sz bytes (all fields little-endian, unaligned):

     parse (fd_shred.c:3-72): NULL gives ERR_PARSE
       sz < 0x58                                                        (:8)
       variant = s[0x40], type = variant & 0xf0; accepted: types 0x80 0x40
         0x90 0x60 0xb0 0x70 and the legacy variants 0xa5 0x5a          (:14-24)
       header 0x58 (type & 0x80: data) or 0x59 (type & 0x40: code); proof
         20 (variant & 0xf) bytes, none for types 0xa0 0x50; chained root 32
         bytes for types 0x90 0x60 0xb0 0x70                            (:30-39)
       data: size = u16 at 0x56; size < 0x58; type != 0xa0 and sz < 1203;
         eff = (type & 0x20) ? sz : 1203 (0xb0 has that bit too);
         eff < 0x58 + proof + (size - 0x58) + chained; sz < eff         (:41-59,69)
       code: sz < 1228                                                  (:60-66,69)
     supported: types 0x80 and 0x40; every other parsed variant gives
       UNSUPPORTED (the resolver tests type==0x80 and reads everything else
       as a code shred, fd_fec_resolver.c:327; that misreading of chained and
       legacy shreds is not imitated)
     header (fd_fec_resolver.c, in this order), each ERR_HEADER:
       the 64-byte signature all zero                                   (:314)
       code: data_cnt (u16 at 0x53) or code_cnt (u16 at 0x55) 0 or > 67 (:330-332)
       in_type_idx >= 67: data idx (u32 at 0x49) - fec_set_idx (u32 at
         0x4f) mod 2^32, code code.idx (u16 at 0x57)                    (:351-355)
       fd_bmtree_depth( shred_idx+1 ) > tree_depth+1, shred_idx =
         in_type_idx (+ data_cnt for code), tree_depth = variant & 0xf:
         depth(1) = 1 always fits, depth(n) = msb(n-1)+2 for n >= 2, so the
         test is shred_idx >> tree_depth != 0                           (:359)
     leaf (:339-342): SHA-256( "\0SOLANA_MERKLE_SHREDS_LEAF" (26 bytes) ||
       s[64 .. 64+P) ), P = 1115 - 20 tree_depth + 0x18 (+ 0x19 for code)
     walk: proof node l at 1203 (data) or 1228 (code) - 20 tree_depth + 20 l;
       layer l = 0 .. tree_depth-1: SHA-256( "\1SOLANA_MERKLE_SHREDS_NODE"
       (26 bytes) || left[0..20) || right[0..20) ), the running node right
       when bit l of shred_idx is set, the sibling proof node l; the root is
       the last hash's 32 bytes (the leaf hash itself at tree_depth 0)

   The leaf and the proof lie inside what the parser proved present: a data
   shred ends them at 1203 <= sz, a code shred at 1228 <= sz. */
#ifndef FD_SHRED_CORE_H
#define FD_SHRED_CORE_H

#ifndef FD_SHRED_FN
#define FD_SHRED_FN static inline
#endif

#define FD_SHRED_CORE_OK            (  0)
#define FD_SHRED_CORE_ERR_PARSE     (-16)
#define FD_SHRED_CORE_UNSUPPORTED   (-18)
#define FD_SHRED_CORE_ERR_HEADER    (-19)
#define FD_SHRED_CORE_ERR_SIGNATURE (-20)

#define FD_SHRED_CORE_MIN_SZ      1203U   /* FD_SHRED_MIN_SZ */
#define FD_SHRED_CORE_MAX_SZ      1228U   /* FD_SHRED_MAX_SZ */
#define FD_SHRED_CORE_DATA_HDR_SZ 0x58U
#define FD_SHRED_CORE_CODE_HDR_SZ 0x59U
#define FD_SHRED_CORE_NODE_SZ     20U     /* FD_SHRED_MERKLE_NODE_SZ */
#define FD_SHRED_CORE_PREFIX_SZ   26U     /* FD_BMTREE_LONG_PREFIX_SZ */
#define FD_SHRED_CORE_IDX_MAX     67U     /* FD_REEDSOL_DATA_SHREDS_MAX == FD_REEDSOL_PARITY_SHREDS_MAX */

/* what the hashing needs of a judged shred */
typedef struct {
  unsigned tree_depth;   /* 0..15 */
  unsigned shred_idx;    /* < 2^tree_depth */
  unsigned leaf_sz;      /* P: bytes hashed from s + 64 */
  unsigned proof_off;    /* of proof node 0 */
} fd_shred_core_t;

FD_SHRED_FN unsigned
fd_shred_core_u16( unsigned char const * p ) { return (unsigned)p[ 0 ] | ( (unsigned)p[ 1 ] << 8 ); }

FD_SHRED_FN unsigned
fd_shred_core_u32( unsigned char const * p ) {
  return (unsigned)p[ 0 ] | ( (unsigned)p[ 1 ] << 8 ) | ( (unsigned)p[ 2 ] << 16 ) | ( (unsigned)p[ 3 ] << 24 );
}

/* fd_shred_parse: nonzero when it returns the shred */
FD_SHRED_FN int
fd_shred_core_parse( unsigned char const * s, unsigned long sz ) {
  if( sz<FD_SHRED_CORE_DATA_HDR_SZ ) return 0;                                          /* :8 */
  unsigned variant = s[ 0x40 ], type = variant & 0xf0U;
  if( ( type!=0x80U ) & ( type!=0x40U ) & ( type!=0x90U ) & ( type!=0x60U ) & ( type!=0xb0U ) & ( type!=0x70U ) &
      ( variant!=0xa5U ) & ( variant!=0x5aU ) ) return 0;                               /* :16-24 */
  unsigned long proof   = ( ( type==0xa0U ) | ( type==0x50U ) ) ? 0UL : 20UL*( variant & 0xfU );
  unsigned long chained = ( ( type==0x90U ) | ( type==0x60U ) | ( type==0xb0U ) | ( type==0x70U ) ) ? 32UL : 0UL;
  if( type & 0x80U ) {
    unsigned long size = fd_shred_core_u16( s + 0x56 );
    if( size<FD_SHRED_CORE_DATA_HDR_SZ ) return 0;                                      /* :42 */
    if( ( type!=0xa0U ) & ( sz<FD_SHRED_CORE_MIN_SZ ) ) return 0;                       /* :44 */
    unsigned long eff = ( type & 0x20U ) ? sz : (unsigned long)FD_SHRED_CORE_MIN_SZ;    /* :55-56 */
    if( eff < proof + size + chained ) return 0;                                        /* :57 */
    return sz>=eff;                                                                     /* :69 */
  }
  /* type & 0x40: the payload fills the shred to 1228 bytes (:60-66) */
  return sz>=FD_SHRED_CORE_MAX_SZ;                                                      /* :69 */
}

/* Rules 1-3: 0 with *o filled for a shred to hash, else its code.  Reads
   bytes below 0x59 only, each once the parser has proved it present. */
FD_SHRED_FN int
fd_shred_core_judge( unsigned char const * s, unsigned long sz, fd_shred_core_t * o ) {
  o->tree_depth = 0U; o->shred_idx = 0U; o->leaf_sz = 0U; o->proof_off = 0U;
  if( !s || !fd_shred_core_parse( s, sz ) ) return FD_SHRED_CORE_ERR_PARSE;
  unsigned variant = s[ 0x40 ], type = variant & 0xf0U;
  if( ( type!=0x80U ) & ( type!=0x40U ) ) return FD_SHRED_CORE_UNSUPPORTED;
  int is_data = type==0x80U;
  unsigned nz = 0U;
  for( int i=0; i<64; i++ ) nz |= s[ i ];
  if( !nz ) return FD_SHRED_CORE_ERR_HEADER;                                            /* :314 */
  unsigned data_cnt = 0U;
  if( !is_data ) {                                   /* sz >= 1228: the code header is there */
    data_cnt = fd_shred_core_u16( s + 0x53 );
    unsigned code_cnt = fd_shred_core_u16( s + 0x55 );
    if( ( data_cnt>FD_SHRED_CORE_IDX_MAX ) | ( code_cnt>FD_SHRED_CORE_IDX_MAX ) ) return FD_SHRED_CORE_ERR_HEADER;   /* :330 */
    if( ( data_cnt==0U ) | ( code_cnt==0U ) ) return FD_SHRED_CORE_ERR_HEADER;          /* :332 */
  }
  unsigned depth = variant & 0xfU;
  unsigned in_type_idx = is_data ? fd_shred_core_u32( s + 0x49 ) - fd_shred_core_u32( s + 0x4f )
                                 : fd_shred_core_u16( s + 0x57 );                       /* :351 */
  if( in_type_idx>=FD_SHRED_CORE_IDX_MAX ) return FD_SHRED_CORE_ERR_HEADER;             /* :354 */
  unsigned shred_idx = in_type_idx + data_cnt;                                          /* :352; below 134 */
  if( shred_idx >> depth ) return FD_SHRED_CORE_ERR_HEADER;                             /* :359 */
  o->tree_depth = depth;
  o->shred_idx  = shred_idx;
  o->leaf_sz    = 1115U - 20U*depth + 0x18U + ( is_data ? 0U : 0x19U );                 /* :339-340 */
  o->proof_off  = ( is_data ? FD_SHRED_CORE_MIN_SZ : FD_SHRED_CORE_MAX_SZ ) - 20U*depth;
  return FD_SHRED_CORE_OK;
}

/* ---- SHA-256 (FIPS 180-4), written from the standard: portable C, one
   64-byte block at a time, of prefix || data for the two prefixed hashes
   above.  The device kernel has its own form of the same function. ---- */

FD_SHRED_FN unsigned
fd_shred_core_ror( unsigned x, int n ) { return ( x >> n ) | ( x << ( 32 - n ) ); }

FD_SHRED_FN void
fd_shred_core_sha256_block( unsigned h[ 8 ], unsigned char const * p ) {
  const unsigned K[ 64 ] = {
    0x428a2f98U,0x71374491U,0xb5c0fbcfU,0xe9b5dba5U,0x3956c25bU,0x59f111f1U,0x923f82a4U,0xab1c5ed5U,
    0xd807aa98U,0x12835b01U,0x243185beU,0x550c7dc3U,0x72be5d74U,0x80deb1feU,0x9bdc06a7U,0xc19bf174U,
    0xe49b69c1U,0xefbe4786U,0x0fc19dc6U,0x240ca1ccU,0x2de92c6fU,0x4a7484aaU,0x5cb0a9dcU,0x76f988daU,
    0x983e5152U,0xa831c66dU,0xb00327c8U,0xbf597fc7U,0xc6e00bf3U,0xd5a79147U,0x06ca6351U,0x14292967U,
    0x27b70a85U,0x2e1b2138U,0x4d2c6dfcU,0x53380d13U,0x650a7354U,0x766a0abbU,0x81c2c92eU,0x92722c85U,
    0xa2bfe8a1U,0xa81a664bU,0xc24b8b70U,0xc76c51a3U,0xd192e819U,0xd6990624U,0xf40e3585U,0x106aa070U,
    0x19a4c116U,0x1e376c08U,0x2748774cU,0x34b0bcb5U,0x391c0cb3U,0x4ed8aa4aU,0x5b9cca4fU,0x682e6ff3U,
    0x748f82eeU,0x78a5636fU,0x84c87814U,0x8cc70208U,0x90befffaU,0xa4506cebU,0xbef9a3f7U,0xc67178f2U };
  unsigned w[ 64 ];
  for( int t=0; t<16; t++ )
    w[ t ] = ( (unsigned)p[ 4*t ] << 24 ) | ( (unsigned)p[ 4*t+1 ] << 16 ) | ( (unsigned)p[ 4*t+2 ] << 8 ) | (unsigned)p[ 4*t+3 ];
  for( int t=16; t<64; t++ ) {
    unsigned s0 = fd_shred_core_ror( w[ t-15 ], 7 ) ^ fd_shred_core_ror( w[ t-15 ], 18 ) ^ ( w[ t-15 ] >> 3 );
    unsigned s1 = fd_shred_core_ror( w[ t-2 ], 17 ) ^ fd_shred_core_ror( w[ t-2 ], 19 ) ^ ( w[ t-2 ] >> 10 );
    w[ t ] = w[ t-16 ] + s0 + w[ t-7 ] + s1;
  }
  unsigned a = h[ 0 ], b = h[ 1 ], c = h[ 2 ], d = h[ 3 ], e = h[ 4 ], f = h[ 5 ], g = h[ 6 ], hh = h[ 7 ];
  for( int t=0; t<64; t++ ) {
    unsigned t1 = hh + ( fd_shred_core_ror( e, 6 ) ^ fd_shred_core_ror( e, 11 ) ^ fd_shred_core_ror( e, 25 ) )
                + ( ( e & f ) ^ ( ~e & g ) ) + K[ t ] + w[ t ];
    unsigned t2 = ( fd_shred_core_ror( a, 2 ) ^ fd_shred_core_ror( a, 13 ) ^ fd_shred_core_ror( a, 22 ) )
                + ( ( a & b ) ^ ( a & c ) ^ ( b & c ) );
    hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  h[ 0 ] += a; h[ 1 ] += b; h[ 2 ] += c; h[ 3 ] += d; h[ 4 ] += e; h[ 5 ] += f; h[ 6 ] += g; h[ 7 ] += hh;
}

/* out = SHA-256( kind || "SOLANA_MERKLE_SHREDS_" || tag (4 bytes) || d0[0..n0)
   || d1[0..n1) ): the leaf (kind 0, "LEAF") and the node (kind 1, "NODE")
   prefixes of fd_bmtree.h:141-142 */
FD_SHRED_FN void
fd_shred_core_sha256_prefixed( unsigned char out[ 32 ], unsigned kind, char const * tag, unsigned char const * d0,
                               unsigned long n0, unsigned char const * d1, unsigned long n1 ) {
  const char mid[ 21 ] = { 'S','O','L','A','N','A','_','M','E','R','K','L','E','_','S','H','R','E','D','S','_' };
  unsigned h[ 8 ] = { 0x6a09e667U, 0xbb67ae85U, 0x3c6ef372U, 0xa54ff53aU, 0x510e527fU, 0x9b05688cU, 0x1f83d9abU, 0x5be0cd19U };
  unsigned char buf[ 64 ];
  unsigned long used = 0UL, total = FD_SHRED_CORE_PREFIX_SZ + n0 + n1;
  buf[ used++ ] = (unsigned char)kind;
  for( int i=0; i<21; i++ ) buf[ used++ ] = (unsigned char)mid[ i ];
  for( int i=0; i<4;  i++ ) buf[ used++ ] = (unsigned char)tag[ i ];
  for( int part=0; part<2; part++ ) {
    unsigned char const * d = part ? d1 : d0;
    unsigned long         n = part ? n1 : n0;
    for( unsigned long i=0UL; i<n; i++ ) {
      buf[ used++ ] = d[ i ];
      if( used==64UL ) { fd_shred_core_sha256_block( h, buf ); used = 0UL; }
    }
  }
  buf[ used++ ] = 0x80;
  if( used>56UL ) {
    while( used<64UL ) buf[ used++ ] = 0;
    fd_shred_core_sha256_block( h, buf );
    used = 0UL;
  }
  while( used<56UL ) buf[ used++ ] = 0;
  unsigned long bits = total << 3;
  for( int i=0; i<8; i++ ) buf[ 56+i ] = (unsigned char)( bits >> ( 56 - 8*i ) );
  fd_shred_core_sha256_block( h, buf );
  for( int i=0; i<8; i++ ) {
    out[ 4*i   ] = (unsigned char)( h[ i ] >> 24 ); out[ 4*i+1 ] = (unsigned char)( h[ i ] >> 16 );
    out[ 4*i+2 ] = (unsigned char)( h[ i ] >>  8 ); out[ 4*i+3 ] = (unsigned char)( h[ i ]       );
  }
}

/* Rules 1-5 on a CPU: 0 with the root written, else the code (root
   untouched). */
FD_SHRED_FN int
fd_shred_core_root( unsigned char const * s, unsigned long sz, unsigned char root[ 32 ] ) {
  fd_shred_core_t c;
  int code = fd_shred_core_judge( s, sz, &c );
  if( code ) return code;
  unsigned char node[ 32 ], next[ 32 ];
  fd_shred_core_sha256_prefixed( node, 0U, "LEAF", s + 64, c.leaf_sz, s, 0UL );
  for( unsigned l=0U; l<c.tree_depth; l++ ) {
    unsigned char const * sib = s + c.proof_off + FD_SHRED_CORE_NODE_SZ*l;
    if( ( c.shred_idx >> l ) & 1U ) fd_shred_core_sha256_prefixed( next, 1U, "NODE", sib, 20UL, node, 20UL );
    else                            fd_shred_core_sha256_prefixed( next, 1U, "NODE", node, 20UL, sib, 20UL );
    for( int i=0; i<32; i++ ) node[ i ] = next[ i ];
  }
  for( int i=0; i<32; i++ ) root[ i ] = node[ i ];
  return FD_SHRED_CORE_OK;
}

#endif
