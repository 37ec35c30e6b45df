/* fd_reedsol_core.h -- the Reed-Solomon parity of a leader's FEC set, what
   fd_shredder_next_fec_set does before the Merkle tree
   (src/disco/shred/fd_shredder.c:167-223 on fd_reedsol_encode_fini),
   restated once and compiled three ways: into the device parity kernel
   (fd_ed25519_reedsol.hip, hipcc: the rules; the kernel multiplies with the
   tables this header builds), into the host library
   (host/fd_ed25519_hip_fronts.c, gcc: fd_ed25519_hip_fec_parity and the
   tables an engine uploads) and into the hostile input test's stand-alone
   program (tests/reedsol_walk_main.c, gcc with sanitizers).  Adds to
   fd_fec_core.h and changes nothing of it; the includer may define
   FD_SHRED_FN (the function qualifiers).

   Reference: src/ballet/reedsol/test_reedsol.c:27-117 states the code as a
   matrix; fd_reedsol_encode_*.c computes it with an FFT, which is not
   imitated.  fd_shredder.c:159-162, 200, 219 give the protected region.

   The code.  GF(2^8) with the polynomial x^8+x^4+x^3+x^2+1 (0x11D); an
   element is its byte value, addition is XOR.  For a set of d data and p
   parity shreds (1 <= d, p <= 67), at each byte position b of the protected
   region, P_b is the polynomial of degree < d with P_b( i ) = data_i[ b ] for
   i < d (the point i is the element with byte value i), and byte b of parity
   shred j is P_b( d + j ):

     parity_j[ b ] = sum_i M_d[ j ][ i ] data_i[ b ]
     M_d[ j ][ i ] = prod_{ m != i, m < d } ( (d+j) ^ m ) / ( i ^ m )

   M_d depends on d and j only: the parity of (d, p) is the first p rows of
   the parity of (d, 67).

   The protected region.  With depth = fd_fec_core_depth( d + p ) and
   P = 1139 - 20 depth: a data shred's bytes [0x40, 0x40 + P), a code shred's
   bytes [0x59, 0x59 + P); both end where the proof begins.  P = 3 mod 4.

   Rules for a set of cnt shreds in tree order, on top of fd_fec_core.h's
   rules 1 and 2 and with their priority -- shred by shred in set order, the
   first failing shred decides, per shred fd_fec_core_judge's code first:

     7  a data shred that stands behind a code shred                 ERR_SET
        a data shred at place 67 or beyond (more than 67 data)       ERR_SET
        a data shred that is the set's last (no parity)              ERR_SET
        a code shred with d the number of shreds before the set's first code
          shred: d == 0, data_cnt != d or code_cnt != cnt - d (which covers
          more than 67 parity: rule 2 bounds code_cnt)               ERR_SET
     8  a set with a nonzero code has no byte of any of its shreds written;
        in a set with code 0 exactly the bytes [0x59, 0x59 + P) of every code
        shred are written

   Rule 2 lets a code shred's claimed data_cnt differ from the set's real
   split, which the seal does not care about; the parity must.

   The other direction: recovering a received set, the second half of
   fd_fec_resolver_add_shred (src/disco/shred/fd_fec_resolver.c:474-594 on
   fd_reedsol_recover_fini, src/ballet/reedsol/fd_reedsol.c:34-77,
   fd_reedsol_recover_32.c:10-30 and 143-162; its FFT and its pi tables are
   not imitated), compiled the same three ways (fd_ed25519_recover.hip,
   fd_ed25519_hip_fec_recover, tests/recover_walk_main.c).  A set is
   cnt = d + p slots in tree order with one erased byte per slot (0: received,
   nonzero: erased).  The basis R is the first d received slots in set order;
   every other slot e is a target, and byte b of its region is

     v_e[ b ] = sum_{r in R} L[ e ][ r ] v_r[ b ]
     L[ e ][ r ] = N_e / ( ( e ^ r ) D_r )
     N_e = prod_{m in R} ( e ^ m ),  D_r = prod_{m in R, m != r} ( r ^ m )

   -- the Lagrange form of the one polynomial of degree < d through the basis
   (the point of slot i is the byte value i), in logarithms d additions per
   N_e and per D_r and one table look-up per coefficient.  An erased target
   is written; a received one is compared.

   Rules, numbered on.  The first failing slot in set order decides among the
   per-slot rules; then the set-level rules apply in the order given.

     9  per slot: a received slot is judged by fd_fec_core_judge    its code
        with d the data_cnt of the set's first received code shred in set
        order that fd_fec_core_judge passes (cnt when there is none):
        an erased slot (not read) whose shred_sz is below 1203 at a place
          j < d or below 1228 at a place j >= d                      ERR_PARSE
        a received data shred at a place j >= d                      ERR_SET
        a received code shred with data_cnt != d or code_cnt != cnt - d
          (its place, data_cnt + code.idx, is then >= d)             ERR_SET
    10  no received code shred (the resolver learns data_cnt only from one)
                                                                     ERR_SET
        fewer than d received                                        ERR_PARTIAL
        a received target that differs from its recomputed region in any
          byte                                                       ERR_CORRUPT
    11  on the set as it would stand after recovery (fd_fec_resolver.c:546-572):
        a recovered data shred (its first 0x19 region bytes are its header
          from 0x40 on) that fd_fec_core_judge does not pass at its place as
          a shred of 1203 bytes                                      ERR_SET
        a data shred whose slot, version, fec_set_idx or parent_off, or a
          received code shred whose slot, version or fec_set_idx, is not
          data shred 0's                                             ERR_SET
    12  a set with a nonzero code has no byte of any slot written; in a set
        with code 0 nothing of a received slot is written, an erased data
        slot gets bytes [0, 64) (the signature of the set's first received
        shred) and [0x40, 0x40 + P), an erased code slot d + i gets [0, 64)
        likewise, the header of fd_fec_resolver.c:515-524 in [0x40, 0x59)
        (variant 0x40 | depth; slot, version and fec_set_idx of the first
        received code shred; idx = that shred's idx - its code.idx + i;
        data_cnt d, code_cnt p, code.idx i) and [0x59, 0x59 + P).  The proof
        bytes are the seal's; bytes beyond 1203 or 1228 are not written. */
#ifndef FD_REEDSOL_CORE_H
#define FD_REEDSOL_CORE_H

#include "fd_fec_core.h"

#define FD_REEDSOL_CORE_MAX        FD_SHRED_CORE_IDX_MAX   /* 67 data, 67 parity */
#define FD_REEDSOL_CORE_DATA_AT    0x40U                   /* the protected region of a data shred ... */
#define FD_REEDSOL_CORE_CODE_AT    FD_SHRED_CORE_CODE_HDR_SZ   /* ... and of a code shred */
#define FD_REEDSOL_CORE_REGION( depth ) ( 1139U - 20U*(depth) )

/* The tables of the device kernel, as one block of bytes:
     [0, 8192)        for every c, 32 bytes: c v for v < 8, c (v<<3) for
                      v < 8, c (v<<6) for v < 4, 12 bytes of zero --
                      multiplication by c is GF(2)-linear, so
                      c x = T0[ x&7 ] ^ T1[ (x>>3)&7 ] ^ T2[ x>>6 ]
     [8192, +152626)  M_d for d = 1..67, 67 rows of d bytes each, M_d at
                      8192 + 67 d (d-1) / 2
     [160832, +768)   fd_reedsol_core_gf_t: exp[ 512 ], log[ 256 ] (the
                      recover kernel builds its coefficients from them) */
#define FD_REEDSOL_CORE_MUL_BYTES  8192UL
#define FD_REEDSOL_CORE_MAT_AT( d ) ( FD_REEDSOL_CORE_MUL_BYTES + 67UL*(unsigned long)(d)*( (unsigned long)(d)-1UL )/2UL )
#define FD_REEDSOL_CORE_GF_AT      ( ( FD_REEDSOL_CORE_MAT_AT( 68 ) + 15UL ) & ~15UL )   /* 160,818 up to 160,832 */
#define FD_REEDSOL_CORE_TAB_BYTES  ( FD_REEDSOL_CORE_GF_AT + 768UL )                      /* 161,600 */

/* the field: exp[ k ] = 2^k for k < 510 (twice around, so that a sum of two
   logarithms needs no reduction), log[ x ] for x != 0 */
typedef struct {
  unsigned char exp[ 512 ];
  unsigned char log[ 256 ];
} fd_reedsol_core_gf_t;

FD_SHRED_FN void
fd_reedsol_core_gf_init( fd_reedsol_core_gf_t * gf ) {
  unsigned x = 1U;
  for( unsigned k=0U; k<255U; k++ ) {
    gf->exp[ k ] = (unsigned char)x; gf->exp[ k+255U ] = (unsigned char)x;
    gf->log[ x ] = (unsigned char)k;
    x <<= 1;
    if( x & 0x100U ) x ^= 0x11DU;
  }
  gf->exp[ 510 ] = gf->exp[ 0 ]; gf->exp[ 511 ] = gf->exp[ 1 ];
  gf->log[ 0 ] = 0U;   /* never read */
}

FD_SHRED_FN unsigned
fd_reedsol_core_mul( fd_reedsol_core_gf_t const * gf, unsigned a, unsigned b ) {
  return ( a && b ) ? gf->exp[ (unsigned)gf->log[ a ] + gf->log[ b ] ] : 0U;
}

/* row j of M_d: row[ i ] for i < d; 1 <= d <= 67, j < 67 (d + j <= 133, so
   the point d+j is no data point and no factor is zero) */
FD_SHRED_FN void
fd_reedsol_core_row( fd_reedsol_core_gf_t const * gf, unsigned d, unsigned j, unsigned char * row ) {
  unsigned x = d + j, num = 0U;
  for( unsigned m=0U; m<d; m++ ) num += gf->log[ x ^ m ];
  for( unsigned i=0U; i<d; i++ ) {
    unsigned den = 0U;
    for( unsigned m=0U; m<d; m++ ) if( m!=i ) den += gf->log[ i ^ m ];
    /* num - log( x^i ) - den mod 255, kept positive: den < 67*255 */
    unsigned l = ( num - gf->log[ x ^ i ] + 255U*68U - den ) % 255U;
    row[ i ] = gf->exp[ l ];
  }
}

/* the device kernel's tables: tab[ 0 .. FD_REEDSOL_CORE_TAB_BYTES ) */
FD_SHRED_FN void
fd_reedsol_core_tables( unsigned char * tab ) {
  fd_reedsol_core_gf_t gf;
  fd_reedsol_core_gf_init( &gf );
  for( unsigned c=0U; c<256U; c++ ) {
    unsigned char * t = tab + 32U*c;
    for( unsigned v=0U; v<8U; v++ ) {
      t[ v ]      = (unsigned char)fd_reedsol_core_mul( &gf, c, v );
      t[ 8U + v ] = (unsigned char)fd_reedsol_core_mul( &gf, c, v << 3 );
    }
    for( unsigned v=0U; v<4U; v++ ) t[ 16U + v ] = (unsigned char)fd_reedsol_core_mul( &gf, c, v << 6 );
    for( unsigned v=20U; v<32U; v++ ) t[ v ] = 0U;
  }
  for( unsigned d=1U; d<=FD_REEDSOL_CORE_MAX; d++ )
    for( unsigned j=0U; j<FD_REEDSOL_CORE_MAX; j++ )
      fd_reedsol_core_row( &gf, d, j, tab + FD_REEDSOL_CORE_MAT_AT( d ) + (unsigned long)j*d );
  for( unsigned long q=FD_REEDSOL_CORE_MAT_AT( 68 ); q<FD_REEDSOL_CORE_GF_AT; q++ ) tab[ q ] = 0U;
  for( unsigned k=0U; k<512U; k++ ) tab[ FD_REEDSOL_CORE_GF_AT + k ] = gf.exp[ k ];
  for( unsigned k=0U; k<256U; k++ ) tab[ FD_REEDSOL_CORE_GF_AT + 512UL + k ] = gf.log[ k ];
}

/* Rule 7 for shred j of a set of cnt, once fd_fec_core_judge has passed it:
   d is the number of shreds in front of the set's first shred that is no
   data shred fd_fec_core_judge passes (cnt when there is none) -- when that
   shred is no code shred it fails ahead of every shred this rule could fail
   behind it, so what d means there does not matter. */
FD_SHRED_FN int
fd_reedsol_core_judge( unsigned char const * s, unsigned cnt, unsigned j, unsigned d ) {
  if( ( s[ 0x40 ] & 0xf0U )==0x80U ) {
    if( ( j>d ) | ( j>=FD_REEDSOL_CORE_MAX ) | ( j+1U==cnt ) ) return FD_FEC_CORE_ERR_SET;
    return FD_FEC_CORE_OK;
  }
  if( d==0U || fd_shred_core_u16( s + 0x53 )!=d || fd_shred_core_u16( s + 0x55 )!=cnt-d ) return FD_FEC_CORE_ERR_SET;
  return FD_FEC_CORE_OK;
}

/* Rules 1, 2 and 7 on a CPU for the set shreds[shred_off[j] .. +shred_sz[j]),
   j < cnt: 0 with *d_out the number of data shreds, else the set's code. */
FD_SHRED_FN int
fd_reedsol_core_set( unsigned char const * shreds, unsigned long const * shred_off, unsigned int const * shred_sz,
                     unsigned long cnt, unsigned * d_out ) {
  if( ( cnt==0UL ) | ( cnt>FD_FEC_CORE_CNT_MAX ) ) return FD_FEC_CORE_ERR_SET;
  if( !shreds || !shred_off || !shred_sz ) return FD_FEC_CORE_ERR_PARSE;
  unsigned n = (unsigned)cnt, d = n;
  for( unsigned j=0U; j<n; j++ ) {
    fd_shred_core_t c;
    unsigned char const * s = shreds + shred_off[ j ];
    int code = fd_fec_core_judge( s, shred_sz[ j ], n, j, &c );
    if( code ) return code;
    if( ( d==n ) & ( ( s[ 0x40 ] & 0xf0U )!=0x80U ) ) d = j;
    code = fd_reedsol_core_judge( s, n, j, d );
    if( code ) return code;
  }
  *d_out = d;
  return FD_FEC_CORE_OK;
}

/* The plain encoder of one set: 0 with the parity regions of its code shreds
   written in place (rule 8), else the set's code and nothing written. */
FD_SHRED_FN int
fd_reedsol_core_encode( unsigned char * shreds, unsigned long const * shred_off, unsigned int const * shred_sz,
                        unsigned long cnt ) {
  unsigned d = 0U;
  int code = fd_reedsol_core_set( shreds, shred_off, shred_sz, cnt, &d );
  if( code ) return code;
  unsigned n = (unsigned)cnt, region = FD_REEDSOL_CORE_REGION( fd_fec_core_depth( n ) );
  fd_reedsol_core_gf_t gf;
  fd_reedsol_core_gf_init( &gf );
  for( unsigned j=0U; j<n-d; j++ ) {
    unsigned char row[ FD_REEDSOL_CORE_MAX ];
    fd_reedsol_core_row( &gf, d, j, row );
    unsigned char * out = shreds + shred_off[ d+j ] + FD_REEDSOL_CORE_CODE_AT;
    for( unsigned b=0U; b<region; b++ ) out[ b ] = 0U;
    for( unsigned i=0U; i<d; i++ ) {
      unsigned char const * in = shreds + shred_off[ i ] + FD_REEDSOL_CORE_DATA_AT;
      unsigned lc = gf.log[ row[ i ] ];   /* row[ i ] != 0: a product of nonzero factors */
      for( unsigned b=0U; b<region; b++ ) if( in[ b ] ) out[ b ] ^= gf.exp[ lc + gf.log[ in[ b ] ] ];
    }
  }
  return FD_FEC_CORE_OK;
}

/* ---- recovery (rules 9-12) ---- */

#define FD_REEDSOL_CORE_ERR_PARTIAL (-23)
#define FD_REEDSOL_CORE_ERR_CORRUPT (-24)
#define FD_REEDSOL_CORE_HDR_BYTES   0x19U   /* a shred's bytes [0x40, 0x59): what rule 11 reads of a data shred */

/* where the protected region of slot j starts in its shred */
FD_SHRED_FN unsigned
fd_reedsol_core_region_at( unsigned j, unsigned d ) { return j<d ? FD_REEDSOL_CORE_DATA_AT : FD_REEDSOL_CORE_CODE_AT; }

/* Rule 9 for slot j once d is known; a received slot has passed
   fd_fec_core_judge, an erased slot is not read (s may be anything). */
FD_SHRED_FN int
fd_reedsol_core_recover_judge( unsigned char const * s, unsigned long sz, int erased, unsigned cnt, unsigned j, unsigned d ) {
  if( erased ) return sz>=( j<d ? FD_SHRED_CORE_MIN_SZ : FD_SHRED_CORE_MAX_SZ ) ? FD_FEC_CORE_OK : FD_FEC_CORE_ERR_PARSE;
  if( ( s[ 0x40 ] & 0xf0U )==0x80U ) return j>=d ? FD_FEC_CORE_ERR_SET : FD_FEC_CORE_OK;
  if( fd_shred_core_u16( s + 0x53 )!=d || fd_shred_core_u16( s + 0x55 )!=cnt-d ) return FD_FEC_CORE_ERR_SET;
  return FD_FEC_CORE_OK;
}

/* log D_r mod 255 for the basis slot r, and log N_e mod 255 for the target
   e, over the d basis slots basis[ 0 .. d ): d additions each */
FD_SHRED_FN unsigned
fd_reedsol_core_log_d( fd_reedsol_core_gf_t const * gf, unsigned char const * basis, unsigned d, unsigned r ) {
  unsigned l = 0U;
  for( unsigned m=0U; m<d; m++ ) if( basis[ m ]!=r ) l += gf->log[ r ^ basis[ m ] ];
  return l % 255U;
}

FD_SHRED_FN unsigned
fd_reedsol_core_log_n( fd_reedsol_core_gf_t const * gf, unsigned char const * basis, unsigned d, unsigned e ) {
  unsigned l = 0U;
  for( unsigned m=0U; m<d; m++ ) l += gf->log[ e ^ basis[ m ] ];   /* e is no basis slot: no factor is zero */
  return l % 255U;
}

/* L[ e ][ r ] from log N_e and log D_r, both below 255 */
FD_SHRED_FN unsigned
fd_reedsol_core_coef( fd_reedsol_core_gf_t const * gf, unsigned log_n, unsigned log_d, unsigned e, unsigned r ) {
  return gf->exp[ ( log_n + 510U - gf->log[ e ^ r ] - log_d ) % 255U ];
}

/* Rule 11 for a recovered data shred at place j whose bytes [0x40, 0x59) are
   h: fd_fec_core_judge on a shred of 1203 bytes with that header (a code
   variant does not parse at that size, so what passes is a data shred). */
FD_SHRED_FN int
fd_reedsol_core_hdr_judge( unsigned char const * h, unsigned cnt, unsigned j ) {
  unsigned char s[ FD_SHRED_CORE_CODE_HDR_SZ ];
  for( unsigned b=0U; b<0x40U; b++ ) s[ b ] = 0U;
  for( unsigned b=0U; b<FD_REEDSOL_CORE_HDR_BYTES; b++ ) s[ 0x40U+b ] = h[ b ];
  fd_shred_core_t c;
  return fd_fec_core_judge( s, FD_SHRED_CORE_MIN_SZ, cnt, j, &c ) ? FD_FEC_CORE_ERR_SET : FD_FEC_CORE_OK;
}

/* Rule 11's agreement of a shred's header h (its bytes from 0x40 on) with
   data shred 0's: slot (0x41, 8 bytes), version (0x4d, 2), fec_set_idx
   (0x4f, 4) and, of a data shred, parent_off (0x53, 2) */
FD_SHRED_FN int
fd_reedsol_core_hdr_agree( unsigned char const * h, unsigned char const * h0, int is_data ) {
  unsigned diff = 0U;
  for( unsigned b=0x01U; b<0x09U; b++ ) diff |= (unsigned)( h[ b ] ^ h0[ b ] );
  for( unsigned b=0x0dU; b<0x13U; b++ ) diff |= (unsigned)( h[ b ] ^ h0[ b ] );
  if( is_data ) for( unsigned b=0x13U; b<0x15U; b++ ) diff |= (unsigned)( h[ b ] ^ h0[ b ] );
  return diff ? FD_FEC_CORE_ERR_SET : FD_FEC_CORE_OK;
}

/* Rule 12: byte k < 0x19 of the header (from 0x40 on) of the recovered code
   shred d + i, ref the bytes from 0x40 on of the set's first received code
   shred */
FD_SHRED_FN unsigned
fd_reedsol_core_code_hdr_byte( unsigned char const * ref, unsigned depth, unsigned d, unsigned p, unsigned i, unsigned k ) {
  if( k==0U ) return 0x40U | depth;
  if( ( k>=0x09U ) & ( k<0x0dU ) ) {
    unsigned idx = fd_shred_core_u32( ref + 0x09 ) - fd_shred_core_u16( ref + 0x17 ) + i;
    return ( idx >> ( 8U*( k-0x09U ) ) ) & 0xffU;
  }
  if( k<0x13U ) return ref[ k ];
  unsigned v = k<0x15U ? d : k<0x17U ? p : i;
  return ( v >> ( 8U*( ( k-0x13U ) & 1U ) ) ) & 0xffU;
}

/* Rules 9 and 10 up to ERR_PARTIAL on a CPU: 0 with *d_out, the basis slots
   basis[ 0 .. d ), and the set's first received slot and first received code
   shred, else the set's code. */
FD_SHRED_FN int
fd_reedsol_core_recover_set( unsigned char const * shreds, unsigned long const * shred_off, unsigned int const * shred_sz,
                             unsigned char const * erased, unsigned long cnt, unsigned * d_out, unsigned char * basis,
                             unsigned * first_rcvd, unsigned * first_code ) {
  if( ( cnt==0UL ) | ( cnt>FD_FEC_CORE_CNT_MAX ) ) return FD_FEC_CORE_ERR_SET;
  if( !shreds || !shred_off || !shred_sz || !erased ) return FD_FEC_CORE_ERR_PARSE;
  unsigned n = (unsigned)cnt, d = n, fc = n, fr = n;
  for( unsigned j=0U; j<n; j++ ) {
    if( erased[ j ] ) continue;
    fd_shred_core_t c;
    unsigned char const * s = shreds + shred_off[ j ];
    if( fr==n ) fr = j;
    if( !fd_fec_core_judge( s, shred_sz[ j ], n, j, &c ) && ( s[ 0x40 ] & 0xf0U )==0x40U ) { fc = j; d = fd_shred_core_u16( s + 0x53 ); break; }
  }
  for( unsigned j=0U; j<n; j++ ) {
    unsigned char const * s = shreds + shred_off[ j ];
    if( !erased[ j ] ) {
      fd_shred_core_t c;
      int code = fd_fec_core_judge( s, shred_sz[ j ], n, j, &c );
      if( code ) return code;
    }
    int code = fd_reedsol_core_recover_judge( s, shred_sz[ j ], erased[ j ]!=0U, n, j, d );
    if( code ) return code;
  }
  if( fc==n ) return FD_FEC_CORE_ERR_SET;
  unsigned got = 0U;
  for( unsigned j=0U; ( j<n ) & ( got<d ); j++ ) if( !erased[ j ] ) basis[ got++ ] = (unsigned char)j;
  if( got<d ) return FD_REEDSOL_CORE_ERR_PARTIAL;
  *d_out = d; *first_rcvd = fr; *first_code = fc;
  return FD_FEC_CORE_OK;
}

/* the first nb bytes of target e's region from the basis, into out */
FD_SHRED_FN void
fd_reedsol_core_recover_row( fd_reedsol_core_gf_t const * gf, unsigned char const * shreds, unsigned long const * shred_off,
                             unsigned char const * basis, unsigned char const * log_d, unsigned d, unsigned e, unsigned nb,
                             unsigned char * out ) {
  unsigned log_n = fd_reedsol_core_log_n( gf, basis, d, e );
  for( unsigned b=0U; b<nb; b++ ) out[ b ] = 0U;
  for( unsigned i=0U; i<d; i++ ) {
    unsigned r = basis[ i ];
    unsigned char const * in = shreds + shred_off[ r ] + fd_reedsol_core_region_at( r, d );
    unsigned lc = gf->log[ fd_reedsol_core_coef( gf, log_n, log_d[ i ], e, r ) ];   /* a coefficient is no zero */
    for( unsigned b=0U; b<nb; b++ ) if( in[ b ] ) out[ b ] ^= gf->exp[ lc + gf->log[ in[ b ] ] ];
  }
}

/* The plain decoder of one set: 0 with its erased slots written as rule 12
   says, else the set's code and nothing written. */
FD_SHRED_FN int
fd_reedsol_core_recover( unsigned char * shreds, unsigned long const * shred_off, unsigned int const * shred_sz,
                         unsigned char const * erased, unsigned long cnt ) {
  unsigned d = 0U, first_rcvd = 0U, first_code = 0U;
  unsigned char basis[ FD_REEDSOL_CORE_MAX ], log_d[ FD_REEDSOL_CORE_MAX ];
  int code = fd_reedsol_core_recover_set( shreds, shred_off, shred_sz, erased, cnt, &d, basis, &first_rcvd, &first_code );
  if( code ) return code;
  unsigned n = (unsigned)cnt, depth = fd_fec_core_depth( n ), region = FD_REEDSOL_CORE_REGION( depth );
  fd_reedsol_core_gf_t gf;
  fd_reedsol_core_gf_init( &gf );
  for( unsigned i=0U; i<d; i++ ) log_d[ i ] = (unsigned char)fd_reedsol_core_log_d( &gf, basis, d, basis[ i ] );
  /* nothing is stored before the received targets are compared and the recovered headers judged */
  unsigned char row[ FD_REEDSOL_CORE_REGION( 0 ) ];
  unsigned char hdr[ FD_REEDSOL_CORE_MAX ][ FD_REEDSOL_CORE_HDR_BYTES ];
  for( unsigned e=basis[ d-1U ]+1U; e<n; e++ ) {   /* a received slot behind the last basis slot is a target */
    if( erased[ e ] ) continue;
    unsigned char const * have = shreds + shred_off[ e ] + fd_reedsol_core_region_at( e, d );
    unsigned diff = 0U;
    fd_reedsol_core_recover_row( &gf, shreds, shred_off, basis, log_d, d, e, region, row );
    for( unsigned b=0U; b<region; b++ ) diff |= (unsigned)( row[ b ] ^ have[ b ] );
    if( diff ) return FD_REEDSOL_CORE_ERR_CORRUPT;
  }
  for( unsigned j=0U; j<d; j++ ) {
    if( erased[ j ] ) {
      fd_reedsol_core_recover_row( &gf, shreds, shred_off, basis, log_d, d, j, FD_REEDSOL_CORE_HDR_BYTES, hdr[ j ] );
      if( fd_reedsol_core_hdr_judge( hdr[ j ], n, j ) ) return FD_FEC_CORE_ERR_SET;
    } else {
      for( unsigned b=0U; b<FD_REEDSOL_CORE_HDR_BYTES; b++ ) hdr[ j ][ b ] = shreds[ shred_off[ j ] + 0x40U + b ];
    }
    if( fd_reedsol_core_hdr_agree( hdr[ j ], hdr[ 0 ], 1 ) ) return FD_FEC_CORE_ERR_SET;
  }
  for( unsigned j=d; j<n; j++ )
    if( !erased[ j ] && fd_reedsol_core_hdr_agree( shreds + shred_off[ j ] + 0x40U, hdr[ 0 ], 0 ) ) return FD_FEC_CORE_ERR_SET;
  /* rule 12 */
  unsigned char const * sig = shreds + shred_off[ first_rcvd ];
  unsigned char const * ref = shreds + shred_off[ first_code ] + 0x40U;
  for( unsigned e=0U; e<n; e++ ) {
    if( !erased[ e ] ) continue;
    unsigned char * out = shreds + shred_off[ e ];
    for( unsigned b=0U; b<64U; b++ ) out[ b ] = sig[ b ];
    if( e>=d )
      for( unsigned k=0U; k<FD_REEDSOL_CORE_HDR_BYTES; k++ )
        out[ 0x40U+k ] = (unsigned char)fd_reedsol_core_code_hdr_byte( ref, depth, d, n-d, e-d, k );
    fd_reedsol_core_recover_row( &gf, shreds, shred_off, basis, log_d, d, e, region, out + fd_reedsol_core_region_at( e, d ) );
  }
  return FD_FEC_CORE_OK;
}

#endif
