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
   split, which the seal does not care about; the parity must. */
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
                      8192 + 67 d (d-1) / 2 */
#define FD_REEDSOL_CORE_MUL_BYTES  8192UL
#define FD_REEDSOL_CORE_MAT_AT( d ) ( FD_REEDSOL_CORE_MUL_BYTES + 67UL*(unsigned long)(d)*( (unsigned long)(d)-1UL )/2UL )
#define FD_REEDSOL_CORE_TAB_BYTES  FD_REEDSOL_CORE_MAT_AT( 68 )   /* 160,818 */

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

#endif
