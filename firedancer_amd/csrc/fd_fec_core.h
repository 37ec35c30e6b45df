/* fd_fec_core.h -- what fd_shredder_next_fec_set does to a filled FEC set
   before it leaves the leader (src/disco/shred/fd_shredder.c:225-260): the
   Merkle tree over the set's data and parity shreds, the root the leader
   signs and each shred's inclusion proof -- the inverse of fd_shred_core.h's
   walk -- restated once and compiled three ways: into the device tree kernel
   (fd_ed25519_fec.hip, hipcc: the rules; the kernel hashes with its own
   SHA-256), into the host library (host/fd_ed25519_hip_fronts.c, gcc:
   fd_ed25519_hip_fec_root) and into the hostile input test's stand-alone
   program (tests/fec_walk_main.c, gcc with sanitizers).  Adds to
   fd_shred_core.h and changes nothing of it; the includer may define
   FD_SHRED_FN (the function qualifiers).

   Reference: fd_shredder.c:158 (the tree depth of a set), :225-260 (leaves,
   tree, signature, proofs), src/ballet/bmtree/fd_bmtree.c:51-68 (the leaf),
   :78-130 (the node), :147-153 (fd_bmtree_depth), :216-348 (commit: an odd
   layer's last node is merged with itself, :304-306; get_proof: the sibling
   of a layer's unpaired last node is that node, :336-338).

   A set is cnt shreds in tree order, the data shreds first, then the parity
   shreds; shred j is leaf j.  Rules:

     1  cnt == 0 or cnt > 134 (67 + 67): ERR_SET, no shred read
     2  shred by shred in set order, the first failing shred decides; per
        shred, in this order:
          fd_shred_core_parse fails                          ERR_PARSE
          type neither 0x80 nor 0x40                         UNSUPPORTED
          variant & 0xf != fd_bmtree_depth( cnt ) - 1 (0 for cnt 1, else
            msb( cnt-1 ) + 1; fd_shredder.c:158)             ERR_SET
          code shred with data_cnt or code_cnt 0 or > 67     ERR_SET
          the header's index in the set (data idx - fec_set_idx mod 2^32,
            code data_cnt + code.idx, as fd_shred_core_judge) != j
                                                             ERR_SET
        The resolver's rejection of an all-zero signature does not apply:
        the signature field is an output.
     3  leaf j = SHA-256( "\0SOLANA_MERKLE_SHREDS_LEAF" || s[64 .. 64+P) ), P
        as in fd_shred_core.h; a node = SHA-256( "\1SOLANA_MERKLE_SHREDS_NODE"
        || left[0..20) || right[0..20) )
     4  a layer of m nodes has (m+1)/2 parents, node t of the next layer from
        nodes 2t and min( 2t+1, m-1 ); the root is the 32 bytes of the top
        node (of the leaf for cnt 1)
     5  proof node l of leaf j is the first 20 bytes of layer l's node
        min( (j>>l)^1, m_l-1 ), at proof_off + 20 l of the shred
     6  a set with a nonzero code has no byte of any of its shreds written */
#ifndef FD_FEC_CORE_H
#define FD_FEC_CORE_H

#include "fd_shred_core.h"

#define FD_FEC_CORE_OK          FD_SHRED_CORE_OK
#define FD_FEC_CORE_ERR_PARSE   FD_SHRED_CORE_ERR_PARSE
#define FD_FEC_CORE_UNSUPPORTED FD_SHRED_CORE_UNSUPPORTED
#define FD_FEC_CORE_ERR_SET     FD_SHRED_CORE_ERR_HEADER   /* -19: the shred front's number for a header it rejects */

#define FD_FEC_CORE_CNT_MAX   ( 2U*FD_SHRED_CORE_IDX_MAX )   /* 134 leaves */
#define FD_FEC_CORE_DEPTH_MAX 8U                             /* proof nodes of a leaf of 134 */
/* nodes of every layer of the largest tree: 134+67+34+17+9+5+3+2+1 */
#define FD_FEC_CORE_NODE_MAX  272U

/* The shreds of the set [first, last) of a batch of n as the host wrappers
   send it (fd_fec_pass.h): last - first, or 0 for a range that runs
   backwards, leaves [0, n) or holds more than CNT_MAX shreds -- a set_first
   that is no prefix sum.  0 is rule 1's ERR_SET, an empty range included,
   and no shred of such a range is read or travels.  This is the cnt of the
   three kernels (fd_ed25519_fec.hip, fd_ed25519_reedsol.hip,
   fd_ed25519_recover.hip), whose range_ok is cnt != 0; they spell the
   condition themselves, since taking it from here moved their scalar code
   (profiles/fec_pass_ab.txt): change all four together. */
FD_SHRED_FN unsigned
fd_fec_core_set_cnt( unsigned long first, unsigned long last, unsigned long n ) {
  return ( first<=last && last<=n && last-first<=FD_FEC_CORE_CNT_MAX ) ? (unsigned)( last-first ) : 0U;
}

/* fd_bmtree_depth( cnt ) - 1, the proof nodes of a leaf: cnt in [1,134] */
FD_SHRED_FN unsigned
fd_fec_core_depth( unsigned cnt ) {
  unsigned d = 0U;
  while( ( 1U << d ) < cnt ) d++;
  return d;
}

/* Rule 2 for shred j of a set of cnt: 0 with *o filled (tree_depth,
   shred_idx == j, leaf_sz, proof_off), else the shred's code.  Reads bytes
   below 0x59 only, each once the parser has proved it present. */
FD_SHRED_FN int
fd_fec_core_judge( unsigned char const * s, unsigned long sz, unsigned cnt, unsigned j, fd_shred_core_t * o ) {
  o->tree_depth = 0U; o->shred_idx = 0U; o->leaf_sz = 0U; o->proof_off = 0U;
  if( !s || !fd_shred_core_parse( s, sz ) ) return FD_FEC_CORE_ERR_PARSE;
  unsigned variant = s[ 0x40 ], type = variant & 0xf0U;
  if( ( type!=0x80U ) & ( type!=0x40U ) ) return FD_FEC_CORE_UNSUPPORTED;
  int is_data = type==0x80U;
  unsigned depth = variant & 0xfU;
  if( depth!=fd_fec_core_depth( cnt ) ) return FD_FEC_CORE_ERR_SET;
  unsigned data_cnt = 0U;
  if( !is_data ) {                                   /* sz >= 1228: the code header is there */
    data_cnt = fd_shred_core_u16( s + 0x53 );
    unsigned code_cnt = fd_shred_core_u16( s + 0x55 );
    if( ( data_cnt>FD_SHRED_CORE_IDX_MAX ) | ( code_cnt>FD_SHRED_CORE_IDX_MAX ) ) return FD_FEC_CORE_ERR_SET;
    if( ( data_cnt==0U ) | ( code_cnt==0U ) ) return FD_FEC_CORE_ERR_SET;
  }
  unsigned idx = is_data ? fd_shred_core_u32( s + 0x49 ) - fd_shred_core_u32( s + 0x4f )
                         : data_cnt + fd_shred_core_u16( s + 0x57 );
  if( idx!=j ) return FD_FEC_CORE_ERR_SET;
  o->tree_depth = depth;
  o->shred_idx  = j;
  o->leaf_sz    = 1115U - 20U*depth + 0x18U + ( is_data ? 0U : 0x19U );
  o->proof_off  = ( is_data ? FD_SHRED_CORE_MIN_SZ : FD_SHRED_CORE_MAX_SZ ) - 20U*depth;
  return FD_FEC_CORE_OK;
}

/* where layer l of a tree of cnt leaves starts in an array of all its nodes,
   layer 0 first, and how many nodes it has */
FD_SHRED_FN unsigned
fd_fec_core_layer( unsigned cnt, unsigned l, unsigned * m_out ) {
  unsigned at = 0U, m = cnt;
  for( unsigned q=0U; q<l; q++ ) { at += m; m = ( m+1U ) >> 1; }
  *m_out = m;
  return at;
}

/* Rules 1-5 on a CPU for the set shreds[shred_off[j] .. +shred_sz[j]), j <
   cnt: 0 with the root written and, when proofs is not NULL, leaf j's proof
   nodes at proofs + 20 depth j (nothing is written into the shreds); else
   the set's code, root and proofs untouched. */
FD_SHRED_FN int
fd_fec_core_root( unsigned char const * shreds, unsigned long const * shred_off, unsigned int const * shred_sz,
                  unsigned long cnt, unsigned char root[ 32 ], unsigned char * proofs ) {
  if( ( cnt==0UL ) | ( cnt>FD_FEC_CORE_CNT_MAX ) ) return FD_FEC_CORE_ERR_SET;
  if( !shreds || !shred_off || !shred_sz ) return FD_FEC_CORE_ERR_PARSE;
  unsigned char node[ FD_FEC_CORE_NODE_MAX ][ 32 ];
  unsigned n = (unsigned)cnt, depth = fd_fec_core_depth( n );
  for( unsigned j=0U; j<n; j++ ) {
    fd_shred_core_t c;
    unsigned char const * s = shreds + shred_off[ j ];
    int code = fd_fec_core_judge( s, shred_sz[ j ], n, j, &c );
    if( code ) return code;
    fd_shred_core_sha256_prefixed( node[ j ], 0U, "LEAF", s + 64, c.leaf_sz, s, 0UL );
  }
  unsigned at = 0U, m = n;
  for( unsigned l=0U; l<depth; l++ ) {
    unsigned up = at + m, pm = ( m+1U ) >> 1;
    for( unsigned t=0U; t<pm; t++ ) {
      unsigned r = 2U*t+1U<m ? 2U*t+1U : m-1U;
      fd_shred_core_sha256_prefixed( node[ up+t ], 1U, "NODE", node[ at+2U*t ], 20UL, node[ at+r ], 20UL );
    }
    at = up; m = pm;
  }
  for( int i=0; i<32; i++ ) root[ i ] = node[ at ][ i ];
  if( proofs ) {
    for( unsigned j=0U; j<n; j++ ) {
      for( unsigned l=0U; l<depth; l++ ) {
        unsigned ml, base = fd_fec_core_layer( n, l, &ml );
        unsigned sib = ( j>>l ) ^ 1U;
        if( sib>ml-1U ) sib = ml-1U;
        for( unsigned i=0U; i<FD_SHRED_CORE_NODE_SZ; i++ )
          proofs[ FD_SHRED_CORE_NODE_SZ*( (unsigned long)depth*j + l ) + i ] = node[ base+sib ][ i ];
      }
    }
  }
  return FD_FEC_CORE_OK;
}

#endif
