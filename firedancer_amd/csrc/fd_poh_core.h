/* fd_poh_core.h -- the proof-of-history check of a block's microblocks
   (fd_runtime_poh_verify_wide_task, src/flamenco/runtime/fd_runtime.c:
   2007-2063) and the walk that finds them in a raw block
   (fd_runtime_block_prepare, :349-580), restated once in plain C: compiled
   into the device kernels (fd_ed25519_poh.hip, which takes the judge and does
   the hashing with fd_sha256_dev.h), the host library
   (host/fd_ed25519_hip_fronts.c) and a stand-alone sanitizer program
   (tests/poh_walk_main.c).  The includer may define FD_POH_FN (the function
   qualifiers) and FD_POH_CORE_NO_HOST (the device: the judge alone, no
   hashing and no walk); the host includes fd_shred_core.h (the portable
   SHA-256) and fd_txn_parse_core.h (the transaction sizes) first.

   A microblock is described by offsets into one byte buffer buf[0, buf_sz):
   hdr_off, its 48-byte header (hash_cnt u64 at 0x00, hash[32] at 0x08,
   txn_cnt u64 at 0x28, little-endian, at any byte address); in_off, the 32
   bytes of the state it starts from (a chained microblock's is its
   predecessor's hdr_off + 8); and the signatures sig_off[first .. last) of
   its transactions in transaction order, 64 bytes each.

   The rules, per microblock:

   1. txn_cnt == 0: k = hash_cnt, no mixin.
   2. txn_cnt  > 0: k = hash_cnt ? hash_cnt - 1 : 0, then a mixin -- so
      hash_cnt 0 and 1 give the same result with transactions (:2026).
   3. state = in; k times state = SHA256( state ) (fd_poh_append).
   4. mixin (fd_poh_mixin): state = SHA256( state || root ), root the
      fd_wbmtree32 root of the signatures: a leaf is SHA256( 0x00 || sig ), a
      node SHA256( 0x01 || left || right ), a layer of odd size duplicates its
      last node, and a single leaf is the root.
   5. 0 if state == hdr.hash, else ERR_HASH.
   6. ERR_PARSE for a descriptor the walk cannot produce: a header, an in
      state or a signature that leaves the buffer, a signature range that runs
      backwards or leaves [0, n_sig), txn_cnt > 0 with no signatures, txn_cnt
      == 0 with some.  UNSUPPORTED if k > hash_cnt_max: the one deliberate
      difference from the reference, which would hash for as long as the 64
      attacker-chosen bits of hash_cnt say (its TODO about hashes_per_slot is
      the same gap).  Such a microblock is not hashed at all.  Parse comes
      before unsupported, unsupported before hash.

   The state of a microblock with ERR_PARSE or UNSUPPORTED is 32 zero bytes. */
#ifndef FD_POH_CORE_H
#define FD_POH_CORE_H

#ifndef FD_POH_FN
#define FD_POH_FN static inline
#endif

#define FD_POH_CORE_OK           (  0)
#define FD_POH_CORE_ERR_PARSE    (-16)
#define FD_POH_CORE_UNSUPPORTED  (-18)
#define FD_POH_CORE_ERR_HASH     (-25)

#define FD_POH_CORE_HDR_SZ        48UL
#define FD_POH_CORE_HASH_CNT_CEIL (1UL<<17)   /* twice a mainnet tick's 62,500 */

FD_POH_FN unsigned long
fd_poh_core_u64( unsigned char const * p ) {
  unsigned long v = 0UL;
  for( int i=7; i>=0; i-- ) v = ( v << 8 ) | (unsigned long)p[ i ];
  return v;
}

/* a field of sz bytes at off lies inside [0, buf_sz) */
FD_POH_FN int
fd_poh_core_inside( unsigned long off, unsigned long sz, unsigned long buf_sz ) {
  return sz<=buf_sz && off<=buf_sz-sz;
}

/* Rules 1, 2 and 6 but for the places of the signatures themselves (the
   caller holds every sig_off[ first .. last ) to fd_poh_core_inside( ., 64,
   buf_sz ), ERR_PARSE): the code so far -- 0, ERR_PARSE or UNSUPPORTED --
   and, for 0, k and whether a mixin follows.  No byte is read before its
   field is known to lie inside the buffer. */
FD_POH_FN int
fd_poh_core_judge( unsigned char const * buf, unsigned long buf_sz, unsigned long hdr_off, unsigned long in_off,
                   unsigned long first, unsigned long last, unsigned long n_sig, unsigned long hash_cnt_max,
                   unsigned long * k, int * mixin ) {
  *k = 0UL; *mixin = 0;
  if( !fd_poh_core_inside( hdr_off, FD_POH_CORE_HDR_SZ, buf_sz ) ) return FD_POH_CORE_ERR_PARSE;
  if( !fd_poh_core_inside( in_off, 32UL, buf_sz ) )                return FD_POH_CORE_ERR_PARSE;
  if( !( first<=last && last<=n_sig ) )                            return FD_POH_CORE_ERR_PARSE;
  unsigned long hash_cnt = fd_poh_core_u64( buf + hdr_off );
  unsigned long txn_cnt  = fd_poh_core_u64( buf + hdr_off + 0x28UL );
  if( ( txn_cnt!=0UL )!=( last>first ) )                           return FD_POH_CORE_ERR_PARSE;
  *mixin = txn_cnt!=0UL;
  *k     = txn_cnt ? ( hash_cnt ? hash_cnt-1UL : 0UL ) : hash_cnt;
  return *k>hash_cnt_max ? FD_POH_CORE_UNSUPPORTED : FD_POH_CORE_OK;
}

#ifndef FD_POH_CORE_NO_HOST

FD_POH_FN void
fd_poh_core_sha256( unsigned char out[ 32 ], unsigned char const * msg, unsigned long sz ) {
  unsigned h[ 8 ] = { 0x6a09e667U, 0xbb67ae85U, 0x3c6ef372U, 0xa54ff53aU, 0x510e527fU, 0x9b05688cU, 0x1f83d9abU, 0x5be0cd19U };
  unsigned char blk[ 64 ];
  unsigned long at = 0UL;
  for( ; sz-at>=64UL; at+=64UL ) fd_shred_core_sha256_block( h, msg + at );
  unsigned long used = sz-at;
  for( unsigned long i=0UL; i<used; i++ ) blk[ i ] = msg[ at+i ];
  blk[ used++ ] = 0x80;
  if( used>56UL ) {
    while( used<64UL ) blk[ used++ ] = 0;
    fd_shred_core_sha256_block( h, blk );
    used = 0UL;
  }
  while( used<56UL ) blk[ used++ ] = 0;
  unsigned long bits = sz << 3;
  for( int i=0; i<8; i++ ) blk[ 56+i ] = (unsigned char)( bits >> ( 56 - 8*i ) );
  fd_shred_core_sha256_block( h, blk );
  for( int i=0; i<8; i++ ) {
    out[ 4*i   ] = (unsigned char)( h[ i ] >> 24 ); out[ 4*i+1 ] = (unsigned char)( h[ i ] >> 16 );
    out[ 4*i+2 ] = (unsigned char)( h[ i ] >>  8 ); out[ 4*i+3 ] = (unsigned char)( h[ i ]       );
  }
}

/* node = SHA256( 0x01 || l || r ); out may be l or r */
FD_POH_FN void
fd_poh_core_node( unsigned char out[ 32 ], unsigned char const * l, unsigned char const * r ) {
  unsigned char m[ 65 ];
  m[ 0 ] = 1;
  for( int i=0; i<32; i++ ) { m[ 1+i ] = l[ i ]; m[ 33+i ] = r[ i ]; }
  fd_poh_core_sha256( out, m, 65UL );
}

/* Rule 4's root of the signatures sig_off[ 0 .. cnt ) of buf, cnt >= 1,
   without a workspace.  The node over the 2^l leaf places from `at` on, of
   which those below cnt exist (at < cnt): a layer's last node stands in for
   a missing right neighbour, so a node whose right half holds no leaf is
   node( left, left ).  Recursion as deep as the tree, 32 at most. */
FD_POH_FN void
fd_poh_core_subtree( unsigned char out[ 32 ], unsigned char const * buf, unsigned long const * sig_off, unsigned long at,
                     unsigned long cnt, unsigned l ) {
  if( !l ) {
    unsigned char m[ 65 ];
    m[ 0 ] = 0;
    for( int b=0; b<64; b++ ) m[ 1+b ] = buf[ sig_off[ at ] + (unsigned long)b ];
    fd_poh_core_sha256( out, m, 65UL );
    return;
  }
  unsigned char right[ 32 ];
  unsigned long half = 1UL<<( l-1U );
  fd_poh_core_subtree( out, buf, sig_off, at, cnt, l-1U );
  if( cnt-at>half ) {
    fd_poh_core_subtree( right, buf, sig_off, at+half, cnt, l-1U );
    fd_poh_core_node( out, out, right );
  } else {
    fd_poh_core_node( out, out, out );
  }
}

FD_POH_FN void
fd_poh_core_root( unsigned char root[ 32 ], unsigned char const * buf, unsigned long const * sig_off, unsigned long cnt ) {
  unsigned l = 0U;
  while( l<63U && ( 1UL<<l )<cnt ) l++;
  fd_poh_core_subtree( root, buf, sig_off, 0UL, cnt, l );
}

/* One microblock, rules 1-6: the code, and in state (optional) the computed
   state or, for ERR_PARSE and UNSUPPORTED, zeros.  sig_off is the whole
   array of n_sig places. */
FD_POH_FN int
fd_poh_core_verify( unsigned char const * buf, unsigned long buf_sz, unsigned long hdr_off, unsigned long in_off,
                    unsigned long first, unsigned long last, unsigned long n_sig, unsigned long const * sig_off,
                    unsigned long hash_cnt_max, unsigned char * state ) {
  unsigned long k;
  int mixin;
  unsigned char s[ 32 ], root[ 32 ], m[ 64 ];
  if( state ) for( int i=0; i<32; i++ ) state[ i ] = 0;
  int code = fd_poh_core_judge( buf, buf_sz, hdr_off, in_off, first, last, n_sig, hash_cnt_max, &k, &mixin );
  if( code==FD_POH_CORE_ERR_PARSE ) return code;
  for( unsigned long j=first; j<last; j++ )
    if( !fd_poh_core_inside( sig_off[ j ], 64UL, buf_sz ) ) return FD_POH_CORE_ERR_PARSE;
  if( code ) return code;
  for( int i=0; i<32; i++ ) s[ i ] = buf[ in_off + (unsigned long)i ];
  if( k>hash_cnt_max ) k = hash_cnt_max;   /* the kernel's loop bound; never taken after the judge */
  for( unsigned long t=0UL; t<k; t++ ) fd_poh_core_sha256( s, s, 32UL );
  if( mixin ) {
    fd_poh_core_root( root, buf, sig_off + first, last-first );
    for( int i=0; i<32; i++ ) { m[ i ] = s[ i ]; m[ 32+i ] = root[ i ]; }
    fd_poh_core_sha256( s, m, 64UL );
  }
  if( state ) for( int i=0; i<32; i++ ) state[ i ] = s[ i ];
  int diff = 0;
  for( int i=0; i<32; i++ ) diff |= s[ i ] ^ buf[ hdr_off + 8UL + (unsigned long)i ];
  return diff ? FD_POH_CORE_ERR_HASH : FD_POH_CORE_OK;
}

/* The walk of fd_runtime_block_prepare over one raw block: batches until
   the buffer ends, each a u64 microblock_cnt and that many microblocks, each
   a 48-byte header and txn_cnt transactions, measured by
   fd_txn_core_parse_prefix on at most 1,232 of the bytes that remain
   (fd_runtime_parse_microblock_txns, :385).  Counts are believed only as far
   as bytes remain: nothing is allocated or looped over by a count alone,
   every iteration consumes bytes or fails.

   Returns 0 with *n_mb and *n_sig the block's microblocks and signatures,
   else ERR_PARSE: junk at the end (fewer than 8 bytes where a batch would
   begin), a short header, a failed transaction parse, and a batch with
   microblock_cnt == 0 -- the reference's collect step
   (fd_runtime_block_verify_info_collect) reads microblock index -1 of such a
   batch, so its behaviour there is undefined; this walk refuses it.  An
   empty block is 0 microblocks.

   With arrays (hdr_off non-NULL; capacities mb_cap and sig_cap, beyond
   which nothing is written -- the counts still come back): hdr_off[ i ];
   in_off[ i ], first_in_off for the block's first microblock, else
   microblock i-1's hdr_off + 8, across batch boundaries too; sig_first[ i ]
   with sig_first[ n_mb ] == n_sig (mb_cap+1 elements); sig_off[ j ].  Every
   offset has base added (a block inside a larger buffer). */
FD_POH_FN int
fd_poh_core_walk( unsigned char const * blk, unsigned long sz, unsigned long base, unsigned long first_in_off,
                  unsigned long * hdr_off, unsigned long * in_off, unsigned int * sig_first, unsigned long mb_cap,
                  unsigned long * sig_off, unsigned long sig_cap, unsigned long * n_mb, unsigned long * n_sig ) {
  unsigned long at = 0UL, mb = 0UL, sg = 0UL, prev = first_in_off;
  *n_mb = 0UL; *n_sig = 0UL;
  while( at<sz ) {
    if( sz-at<8UL ) return FD_POH_CORE_ERR_PARSE;
    unsigned long cnt = fd_poh_core_u64( blk + at );
    at += 8UL;
    if( !cnt ) return FD_POH_CORE_ERR_PARSE;
    for( unsigned long i=0UL; i<cnt; i++ ) {
      if( sz-at<FD_POH_CORE_HDR_SZ ) return FD_POH_CORE_ERR_PARSE;
      unsigned long hdr = at;
      unsigned long txn_cnt = fd_poh_core_u64( blk + at + 0x28UL );
      at += FD_POH_CORE_HDR_SZ;
      if( hdr_off && mb<mb_cap ) { hdr_off[ mb ] = base + hdr; in_off[ mb ] = prev; sig_first[ mb ] = (unsigned int)sg; }
      for( unsigned long t=0UL; t<txn_cnt; t++ ) {
        unsigned long avail = sz-at<FD_TXN_CORE_MTU ? sz-at : FD_TXN_CORE_MTU;
        unsigned long used  = fd_txn_core_parse_prefix( blk + at, avail );
        if( !used ) return FD_POH_CORE_ERR_PARSE;
        unsigned long sig_cnt = blk[ at ];
        for( unsigned long s=0UL; s<sig_cnt; s++, sg++ )
          if( hdr_off && sg<sig_cap ) sig_off[ sg ] = base + at + 1UL + 64UL*s;
        at += used;
      }
      if( sg>0xffffffffUL ) return FD_POH_CORE_ERR_PARSE;   /* sig_first is 32 bits: a block of 256 GiB */
      prev = base + hdr + 8UL;
      mb++;
    }
  }
  if( hdr_off && mb<=mb_cap ) sig_first[ mb ] = (unsigned int)sg;
  *n_mb = mb; *n_sig = sg;
  return FD_POH_CORE_OK;
}

#endif /* FD_POH_CORE_NO_HOST */
#endif /* FD_POH_CORE_H */
