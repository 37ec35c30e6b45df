/* fd_sha256_dev.h -- the Merkle root of a shred for gfx950, one shred per
   lane: SHA-256 of the prefixed leaf (about 17 blocks) and of the prefixed
   nodes up the inclusion proof (2 blocks a layer), the hashes of
   fd_shred_core.h's leaf and walk rules (src/ballet/bmtree/fd_bmtree.c:51-68,
   :78-130; the function itself src/ballet/sha256/fd_sha256.c).  FIPS 180-4:
   64 rounds of 32-bit big-endian arithmetic per 64-byte block.

   Shred bytes are read as fd_sha512_dev.h reads messages: dword-aligned
   16-byte loads straight from the shred buffer (a shred may start at any
   byte), realigned and byte-swapped in registers (v_perm_b32), the next
   block's loads in flight while the current block is compressed.  Both
   prefixes are 26 bytes, so the hashed bytes sit 2 bytes off the word grid
   of the hash: the leaf is read as the 26 + P bytes that end where the
   leaf data ends, its first 26 then replaced by the prefix; a node's two
   20-byte children are moved over by funnel shifts.  Padding and the
   length are synthesized in registers.

   The includer provides FD_DEV, <stdint.h>, uint4 and fd_shred_core.h. */
#pragma once

__constant__ uint32_t fd_sha256_dev_k[64] = {
  0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
  0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
  0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
  0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
  0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
  0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
  0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
  0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u,
};

/* A rotation is one v_alignbit_b32 (a funnel shift of the word with
   itself), xor3 / maj / ch one v_bitop3_b32 each (truth-table index =
   a<<2 | b<<1 | c), as in fd_sha512_dev.h on the halves of its words. */
FD_DEV uint32_t sha256_ror(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, n); }
FD_DEV uint32_t sha256_xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
FD_DEV uint32_t sha256_maj(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8); }
FD_DEV uint32_t sha256_ch(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xCA); }

/* 16 rounds; the schedule is a rolling 16-word window, the round constants
   are read through the scalar cache */
template <bool SCHED>
FD_DEV void sha256_rounds16(uint32_t (&v)[8], uint32_t (&w)[16], int r0) {
  uint32_t a = v[0], b = v[1], c = v[2], d = v[3], e = v[4], f = v[5], g = v[6], hh = v[7];
#pragma unroll
  for (int r = 0; r < 16; r++) {
    if (SCHED) {
      const uint32_t w15 = w[(r + 1) & 15], w2 = w[(r + 14) & 15];
      const uint32_t s0 = sha256_xor3(sha256_ror(w15, 7), sha256_ror(w15, 18), w15 >> 3);
      const uint32_t s1 = sha256_xor3(sha256_ror(w2, 17), sha256_ror(w2, 19), w2 >> 10);
      w[r] += s0 + w[(r + 9) & 15] + s1;
    }
    const uint32_t S1 = sha256_xor3(sha256_ror(e, 6), sha256_ror(e, 11), sha256_ror(e, 25));
    const uint32_t t1 = hh + S1 + sha256_ch(e, f, g) + fd_sha256_dev_k[r0 + r] + w[r];
    const uint32_t S0 = sha256_xor3(sha256_ror(a, 2), sha256_ror(a, 13), sha256_ror(a, 22));
    const uint32_t mj = sha256_maj(a, b, c);
    hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + S0 + mj;
  }
  v[0] = a; v[1] = b; v[2] = c; v[3] = d; v[4] = e; v[5] = f; v[6] = g; v[7] = hh;
}

/* one compression: h <- h + F(h, w); w is consumed */
FD_DEV void sha256_block(uint32_t (&h)[8], uint32_t (&w)[16]) {
  uint32_t v[8];
#pragma unroll
  for (int i = 0; i < 8; i++) v[i] = h[i];
  sha256_rounds16<false>(v, w, 0);
#pragma clang loop unroll(disable)
  for (int r0 = 16; r0 < 64; r0 += 16) sha256_rounds16<true>(v, w, r0);
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] += v[i];
}

FD_DEV void sha256_init(uint32_t (&h)[8]) {
  h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
  h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
}

/* the first 24 bytes of a prefix as big-endian words ("\0SOLANA_MERKLE_SHREDS_LE",
   "\1SOLANA_MERKLE_SHREDS_NO") and its last two in the high half of word 6
   ("AF", "DE") */
#define SHA256_PRE_W0(kind) (((uint32_t)(kind) << 24) | 0x00534F4Cu)   /* kind 'S' 'O' 'L' */
#define SHA256_PRE_W1 0x414E415Fu                                      /* "ANA_" */
#define SHA256_PRE_W2 0x4D45524Bu                                      /* "MERK" */
#define SHA256_PRE_W3 0x4C455F53u                                      /* "LE_S" */
#define SHA256_PRE_W4 0x48524544u                                      /* "HRED" */
#define SHA256_LEAF_W5 0x535F4C45u                                     /* "S_LE" */
#define SHA256_LEAF_W6 0x41460000u                                     /* "AF"   */
#define SHA256_NODE_W5 0x535F4E4Fu                                     /* "S_NO" */
#define SHA256_NODE_W6 0x44450000u                                     /* "DE"   */

/* A lane's leaf stream: stream byte q is byte shift + q of base (a dword
   address), total bytes in all; the first 26 are the prefix's place. */
struct sha256_src {
  const uint32_t* base;
  uint32_t shift;
  uint32_t total;
};

#define SHA256_CHUNKS 5  /* 20 dwords cover a 64-byte block at any byte shift */

/* 16-byte load of base dwords [j, j+4); skipped (zero) unless it holds a
   stream byte.  The chunk with the last stream byte may read up to 15 bytes
   past it: the shred buffer is readable 16 bytes past its last shred. */
FD_DEV uint4 sha256_chunk(const sha256_src& m, uint32_t j) {
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (4u * j < m.shift + m.total) __builtin_memcpy(&v, m.base + j, 16);
  return v;
}

FD_DEV void sha256_load_block(uint4 (&c)[SHA256_CHUNKS], const sha256_src& m, uint32_t b) {
#pragma unroll
  for (int q = 0; q < SHA256_CHUNKS; q++) c[q] = sha256_chunk(m, 16u * b + 4u * q);
}

FD_DEV uint32_t sha256_chunk_dword(const uint4 (&c)[SHA256_CHUNKS], int i) {
  const uint4 v = c[i >> 2];
  return (i & 3) == 0 ? v.x : (i & 3) == 1 ? v.y : (i & 3) == 2 ? v.z : v.w;
}

/* The schedule words of block b from its chunks.  FULL: every byte of the
   block is a stream byte; else bytes from `total` on are the padding (0x80,
   zeros, and in the last block the bit length). */
template <bool FULL>
FD_DEV void sha256_build_w(uint32_t (&w)[16], const uint4 (&c)[SHA256_CHUNKS], const sha256_src& m, uint32_t b,
                           uint32_t nblk) {
  /* realign and byte-swap in one v_perm_b32: byte k of the big-endian word
     is byte shift + 3 - k of {hi, lo} */
  const uint32_t sel = 0x00010203u + m.shift * 0x01010101u;
#pragma unroll
  for (int t = 0; t < 16; t++) {
    uint32_t x = __builtin_amdgcn_perm(sha256_chunk_dword(c, t + 1), sha256_chunk_dword(c, t), sel);
    if (!FULL) {
      const int n = (int)m.total - (int)(64u * b) - 4 * t;   /* stream bytes from this word on */
      const uint32_t keep = n >= 4 ? 0xffffffffu : (n > 0 ? ~(0xffffffffu >> (8 * n)) : 0u);
      const uint32_t pad = (n >= 0 && n < 4) ? (0x80000000u >> (8 * n)) : 0u;
      x = (x & keep) | pad;
      if (t == 15 && b + 1 == nblk) x = m.total << 3;        /* word 14 is zero already: total < 2^29 */
    }
    w[t] = x;
  }
}

/* h = SHA-256( s[0..total) ) as eight big-endian words, total >= 1 (the
   CRDS value hash, fd_ed25519_crds.hip); the loads are the leaf's:
   dword-aligned 16-byte chunks that may read up to 15 bytes past the last
   byte (the packet buffer is readable 16 bytes past its end).  Not
   FD_DEV: the compiler keeps its choice of inlining the chain of blocks. */
__device__ static inline void sha256_bytes(uint32_t (&h)[8], const uint8_t* s, uint32_t total) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(s);
  sha256_src m;
  m.base = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  m.shift = (uint32_t)(a & 3);
  m.total = total;
  const uint32_t nblk = (total + 9u + 63u) >> 6;
  sha256_init(h);
  uint4 cur[SHA256_CHUNKS];
  uint32_t w[16];
  sha256_load_block(cur, m, 0u);
#pragma clang loop unroll(disable)
  for (uint32_t b = 0; b < nblk; b++) {
    if (64u * b + 64u <= total) sha256_build_w<true>(w, cur, m, b, nblk);
    else sha256_build_w<false>(w, cur, m, b, nblk);
    if (b + 1 < nblk) sha256_load_block(cur, m, b + 1);
    sha256_block(h, w);
  }
}

/* h = SHA-256( leaf prefix || s[64 .. 64 + leaf_sz) ) as eight big-endian
   words; leaf_sz >= 38 (it is 839 at least), so block 0 is full */
FD_DEV void sha256_leaf(uint32_t (&h)[8], const uint8_t* s, uint32_t leaf_sz) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(s) + 64u - FD_SHRED_CORE_PREFIX_SZ;   /* inside the shred */
  sha256_src m;
  m.base = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  m.shift = (uint32_t)(a & 3);
  m.total = FD_SHRED_CORE_PREFIX_SZ + leaf_sz;
  const uint32_t nblk = (m.total + 9u + 63u) >> 6;
  sha256_init(h);
  uint4 cur[SHA256_CHUNKS];
  uint32_t w[16];
  sha256_load_block(cur, m, 0u);
  sha256_build_w<true>(w, cur, m, 0u, nblk);
  w[0] = SHA256_PRE_W0(0); w[1] = SHA256_PRE_W1; w[2] = SHA256_PRE_W2; w[3] = SHA256_PRE_W3; w[4] = SHA256_PRE_W4;
  w[5] = SHA256_LEAF_W5;
  w[6] = SHA256_LEAF_W6 | (w[6] & 0xffffu);
  sha256_load_block(cur, m, 1u);
  sha256_block(h, w);
#pragma clang loop unroll(disable)
  for (uint32_t b = 1; b < nblk; b++) {
    if (64u * b + 64u <= m.total) sha256_build_w<true>(w, cur, m, b, nblk);
    else sha256_build_w<false>(w, cur, m, b, nblk);
    if (b + 1 < nblk) sha256_load_block(cur, m, b + 1);
    sha256_block(h, w);
  }
}

/* the six aligned dwords around a 20-byte proof node at any byte address
   (the sixth only when the node is off the dword grid; it then reads up to
   3 bytes past the node) */
struct sha256_node_raw {
  uint32_t d[6];
  uint32_t shift;
};

FD_DEV void sha256_node_load(sha256_node_raw& r, const uint8_t* node) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(node);
  const uint32_t* p = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  r.shift = (uint32_t)(a & 3);
#pragma unroll
  for (int i = 0; i < 5; i++) r.d[i] = p[i];
  r.d[5] = r.shift ? p[5] : 0u;
}

/* h = SHA-256( node prefix || left[0..20) || right[0..20) ) with the running
   node h[0..5) on the side `right` says and the sibling on the other: 66
   bytes, two blocks.  Children are big-endian words; stream word 7 + i is
   the low half of child word i and the high half of child word i + 1. */
FD_DEV void sha256_node(uint32_t (&h)[8], const sha256_node_raw& r, bool right) {
  const uint32_t sel = 0x00010203u + r.shift * 0x01010101u;
  uint32_t x[10];
#pragma unroll
  for (int i = 0; i < 5; i++) {
    const uint32_t sib = __builtin_amdgcn_perm(r.d[i + 1], r.d[i], sel);
    x[i] = right ? sib : h[i];
    x[5 + i] = right ? h[i] : sib;
  }
  uint32_t w[16];
  w[0] = SHA256_PRE_W0(1); w[1] = SHA256_PRE_W1; w[2] = SHA256_PRE_W2; w[3] = SHA256_PRE_W3; w[4] = SHA256_PRE_W4;
  w[5] = SHA256_NODE_W5;
  w[6] = SHA256_NODE_W6 | (x[0] >> 16);
#pragma unroll
  for (int i = 0; i < 9; i++) w[7 + i] = __builtin_amdgcn_alignbit(x[i], x[i + 1], 16);
  const uint32_t last = (x[9] << 16) | 0x8000u;   /* stream bytes 64, 65 and the padding's 0x80 */
  sha256_init(h);
  sha256_block(h, w);
  w[0] = last;
#pragma unroll
  for (int t = 1; t < 15; t++) w[t] = 0u;
  w[15] = (FD_SHRED_CORE_PREFIX_SZ + 2u * FD_SHRED_CORE_NODE_SZ) << 3;
  sha256_block(h, w);
}

/* h = SHA-256( node prefix || left[0..20) || right[0..20) ) with both
   children given as big-endian words (registers, or LDS rows of a tree held
   by a workgroup: fd_ed25519_fec.hip); the two blocks of sha256_node */
FD_DEV void sha256_node_pair(uint32_t (&h)[8], const uint32_t (&left)[5], const uint32_t (&right)[5]) {
  uint32_t x[10];
#pragma unroll
  for (int i = 0; i < 5; i++) {
    x[i] = left[i];
    x[5 + i] = right[i];
  }
  uint32_t w[16];
  w[0] = SHA256_PRE_W0(1); w[1] = SHA256_PRE_W1; w[2] = SHA256_PRE_W2; w[3] = SHA256_PRE_W3; w[4] = SHA256_PRE_W4;
  w[5] = SHA256_NODE_W5;
  w[6] = SHA256_NODE_W6 | (x[0] >> 16);
#pragma unroll
  for (int i = 0; i < 9; i++) w[7 + i] = __builtin_amdgcn_alignbit(x[i], x[i + 1], 16);
  const uint32_t last = (x[9] << 16) | 0x8000u;   /* stream bytes 64, 65 and the padding's 0x80 */
  sha256_init(h);
  sha256_block(h, w);
  w[0] = last;
#pragma unroll
  for (int t = 1; t < 15; t++) w[t] = 0u;
  w[15] = (FD_SHRED_CORE_PREFIX_SZ + 2u * FD_SHRED_CORE_NODE_SZ) << 3;
  sha256_block(h, w);
}

/* Rules 4-5 of fd_shred_core.h for a shred fd_shred_core_judge passed: the
   root as eight big-endian words.  The next layer's sibling is loaded
   before the current layer is hashed. */
FD_DEV void sha256_shred_root(uint32_t (&h)[8], const uint8_t* s, const fd_shred_core_t& c) {
  const uint8_t* proof = s + c.proof_off;
  sha256_node_raw sib;
  if (c.tree_depth) sha256_node_load(sib, proof);
  sha256_leaf(h, s, c.leaf_sz);
#pragma clang loop unroll(disable)
  for (uint32_t l = 0; l < c.tree_depth; l++) {
    const sha256_node_raw cur = sib;
    if (l + 1 < c.tree_depth) sha256_node_load(sib, proof + FD_SHRED_CORE_NODE_SZ * (l + 1));
    sha256_node(h, cur, (c.shred_idx >> l) & 1u);
  }
}

/* ---- the proof-of-history hashes (fd_poh_core.h, fd_ed25519_poh.hip) ----

   Four fixed-size messages: the chain step SHA-256( state[32] ), the mixin
   SHA-256( state[32] || root[32] ), and the two hashes of the signature
   tree, SHA-256( 0x00 || sig[64] ) and SHA-256( 0x01 || left[32] ||
   right[32] ).  Padding and lengths are compile-time constants. */

/* the round constants as literals: where the index is a compile-time constant
   (an unrolled round) the compiler adds them to constant schedule words */
FD_DEV constexpr uint32_t sha256_k_lit(int i) {
  constexpr uint32_t k[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u,
  };
  return k[i];
}

/* the small sigmas in plain C: of a constant word they fold to a constant */
FD_DEV constexpr uint32_t sha256_s0_c(uint32_t x) { return ((x >> 7) | (x << 25)) ^ ((x >> 18) | (x << 14)) ^ (x >> 3); }
FD_DEV constexpr uint32_t sha256_s1_c(uint32_t x) { return ((x >> 17) | (x << 15)) ^ ((x >> 19) | (x << 13)) ^ (x >> 10); }

/* h <- SHA-256( h[0..8) as 32 bytes ), one compression (fd_poh_append's
   step).  Schedule words 8..15 are the constants 0x80000000, 0, ..., 0, 0x100
   and the state starts at the initial value: rounds 0..15 and schedule steps
   16..31 are unrolled with literal constants, so the eight constant words
   are never carried -- rounds 8..15 add one folded literal, steps 16..30 lose
   the terms that are zero, and round 0 starts from constants.  Rounds 32..63
   are the common loop. */
FD_DEV void sha256_chain32(uint32_t (&h)[8]) {
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = h[i];
  w[8] = 0x80000000u;
#pragma unroll
  for (int i = 9; i < 15; i++) w[i] = 0u;
  w[15] = 0x100u;
  uint32_t a = 0x6a09e667u, b = 0xbb67ae85u, c = 0x3c6ef372u, d = 0xa54ff53au;
  uint32_t e = 0x510e527fu, f = 0x9b05688cu, g = 0x1f83d9abu, hh = 0x5be0cd19u;
#pragma unroll
  for (int r = 0; r < 32; r++) {
    if (r >= 16) {
      const uint32_t w15 = w[(r + 1) & 15], w2 = w[(r + 14) & 15];
      w[r & 15] += sha256_s0_c(w15) + w[(r + 9) & 15] + sha256_s1_c(w2);
    }
    const uint32_t S1 = sha256_xor3(sha256_ror(e, 6), sha256_ror(e, 11), sha256_ror(e, 25));
    const uint32_t t1 = hh + S1 + sha256_ch(e, f, g) + (sha256_k_lit(r) + w[r & 15]);
    const uint32_t S0 = sha256_xor3(sha256_ror(a, 2), sha256_ror(a, 13), sha256_ror(a, 22));
    const uint32_t mj = sha256_maj(a, b, c);
    hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + S0 + mj;
  }
  uint32_t v[8] = {a, b, c, d, e, f, g, hh};
#pragma clang loop unroll(disable)
  for (int r0 = 32; r0 < 64; r0 += 16) sha256_rounds16<true>(v, w, r0);
  h[0] = 0x6a09e667u + v[0]; h[1] = 0xbb67ae85u + v[1]; h[2] = 0x3c6ef372u + v[2]; h[3] = 0xa54ff53au + v[3];
  h[4] = 0x510e527fu + v[4]; h[5] = 0x9b05688cu + v[5]; h[6] = 0x1f83d9abu + v[6]; h[7] = 0x5be0cd19u + v[7];
}

/* h <- SHA-256( h[0..8) || root[0..8) ) (fd_poh_mixin): the data block, then
   the padding block of a 64-byte message, all constants */
FD_DEV void sha256_mix64(uint32_t (&h)[8], const uint32_t (&root)[8]) {
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 8; i++) { w[i] = h[i]; w[8 + i] = root[i]; }
  sha256_init(h);
  sha256_block(h, w);
  w[0] = 0x80000000u;
#pragma unroll
  for (int t = 1; t < 15; t++) w[t] = 0u;
  w[15] = 64u << 3;
  sha256_block(h, w);
}

/* h = SHA-256( kind || x[0..16) as 64 bytes ), 65 bytes in two blocks: the
   one-byte prefix puts the data one byte off the word grid, so stream word i
   is the low byte of x[i-1] and the high three of x[i]; the second block is
   the last data byte, the padding's 0x80, zeros and the length */
FD_DEV void sha256_pre1_64(uint32_t (&h)[8], uint32_t kind, const uint32_t (&x)[16]) {
  uint32_t w[16];
  w[0] = (kind << 24) | (x[0] >> 8);
#pragma unroll
  for (int i = 1; i < 16; i++) w[i] = __builtin_amdgcn_alignbit(x[i - 1], x[i], 8);
  const uint32_t last = (x[15] << 24) | 0x00800000u;
  sha256_init(h);
  sha256_block(h, w);
  w[0] = last;
#pragma unroll
  for (int t = 1; t < 15; t++) w[t] = 0u;
  w[15] = 65u << 3;
  sha256_block(h, w);
}

/* the signature tree's node: h = SHA-256( 0x01 || left || right ), children
   as big-endian words (fd_wbmtree32's branch, fd_bmtree's 32-byte node with
   the 1-byte prefix) */
FD_DEV void sha256_node65(uint32_t (&h)[8], const uint32_t (&left)[8], const uint32_t (&right)[8]) {
  uint32_t x[16];
#pragma unroll
  for (int i = 0; i < 8; i++) { x[i] = left[i]; x[8 + i] = right[i]; }
  sha256_pre1_64(h, 1u, x);
}

/* the signature tree's leaf: h = SHA-256( 0x00 || sig[0..64) ), sig at any
   byte address, read as the shred leaf is: dword-aligned 16-byte loads (the
   fifth only when sig is off the dword grid; it then reads up to 15 bytes
   past the signature) realigned and byte-swapped by v_perm_b32 */
FD_DEV void sha256_leaf65(uint32_t (&h)[8], const uint8_t* sig) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(sig);
  sha256_src m;
  m.base = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  m.shift = (uint32_t)(a & 3);
  m.total = 64u;
  uint4 cur[SHA256_CHUNKS];
  uint32_t x[16];
  sha256_load_block(cur, m, 0u);
  sha256_build_w<true>(x, cur, m, 0u, 1u);
  sha256_pre1_64(h, 0u, x);
}

/* 32 bytes at any byte address as eight big-endian words: the nine aligned
   dwords around them (the ninth only when off the dword grid; it then reads
   up to 3 bytes past the field) */
FD_DEV void sha256_load32(uint32_t (&x)[8], const uint8_t* p) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  const uint32_t shift = (uint32_t)(a & 3);
  uint32_t d[9];
#pragma unroll
  for (int i = 0; i < 8; i++) d[i] = q[i];
  d[8] = shift ? q[8] : 0u;
  const uint32_t sel = 0x00010203u + shift * 0x01010101u;
#pragma unroll
  for (int i = 0; i < 8; i++) x[i] = __builtin_amdgcn_perm(d[i + 1], d[i], sel);
}
