/* fd_ed25519_hip_internal.h -- contract between the plain-C host runtime
   (host/fd_ed25519_hip_*.c) and the HIP kernel shim
   (fd_ed25519_kernels.hip).  Only plain pointers and sizes cross it. */
#ifndef FD_ED25519_HIP_INTERNAL_H
#define FD_ED25519_HIP_INTERNAL_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Base-point table: [0..128] B in affine precomputed form (y+x, y-x, 2dxy),
   36 int32 per entry (30 used), kept in LDS by the verify kernel. */
#define FD_ED25519_BTAB_ENTRIES   129
#define FD_ED25519_BTAB_STRIDE    36
#define FD_ED25519_BTAB_INTS      (FD_ED25519_BTAB_ENTRIES * FD_ED25519_BTAB_STRIDE)

/* Wide base-point tables of the verify kernels, 128-byte entries
   (y+x, y-x, 2dxy, pad), read from HBM / L2 / MALL with each entry loaded
   ahead of its use:
     btab16   [0..2^15]B, signed radix-2^16 digits of S (full-length form), 4.2 MB
     btab_lo  [0..2^24)B, unsigned radix-2^24 digits of s_lo (half-size form), 2 GiB
     btab_hi  [0..2^24)[2^144]B, digits of s_hi, 2 GiB
   The two wide tables are shared by all engines of a device (4 GiB of the
   288 GB: s' = s_lo + 2^144 s_hi costs 6 + 5 mixed additions, against
   7 + 7 at radix 2^20 with 2 x 128 MB; the random 128-byte reads, 11 per
   signature, are prefetched a window ahead). */
#define FD_ED25519_BTAB16_ENTRIES ((1 << 15) + 1)
#define FD_ED25519_BTAB16_STRIDE  32
#define FD_ED25519_BTABW_BITS     24
#define FD_ED25519_BTABW_ENTRIES  (1 << FD_ED25519_BTABW_BITS)
#define FD_ED25519_BTABW_SHIFT    144   /* s_lo: 6 digits (bits 0..143), s_hi: 5 digits (109 bits) */
/* The compact tables (FD_ED25519_HIP_FLAG_COMPACT_TABLES): the same two
   tables at radix 2^16, [0..2^16)B and [0..2^16)[2^144]B, 8 MiB each,
   9 + 7 mixed additions per signature -- for processes that verify little
   (the drop-in's engines) and should not hold 4 GiB. */
#define FD_ED25519_BTABC_BITS     16
#define FD_ED25519_BTABC_ENTRIES  (1 << FD_ED25519_BTABC_BITS)

/* Per-lane tables in cached form, in HBM -- the half-size form's joint
   table a (-A) + r (-+R) (12 slots, fd_ed25519_kernels.hip), sized as the
   two tables [1..8](-A) and [1..8](-+R) it replaced: 2 x 8
   entries x 40 int32 per lane, laid out [wave][lane][entry][quad] (int4
   granules, lane stride 160 int4): a lookup
   reads 160 contiguous bytes of the lane's own table, so every fetched line
   is fully used (the [entry][quad][lane] layout fetched ~2.4x the table
   bytes from HBM because lanes pick different entries).  A zero digit reads
   one identity entry shared by all lanes (L2-resident) instead of a
   per-lane copy: 1/9 less table written, dsm -1.2%
   (profiles/r2_ab_atab_ident.txt).  The full-length form keeps [0..8] at
   tabA, 9 entries, extending into the (then unused) tabR half. */
#define FD_ED25519_ATAB_STRIDE 8UL
#define FD_ED25519_ATAB_BYTES_PER_WAVE (2UL * FD_ED25519_ATAB_STRIDE * 10UL * 64UL * 16UL)  /* -A and -+R tables */

#define FD_ED25519_VERIFY_BLOCK 256
#define FD_ED25519_QUAD_LANE_BYTES 864UL   /* dsm4 lane tables: 2 x 9 entries x 48 B */
/* Occupancy targets (waves per SIMD) of the phase kernels; each caps the
   kernel's register allocation (512 / waves VGPRs). */
#ifndef FD_ED25519_DSM_WAVES_PER_SIMD
#define FD_ED25519_DSM_WAVES_PER_SIMD 2
#endif
#ifndef FD_ED25519_HASH_WAVES_PER_SIMD
#define FD_ED25519_HASH_WAVES_PER_SIMD 2  /* measured: 2 (200 VGPR, no spill) beats 3 (spills) */
#endif
#ifndef FD_ED25519_SCALAR_WAVES_PER_SIMD
#define FD_ED25519_SCALAR_WAVES_PER_SIMD 4
#endif
#ifndef FD_ED25519_DECODE_WAVES_PER_SIMD
#define FD_ED25519_DECODE_WAVES_PER_SIMD 4  /* 128 VGPR: spills 292 B/lane outside the squaring loops; 1.87 -> 1.85 ms (profiles/r2_ab_decode_waves.txt) */
#endif
#define FD_ED25519_SORT_BUCKETS 64

/* Work arrays handed between the phase kernels, per signature of a chunk
   (SoA, [field][cap] so every access is one coalesced dword per lane):
     k        [8][cap]   u32  k = SHA-512(R||A||M) mod L
     sflag    [cap]      u8   S < L
     pflag    [2][cap]   u8   A, R: bit0 decode failure, bit1 small order
     pts      [2][20][cap] i32 A, R: x (10 limbs), y (10 limbs), radix 2^25.5
     hs       [19][cap]  u32  half-size scalars: c, |d|, s_lo (5 words), s_hi (4)
     hflag    [cap]      u8   bit0 d < 0, bit1 no verified half-size pair (full-length form)
     perm     [cap]      u32  hash order (length-sorted)
     fix_list [cap]      u32  signatures for the full-length form (scalar -> dsm)
   FD_ED25519_WORK_BYTES_PER_SIG bytes per signature of capacity. */
#define FD_ED25519_WORK_BYTES_PER_SIG (8UL * 4UL + 1UL + 2UL + 2UL * 20UL * 4UL + 19UL * 4UL + 1UL + 4UL + 4UL)

typedef struct {
  /* inputs (signature i = base + j for chunk-local j in [0,n)) */
  uint8_t const *  msgs;     /* message bytes (any alignment)                 */
  uint64_t const * msg_off;  /* [N] byte offset of message i in msgs          */
  uint32_t const * msg_sz;   /* [N] message size                              */
  uint8_t const *  sigs;     /* [N][64] R||S, 16-byte aligned                  */
  uint8_t const *  pubs;     /* [N][32] A, 16-byte aligned                     */
  uint8_t const *  digests;  /* [N][64] SHA-512(R||A||M) computed by the caller,
                                16-byte aligned (msgs unused); NULL: hashed here */
  int8_t *         out;      /* [N] FD_ED25519_SUCCESS / ERR_* codes           */
  uint64_t         base;
  uint64_t         n;        /* chunk size, <= cap                             */
  /* work arrays */
  uint32_t *       k;
  uint8_t *        sflag;
  uint8_t *        pflag;
  int32_t *        pts;
  uint32_t *       hs;
  uint8_t *        hflag;
  uint32_t *       fix_list;
  uint32_t *       fix_cnt;  /* 1 word: entries of fix_list                   */
  uint32_t *       work_ctr; /* 1 word: dsm items handed out (fix_cnt + 1)      */
  uint32_t *       perm;     /* [cap] hash order (length-sorted), NULL: identity */
  uint32_t *       hist;     /* [2*SORT_BUCKETS] counting-sort scratch          */
  uint64_t         cap;
  int32_t const *  btab;     /* device base-point table (FD_ED25519_BTAB_INTS) */
  int32_t const *  btab16;   /* [0..2^15]B,          [FD_ED25519_BTAB16_ENTRIES][32] */
  int32_t const *  btab_lo;  /* [0..2^24)B,          [FD_ED25519_BTABW_ENTRIES][32] */
  int32_t const *  btab_hi;  /* [0..2^24)[2^144]B,   same layout                     */
  void *           atab;     /* device scratch, waves * ATAB_BYTES_PER_WAVE    */
  int              codes_portable; /* 0: AVX-512 backend codes, 1: portable  */
  int              half_dbits;     /* longest |d| of the half-size form (fd25519_half.h) */
  int              small;          /* small chunk: fused prep kernel, no sort, dsm4 (1: a
                                      quad of lanes per signature), dsm8 (2: two quads)
                                      or dsm16 (3: two waves, prep16 before it); the
                                      full-length items by a scan of hflag (1, 2)    */
  int              full_in_prep;   /* small == 3 and atab holds a lane per signature:
                                      prep16's hash waves run the full-length items
                                      (atab slot j) and no scan follows dsm16          */
  int              bw_bits;        /* radix of btab_lo / btab_hi: FD_ED25519_BTABW_BITS or
                                      FD_ED25519_BTABC_BITS (compact)                 */
  int              hs_host;        /* small == 3 only: the scalars came from the calling
                                      thread (host/fd_ed25519_hip_hsrec.cc): prep16 runs
                                      its decode blocks only, and dsm16's sflag / hs /
                                      hflag point at the caller's page-locked block (the
                                      same [field][cap] layout); never a full-length item */
  int32_t const *  btabq[8];       /* dsm16s<S>: compact [0..2^16)[2^(CB q)]B, q < S (shared per device) */
  uint32_t const * go;             /* dsm16 with host scalars and points: NULL, or a
                                      page-locked word the kernel waits on before it
                                      reads anything else -- the launch goes ahead of
                                      the host's work, so its dispatch overlaps it.
                                      FD_ED25519_GO_RUN: proceed; FD_ED25519_GO_CANCEL:
                                      exit writing nothing (the launch takes another
                                      path); unset after FD_ED25519_GO_SPIN_MAX polls
                                      (>= 0.1 s): exit writing nothing, which the host
                                      reports as a launch that ended without a code */
} fd_ed25519_verify_params_t;

/* host-decoded launches (params.pts in host memory): every host array's
   stride (params.cap), the launch's signatures being at most this many */
#define FD_ED25519_HS_STRIDE   8UL
#define FD_ED25519_GO_RUN      1U
#define FD_ED25519_GO_CANCEL   2U
#define FD_ED25519_GO_SPIN_MAX 200000U

/* 0: prep16 leaves the full-length items to a flag scan after dsm16 (A/B
   build) */
#ifndef FD_ED25519_FULL_IN_PREP
#define FD_ED25519_FULL_IN_PREP 1
#endif

/* All launchers are asynchronous on `stream` (a hipStream_t) and return a
   hipError_t value (0 on success). */
int fd_ed25519_hip_launch_gen_btab( int32_t * d_btab, void * stream );
int fd_ed25519_hip_launch_gen_btab16( int32_t * d_btab16, int base_doublings, void * stream );
/* [0..2^bits)[2^base_doublings]B into d_tab (bits FD_ED25519_BTABW_BITS or
   FD_ED25519_BTABC_BITS); d_scratch holds 2^bits*10 + 40 int32 */
int fd_ed25519_hip_launch_gen_btabw( int32_t * d_tab, int base_doublings, int bits, int32_t * d_scratch, void * stream );
/* counts into *d_bad the entries e < entries-1 of a 32-int-stride base
   table with entry e+1 != entry e + entry 1 (and entry 0 not the identity) */
int fd_ed25519_hip_launch_check_btabw( int32_t const * d_tab, int entries, uint32_t * d_bad, void * stream );
/* Enqueues hash, decode and dsm for one chunk; `grid` caps the persistent
   dsm grid (its atab scratch must hold grid*VERIFY_BLOCK/64 waves). */
int fd_ed25519_hip_launch_verify( fd_ed25519_verify_params_t const * p, uint32_t grid, void * stream );

/* The same, one phase at a time (so the host can bracket each with events). */
#define FD_ED25519_PHASE_HASH   0
#define FD_ED25519_PHASE_SCALAR 1
#define FD_ED25519_PHASE_DECODE 2
#define FD_ED25519_PHASE_DSM    3
#define FD_ED25519_PHASE_CNT    4
int fd_ed25519_hip_launch_phase( fd_ed25519_verify_params_t const * p, int phase, uint32_t grid, void * stream );
/* dsm16s (fd_ed25519_kernels.hip): the four- or eight-wave form for
   launches whose points and split scalars all came from the host */
int fd_ed25519_hip_launch_dsm16s( fd_ed25519_verify_params_t const * p, int waves, void * stream );

/* Host scalars (host/fd_ed25519_hip_hs.c, hsrec.cc, hsdec.cc): a launch of
   a few signatures whose k, S < L and half-size pair the calling thread
   computes while the device decompresses A and R -- or, for the fewest,
   whose A and R the calling thread decompresses too, dsm16 launched ahead
   of that work and waiting on the go word (params.go).
   hsrec: 1 and the 32-word record (k[8], hs[19], sflag, hflag), or 0 when
   k has no half-size pair within dbits (the launch then takes the device's
   own path).  hsdec_n writes each point's 20 limbs and flags as the decode
   blocks would.
   The split forms (dsm16s<S>, S = 4 or 8 waves) for host-decoded
   launches: hssplit turns one signature's record into the split scalars
   and s' chunks (hq: 24 rows of stride cap, layout at the function), and
   hsdec3_n also returns each point doubled step, 2 step, .. nx step times
   (S = 4: nx 1, step 66; S = 8: nx 3, step 33) in extended coordinates
   (40 limbs) for pts rows 2i + side of 40 limbs (row 0 A, 1 R -- affine,
   the first 20 -- 2 A_1, 3 R_1, ..); want_dsms makes (or finds) the
   engine's tables for that form. */
struct fd_ed25519_hip_engine;
int fd_ed25519_hip_private_hsrec( unsigned char const sig[ 64 ], unsigned char const pub[ 32 ],
                                  unsigned char const * msg, unsigned long msg_sz, int dbits, uint32_t rec[ 32 ] );
int fd_ed25519_hip_private_half_dbits( struct fd_ed25519_hip_engine const * e );
int fd_ed25519_hip_private_codes_portable( struct fd_ed25519_hip_engine const * e );
void fd_ed25519_hip_private_hsdec_n( unsigned char const * const * enc, unsigned long n, int avx_rule, int32_t * pt,
                                     unsigned char * flags );
void fd_ed25519_hip_private_hssplit( uint32_t const rec[ 32 ], int waves, uint32_t * hq, unsigned long cap,
                                     unsigned long j );
void fd_ed25519_hip_private_hsdec3_n( unsigned char const * const * enc, unsigned long n, int avx_rule, int32_t * pt,
                                      int32_t * ptx, int nx, int step, unsigned char * flags );
int fd_ed25519_hip_private_want_dsms( struct fd_ed25519_hip_engine * e, int waves );

/* The host-scalar block (host/fd_ed25519_hip_hs.c): what the calling thread
   writes and dsm16 / dsm16s read in place, every array [row][stride] (signature
   j of the launch at column j) and starting 16-byte aligned in a 16-byte
   aligned block:
     sflag [stride]         u8   S < L
     hflag [stride]         u8   bit0 d < 0
     hs    [24][stride]     u32  dsm16: rows 0..18, hsrec's rec[8..26];
                                 dsm16s: 24 rows, hssplit's
     pts   [8][40][stride]  i32  dsm16: rows of 20 limbs (A, R: x, y);
                                 dsm16s: rows of 40 limbs (A, R, A_1, R_1, ..)
     pflag [2][stride]      u8   A, R: hsdec3_n's flags
     go    16 bytes              word 0: params.go
   pts, pflag and go exist only in a host-decoded block, whose stride is
   FD_ED25519_HS_STRIDE; a block whose points the device decodes has the
   work arrays' stride (the engine's max_chunk) and ends after hs row 18
   (the split forms are host-decoded). */
#define FD_ED25519_HS_ALIGN16( x ) ( ( (x) + 15UL ) & ~15UL )
#define FD_ED25519_HS_O_SFLAG( s ) 0UL
#define FD_ED25519_HS_O_HFLAG( s ) FD_ED25519_HS_ALIGN16( s )
#define FD_ED25519_HS_O_HS( s )    ( 2UL*FD_ED25519_HS_ALIGN16( s ) )
#define FD_ED25519_HS_O_PTS( s )   ( FD_ED25519_HS_O_HS( s ) + 24UL*4UL*(s) )
#define FD_ED25519_HS_O_PFLAG( s ) ( FD_ED25519_HS_O_PTS( s ) + 8UL*40UL*4UL*(s) )
#define FD_ED25519_HS_O_GO( s )    FD_ED25519_HS_ALIGN16( FD_ED25519_HS_O_PFLAG( s ) + 2UL*(s) )
/* host-decoded launches have at most this many signatures (hs_points'
   arrays; the drop-in's and the pipe's setters clamp to it) */
#define FD_ED25519_HS_DECODE_MAX 4UL

/* One host-scalar launch.  hs_init describes the block and the launch
   (host only: nothing of the GPU is touched, so the fill steps also run on
   ordinary memory); hs_begin attaches the device side and launches; the
   caller then walks its own inputs with hs_scalars (and hands hs_points
   the encodings); hs_end, exactly once after a hs_begin that returned 0,
   finishes the launch. */
typedef struct {
  unsigned char * host;     /* the block, where the calling thread writes it */
  unsigned long   stride;
  int             decode;   /* the calling thread decodes A and R (pts, pflag, go) */
  unsigned long   n;        /* signatures, columns 0..n-1 */
  int             split;    /* 0: dsm16; 4, 8: dsm16s<split> (decode only) */
  int             avx_rule; /* hsdec3_n's: the engine has no FD_ED25519_HIP_FLAG_CODES_PORTABLE */
  /* set by hs_begin: the block, the signatures, the keys and the codes as
     the device sees them, and where the launches go */
  struct fd_ed25519_hip_engine * eng;
  unsigned char const * dev;
  unsigned char const * sigs;
  unsigned char const * pubs;
  signed char *         out;
  void *                stream;
} fd_ed25519_hip_hs_t;
/* a descriptor fits in this many bytes (tests hold one in a plain buffer) */
#define FD_ED25519_HS_DESC_MAX 128

/* bytes of a block of that stride */
unsigned long fd_ed25519_hip_private_hs_bytes( unsigned long stride, int decode );
void fd_ed25519_hip_private_hs_init( fd_ed25519_hip_hs_t * b, void * host, unsigned long stride, int decode,
                                     unsigned long n, int split, int avx_rule );
/* host-decoded: zeroes the go word, then launches dsm16 (or dsm16s<split>)
   waiting on it, ahead of the caller's arithmetic; else launches prep16's
   decode blocks.  Not 0 (a FD_ED25519_HIP_ERR_*): nothing was launched and
   no hs_end follows. */
int fd_ed25519_hip_private_hs_begin( fd_ed25519_hip_hs_t * b, struct fd_ed25519_hip_engine * e,
                                     unsigned char const * dev, unsigned char const * sigs,
                                     unsigned char const * pubs, signed char * out, void * stream );
/* signature j's scalars and flags into the block.  0: k has no half-size
   pair within dbits, nothing was written and the launch ends with
   hs_end( b, 0 ) */
int fd_ed25519_hip_private_hs_scalars( fd_ed25519_hip_hs_t * b, unsigned long j, unsigned char const sig[ 64 ],
                                       unsigned char const pub[ 32 ], unsigned char const * msg, unsigned long msg_sz,
                                       int dbits );
/* host-decoded only: enc[2j] signature j's A, enc[2j+1] its R (2n
   encodings); the points (doubled too, for a split form) and their flags
   into the block */
void fd_ed25519_hip_private_hs_points( fd_ed25519_hip_hs_t * b, unsigned char const * const * enc );
/* host-decoded: the release store of FD_ED25519_GO_RUN (run not 0) or
   FD_ED25519_GO_CANCEL, after every write of the block; else dsm16's
   launch when run is not 0, nothing when it is 0 */
int fd_ed25519_hip_private_hs_end( fd_ed25519_hip_hs_t * b, int run );
/* the engine's side of hs_begin / hs_end (host/fd_ed25519_hip_engine.c):
   prep16's decode blocks (dsm 0), or dsm16 / dsm16s<b->split> reading b's
   block in place (a host-decoded one: waiting on its go word).  The
   engine's dsm16 form must take n (n <= its r16 bound). */
int fd_ed25519_hip_private_hs_launch( fd_ed25519_hip_hs_t const * b, int dsm );
/* fd_ed25519_verify_batch_single_msg's rule on the host, for a
   transaction's codes[first .. first+cnt) (the device's is
   fd_ed25519_hip_launch_txn_combine below): cnt==0 or cnt>16 ERR_SIG; else
   the first error other than ERR_MSG in signature order, else ERR_MSG if
   any signature had it, else SUCCESS */
int fd_ed25519_hip_private_hs_combine( signed char const * codes, unsigned long first, unsigned long cnt );
int fd_ed25519_hip_verify_occupancy( int * blocks_per_cu );
/* lane-table bytes per dsm wave as compiled into the kernels (the host
   sizes the atab scratch from this, never from its own copy of the macro) */
unsigned long fd_ed25519_hip_atab_bytes_per_wave( void );

/* Per-transaction combine with fd_ed25519_verify_batch_single_msg's
   priority (src/ballet/ed25519/fd_ed25519_user.c:231-309): the first
   phase-1 error (ERR_SIG/ERR_PUBKEY) in signature order wins, else ERR_MSG
   if any equation fails, else SUCCESS; cnt==0 or cnt>16 -> ERR_SIG. */
int fd_ed25519_hip_launch_txn_combine( int8_t const * d_sig_codes, uint32_t const * d_txn_first,
                                       uint32_t const * d_txn_cnt, int8_t * d_txn_out, uint64_t ntxn,
                                       void * stream );

/* diagnostic: fd_half_scalars on the device, 12 words out per k (see
   fd_ed25519_hip_diag_half_scalars) */
int fd_ed25519_hip_launch_diag_half( uint32_t const * d_k, uint32_t * d_out, uint64_t n, int dbits, void * stream );

/* diagnostic (tests/test_gpu_dsm_diag.py): the product's own dsm kernels on
   work arrays the caller wrote, every array [row][n] (stride cap = n) in
   host memory, copied to device temporaries and launched as the dsm phase
   alone -- no hash, no scalar search, no decode.  form: */
#define FD_ED25519_DIAG_DSM_WIDE   0   /* dsm_kernel (small 0): fix_list / fix_cnt from hflag, work_ctr 0  */
#define FD_ED25519_DIAG_DSM_QUAD   1   /* dsm4, then dsm_kernel's scan for the full-length items          */
#define FD_ED25519_DIAG_DSM_OCT    2   /* dsm8, then the scan                                             */
#define FD_ED25519_DIAG_DSM_R16    3   /* dsm16 (full_in_prep 0, hs_host 0), then the scan                */
#define FD_ED25519_DIAG_DSM_SPLIT4 4   /* dsm16s<4> */
#define FD_ED25519_DIAG_DSM_SPLIT8 8   /* dsm16s<8> */
/*   sflag [n], hflag [n], pflag [2][n] as in fd_ed25519_verify_params_t;
     forms 0..3: pts [2][20][n], hs [19][n], and for the full-length items
       (hflag bit 1) k [8][n] and S [n][64] (R||S, only S read); k and S
       may be NULL when hflag marks none;
     split forms: pts [S][40][n] and hs [24][n] as hsdec3_n / hssplit write
       them, no full-length item, k and S unused.
   params.go stays NULL.  out [n]: the codes (a signature no kernel wrote a
   code for keeps FD_ED25519_DIAG_DSM_UNWRITTEN).
   diag_dsm_check is the whole validation, host only (no engine, no GPU);
   diag_dsm launches nothing it refuses (FD_ED25519_HIP_ERR_INVAL): flags
   outside their bits; n == 0 or above n_max (diag_dsm passes what the
   engine's form limits and lane tables admit); forms 0..3, half-size
   items: c >= 2^FD_HALF_BITS, |d| >= 2^half_dbits, s_lo >= 2^144, s_lo +
   2^144 s_hi >= 2^253; full-length items: k >= 2^253, S >= L with sflag
   set (recode_radix65536's S < L); split forms: a split scalar so long
   that 160 - 4 W - SH0 < 8 (S = 4: 88 bits or more, S = 8: 56 or more), a
   chunk of s' >= 2^CB, a full-length flag; affine point limbs outside
   what a decode leaves (x: |limb| <= 1.01 units of 2^25 / 2^24, tight; y:
   above that or at 2^26 / 2^25, fe_frombytes's), extended point limbs
   (split forms, rows >= 2) not tight (table16_build_p3's). */
#define FD_ED25519_DIAG_DSM_UNWRITTEN 0x55
int fd_ed25519_hip_private_diag_dsm_check( int form, unsigned long n, unsigned long n_max, int half_dbits,
                                           unsigned char const * sflag, unsigned char const * hflag,
                                           unsigned char const * pflag, int32_t const * pts, uint32_t const * hs,
                                           uint32_t const * k, unsigned char const * S );
/* what n_max diag_dsm passes for this engine and form (0: the form is not available) */
unsigned long fd_ed25519_hip_private_diag_dsm_nmax( struct fd_ed25519_hip_engine * e, int form );
int fd_ed25519_hip_private_diag_dsm( struct fd_ed25519_hip_engine * e, int form, unsigned long n,
                                     unsigned char const * sflag, unsigned char const * hflag,
                                     unsigned char const * pflag, int32_t const * pts, uint32_t const * hs,
                                     uint32_t const * k, unsigned char const * S, signed char * out );

/* diagnostic (tests/test_gpu_prep_diag.py), the mirror of diag_dsm: the
   product's own hash, scalar and decode phases -- and nothing after them --
   on host inputs, the work arrays they wrote copied back.  form: */
#define FD_ED25519_DIAG_PREP_WIDE       0   /* small 0: the sort trio (hashed only), hash, scalar and decode kernels */
#define FD_ED25519_DIAG_PREP_FUSED1     1   /* small 1: prep_kernel                                               */
#define FD_ED25519_DIAG_PREP_FUSED2     2   /* small 2: prep_kernel                                               */
#define FD_ED25519_DIAG_PREP_R16        3   /* small 3, full_in_prep 0: prep16's hash and decode blocks           */
#define FD_ED25519_DIAG_PREP_R16_DECODE 4   /* small 3, hs_host 1: prep16's decode blocks only                    */
#define FD_ED25519_DIAG_PREP_R16_FULL   5   /* small 3, full_in_prep 1: the full-length items' codes in out too    */
/*   in: sigs [n][64], pubs [n][32] and either msgs / msg_off [n] / msg_sz
       [n] (digests NULL: hashed here, perm the sort's in the wide form) or
       digests [n][64] (msgs unused, perm NULL as the engine sets it); n
       signatures in arrays of stride cap >= n;
     out: k [8][cap], sflag [cap], hflag [cap], pflag [2][cap], pts
       [2][20][cap], hs [19][cap], perm [cap], out [cap] and fix [2 + cap]
       (fix_cnt, work_ctr, fix_list).
   Every device temporary behind them is filled with
   FD_ED25519_DIAG_DSM_UNWRITTEN bytes before the launch, so what no kernel
   wrote comes back as the pattern -- a row that should have been written,
   or one at an index >= n.
   hash_kernel takes perm's entries as indices, so in the wide hashed form
   the hash phase first runs over a perm of zeros and the sort's result is
   held to be a permutation of 0 .. n-1 (FD_ED25519_HIP_ERR_INVAL if not,
   nothing further launched) before the launch proper on the refilled
   temporaries.
   diag_prep_check is the whole validation, host only (no engine, no GPU);
   diag_prep launches nothing it refuses (FD_ED25519_HIP_ERR_INVAL): a form
   outside 0..5, n == 0 or above n_max (diag_prep passes diag_prep_nmax: what
   the engine's form limits admit, and for R16_FULL a lane-table slot per
   signature), cap < n, sigs / pubs / digests NULL or not 16-byte aligned (the
   rule of fd_ed25519_hip_verify_dev), no digests and no msg_off / msg_sz (or
   no msgs with a message that has bytes), a msg_sz above
   FD_ED25519_HIP_MSG_SZ_MAX. */
int fd_ed25519_hip_private_diag_prep_check( int form, unsigned long n, unsigned long n_max, unsigned long cap,
                                            unsigned char const * sigs, unsigned char const * pubs,
                                            unsigned char const * msgs, unsigned long const * msg_off,
                                            unsigned int const * msg_sz, unsigned char const * digests );
/* what n_max diag_prep passes for this engine and form (0: the form is not available) */
unsigned long fd_ed25519_hip_private_diag_prep_nmax( struct fd_ed25519_hip_engine * e, int form );
int fd_ed25519_hip_private_diag_prep( struct fd_ed25519_hip_engine * e, int form, unsigned long n, unsigned long cap,
                                      unsigned char const * sigs, unsigned char const * pubs,
                                      unsigned char const * msgs, unsigned long const * msg_off,
                                      unsigned int const * msg_sz, unsigned char const * digests,
                                      uint32_t * k, unsigned char * sflag, unsigned char * hflag, unsigned char * pflag,
                                      int32_t * pts, uint32_t * hs, uint32_t * perm, signed char * out, uint32_t * fix );

/* diagnostic (tests/test_gpu_sign_diag.py): the engine's [0..128]B table of
   36-int entries (y+x, y-x, 2dxy, six zeros), copied back on the engine's
   stream.  fd_ed25519_sign_kernel alone reads this table (the verify
   kernels take btab16 and btabw), so check_base_tables and base_entry do
   not see it; the test holds it against the curve and hands it to
   libfd_ed25519_diag.so's sign family. */
int fd_ed25519_hip_private_sign_table( struct fd_ed25519_hip_engine * e, int out[ FD_ED25519_BTAB_INTS ] );

/* The device hashes take a message's remaining byte count as a signed
   32-bit value (fd_sha512_dev.h sha_msg_dword: (int)sz - p), so a message
   the device hashes is at most FD_ED25519_HIP_MSG_SZ_MAX (2^31 - 1) bytes.
   FD_ED25519_HIP_ERR_INVAL when one of msg_sz[0..n) is larger, else 0; host
   only (no engine, no GPU, no allocation): what the host-buffer entry
   points run before they stage anything (tests/test_hash_diag_selfcheck.py). */
int fd_ed25519_hip_private_msg_sz_check( unsigned int const * msg_sz, unsigned long n );

/* ---- raw transactions (fd_ed25519_txn.hip) ---- */

/* per-transaction code for a payload fd_txn_parse rejects (never an
   ed25519 code) */
#define FD_ED25519_TXN_PARSE_FAILED_CODE (-4)

typedef struct {
  uint8_t const *  payloads;   /* payload bytes, readable 16 B past each   */
  uint64_t const * pay_off;    /* [ntxn]                                   */
  uint32_t const * pay_sz;     /* [ntxn]                                   */
  uint32_t const * txn_first;  /* [ntxn] first signature slot               */
  uint32_t const * txn_cnt;    /* [ntxn] payload byte 0 (slots: 1..16 -> cnt, else 0) */
  uint64_t         ntxn;
  uint8_t *        sigs;       /* [slots][64] out, 16-B aligned            */
  uint8_t *        pubs;       /* [slots][32] out                          */
  uint64_t *       msg_off;    /* [slots] out: into payloads                */
  uint32_t *       msg_sz;     /* [slots] out                               */
  uint8_t *        parse_ok;   /* [ntxn] out                                */
  uint8_t *        trailer;    /* [ntxn][64] out (optional): fd_txn_t bytes  */
} fd_ed25519_txn_stage_params_t;

int fd_ed25519_hip_launch_txn_stage( fd_ed25519_txn_stage_params_t const * p, void * stream );

/* H2D without the copy engines: one launch in which the device reads up to
   FD_ED25519_PULL_SPAN_MAX spans of page-locked host memory (device-visible
   addresses, 16-byte aligned) and writes them to device memory (16-byte
   aligned), exactly n bytes each.  A launch is asynchronous; a
   hipMemcpyAsync H2D issued by a thread whose stream shares the device with
   busy compute streams can hold the calling thread for the copy's
   duration (measured in the verify service: tools/ubench/h2d_call_probe.hip,
   DESIGN.md 3c). */
#define FD_ED25519_PULL_SPAN_MAX 8
typedef struct {
  uint8_t const * src[ FD_ED25519_PULL_SPAN_MAX ];
  uint8_t *       dst[ FD_ED25519_PULL_SPAN_MAX ];
  uint64_t        n  [ FD_ED25519_PULL_SPAN_MAX ];
  uint32_t        cnt;
} fd_ed25519_pull_params_t;

int fd_ed25519_hip_launch_pull( fd_ed25519_pull_params_t const * p, void * stream );

/* fault-injection build only (-DFD_ED25519_HALF_FAULT=1): one wave that
   sleeps for ms milliseconds (at most 10 s) of the device's wall clock */
int fd_ed25519_hip_launch_stall( unsigned ms, void * stream );
int fd_ed25519_hip_launch_txn_finish( int8_t const * d_sig_codes, uint32_t const * d_txn_first,
                                      uint32_t const * d_txn_cnt, uint8_t const * d_parse_ok, int8_t * d_txn_out,
                                      uint64_t ntxn, void * stream );

/* ---- Ed25519 precompile instructions (fd_ed25519_txn.hip) ---- */

/* stage: one lane per transaction parses the payload, walks its Ed25519
   precompile instructions (fd_precompile_core.h) and fills the slots
   [ent_first[t], ent_first[t+1]) -- never one outside them */
typedef struct {
  uint8_t const *  payloads;   /* payload bytes, readable 16 B past each    */
  uint64_t const * pay_off;    /* [ntxn]                                    */
  uint32_t const * pay_sz;     /* [ntxn]                                    */
  uint32_t const * ent_first;  /* [ntxn+1] the caller's reservation          */
  uint64_t         ntxn;
  uint64_t         n_ent;      /* slots in all                               */
  uint8_t *        sigs;       /* [n_ent][64] out, 16-B aligned              */
  uint8_t *        pubs;       /* [n_ent][32] out, 16-B aligned              */
  uint64_t *       msg_off;    /* [n_ent] out: into payloads                  */
  uint32_t *       msg_sz;     /* [n_ent] out                                 */
  int8_t *         pre;        /* [n_ent] out: 0, DATA_OFFSET, or the transaction's status */
  uint8_t *        ent_instr;  /* [n_ent] out: the listing instruction's index */
  int8_t *         status;     /* [ntxn] out: 0, PARSE_FAILED, BAD_RESERVATION */
  uint8_t *        hdr_instr;  /* [ntxn] out: first instruction whose header fails (0xFF: none) */
  uint8_t *        hdr_pos;    /* [ntxn] out: entries ahead of it             */
} fd_ed25519_precompile_stage_params_t;

typedef struct {
  int8_t const *   codes;      /* [n_ent] the verify phases' codes           */
  int8_t const *   pre;
  uint8_t const *  ent_instr;
  int8_t const *   status;
  uint8_t const *  hdr_instr;
  uint8_t const *  hdr_pos;
  uint32_t const * ent_first;
  uint64_t         ntxn;
  uint64_t         n_ent;
  int8_t *         txn_out;    /* [ntxn]                                     */
  uint8_t *        instr_out;  /* [ntxn]                                     */
  int8_t *         ent_out;    /* [n_ent] or NULL                            */
} fd_ed25519_precompile_finish_params_t;

int fd_ed25519_hip_launch_precompile_stage( fd_ed25519_precompile_stage_params_t const * p, void * stream );
int fd_ed25519_hip_launch_precompile_finish( fd_ed25519_precompile_finish_params_t const * p, void * stream );

/* ---- leader signatures of Merkle shreds (fd_ed25519_shred.hip) ---- */

/* stage: one lane per shred applies fd_shred_core.h's rules, derives the
   root and fills slot i of the verify SoA -- a dummy (zero signature,
   msg_sz 0, zero root) for a shred that is not judged */
typedef struct {
  uint8_t const *  shreds;     /* shred bytes, readable 16 B past each      */
  uint64_t const * shred_off;  /* [n]                                       */
  uint32_t const * shred_sz;   /* [n]                                       */
  uint64_t         n;
  uint8_t *        sigs;       /* [n][64] out, 16-B aligned                 */
  uint8_t *        roots;      /* [n][32] out, 16-B aligned: the messages   */
  uint64_t *       msg_off;    /* [n] out: 32 i, into roots                 */
  uint32_t *       msg_sz;     /* [n] out: 32, or 0                         */
  int8_t *         pre;        /* [n] out: 0, ERR_PARSE, UNSUPPORTED, ERR_HEADER */
} fd_ed25519_shred_stage_params_t;

typedef struct {
  int8_t const *   codes;      /* [n] the verify phases' codes              */
  int8_t const *   pre;
  uint8_t const *  roots;
  uint64_t         n;
  int8_t *         out;        /* [n]                                       */
  uint8_t *        roots_out;  /* [n][32] 16-B aligned, or NULL             */
  int8_t *         sig_out;    /* [n] or NULL                               */
} fd_ed25519_shred_finish_params_t;

int fd_ed25519_hip_launch_shred_stage( fd_ed25519_shred_stage_params_t const * p, void * stream );
int fd_ed25519_hip_launch_shred_finish( fd_ed25519_shred_finish_params_t const * p, void * stream );

/* ---- signed gossip and repair control packets (fd_ed25519_packet.hip) ---- */

/* stage: one lane per packet applies fd_packet_core.h's rules and fills slot
   i of the verify SoA -- signature, key, and the message in the mirror of
   the packet buffer; a dummy (zero signature and key, msg_sz 0) for a packet
   that is not judged */
typedef struct {
  uint8_t const *  pkts;       /* 16-B aligned, readable 16 B past pkt_bytes */
  uint64_t const * pkt_off;    /* [n]                                        */
  uint32_t const * pkt_sz;     /* [n]                                        */
  uint64_t         n;
  uint64_t         pkt_bytes;
  uint32_t         self_key[ 8 ];  /* the own identity, by value             */
  int32_t          proto;
  uint8_t *        sigs;       /* [n][64] out, 16-B aligned                  */
  uint8_t *        pubs;       /* [n][32] out, 16-B aligned                  */
  uint8_t *        msgs;       /* mirror of pkts out, 16-B aligned           */
  uint64_t *       msg_off;    /* [n] out, into msgs                         */
  uint32_t *       msg_sz;     /* [n] out                                    */
  int8_t *         pre;        /* [n] out: 0, ERR_PARSE, UNSUPPORTED, NOT_FOR_SELF */
} fd_ed25519_packet_stage_params_t;

typedef struct {
  int8_t const *   codes;      /* [n] the verify phases' codes               */
  int8_t const *   pre;
  uint64_t         n;
  int8_t *         out;        /* [n]                                        */
  int8_t *         sig_out;    /* [n] or NULL                                */
} fd_ed25519_packet_finish_params_t;

int fd_ed25519_hip_launch_packet_stage( fd_ed25519_packet_stage_params_t const * p, void * stream );
int fd_ed25519_hip_launch_packet_finish( fd_ed25519_packet_finish_params_t const * p, void * stream );

/* ---- CRDS values of gossip pull responses and push messages (fd_ed25519_crds.hip) ---- */

/* stage: one lane per packet walks it by fd_crds_core.h's rules and fills
   the slots [val_first[i], val_first[i+1]) -- never one outside them --
   with each value's signature and key, its message left in place in the
   packet buffer; a dummy (zero signature and key, msg_sz 0) for a value
   under the own identity and for every slot of a packet without verdicts */
typedef struct {
  uint8_t const *  pkts;       /* 4-B aligned, readable 16 B past pkt_bytes  */
  uint64_t const * pkt_off;    /* [n]                                        */
  uint32_t const * pkt_sz;     /* [n]                                        */
  uint32_t const * val_first;  /* [n+1] the caller's reservation             */
  uint64_t         n;
  uint64_t         n_val;
  uint64_t         pkt_bytes;
  uint32_t         self_key[ 8 ];  /* the own identity, by value             */
  uint8_t *        sigs;       /* [n_val][64] out, 16-B aligned              */
  uint8_t *        pubs;       /* [n_val][32] out, 16-B aligned              */
  uint64_t *       msg_off;    /* [n_val] out, into pkts                     */
  uint32_t *       msg_sz;     /* [n_val] out                                */
  uint32_t *       val_sz;     /* [n_val] out: the data's size; 0: no hash   */
  int8_t *         pre;        /* [n_val] out: 0, OWN, or the packet's code  */
  int8_t *         status;     /* [n] out: 0, ERR_PARSE, UNSUPPORTED, BAD_RESERVATION */
} fd_ed25519_crds_stage_params_t;

/* finish: lane k < n_val the value's verdict, lane i < n the packet's code */
typedef struct {
  int8_t const *   codes;      /* [n_val] the verify phases' codes           */
  int8_t const *   pre;
  int8_t const *   status;
  uint64_t         n;
  uint64_t         n_val;
  int8_t *         pkt_out;    /* [n]                                        */
  int8_t *         val_out;    /* [n_val]                                    */
  int8_t *         sig_out;    /* [n_val] or NULL                            */
} fd_ed25519_crds_finish_params_t;

/* hash: one lane per value, SHA-256 of pkts[msg_off-64 .. msg_off+val_sz) */
typedef struct {
  uint8_t const *  pkts;
  uint64_t const * msg_off;
  uint32_t const * val_sz;
  uint64_t         n_val;
  uint8_t *        hash_out;   /* [n_val][32], 4-B aligned                   */
} fd_ed25519_crds_hash_params_t;

int fd_ed25519_hip_launch_crds_stage( fd_ed25519_crds_stage_params_t const * p, void * stream );
int fd_ed25519_hip_launch_crds_finish( fd_ed25519_crds_finish_params_t const * p, void * stream );
int fd_ed25519_hip_launch_crds_hash( fd_ed25519_crds_hash_params_t const * p, void * stream );

/* ---- sealing a leader's FEC sets (fd_ed25519_fec.hip) ---- */

/* tree: workgroup k applies fd_fec_core.h's rules to the shreds
   [set_first[k], set_first[k+1]), builds their Merkle tree, writes every
   shred's proof and leaves the root as message k of the sign kernel -- an
   empty message and a zero root for a set with a code, whose shreds it does
   not write */
typedef struct {
  uint8_t *        shreds;     /* shred bytes, readable 16 B past each      */
  uint64_t const * shred_off;  /* [n]                                       */
  uint32_t const * shred_sz;   /* [n]                                       */
  uint64_t         n;
  uint32_t const * set_first;  /* [n_set+1]                                 */
  uint64_t         n_set;
  uint8_t *        roots;      /* [n_set][32] out, 16-B aligned: the messages */
  uint64_t *       msg_off;    /* [n_set] out: 32 k, into roots             */
  uint32_t *       msg_sz;     /* [n_set] out: 32, or 0                     */
  uint32_t *       set_of;     /* [n] preset to ~0; out: k for a sealed set's shreds */
  int8_t *         set_out;    /* [n_set] out: 0, ERR_PARSE, UNSUPPORTED, ERR_SET */
  uint8_t *        roots_out;  /* [n_set][32] 16-B aligned, or NULL         */
} fd_ed25519_fec_tree_params_t;

/* scatter: lane i < n copies signature set_of[i] into shred i; lane k <
   n_set the caller's copy of signature k */
typedef struct {
  uint8_t *        shreds;
  uint64_t const * shred_off;
  uint64_t         n;
  uint64_t         n_set;
  uint32_t const * set_of;
  uint8_t const *  sigs;       /* [n_set][64] the sign kernel's             */
  int8_t const *   set_out;
  uint8_t *        sigs_out;   /* [n_set][64] 16-B aligned, or NULL         */
} fd_ed25519_fec_scatter_params_t;

int fd_ed25519_hip_launch_fec_tree( fd_ed25519_fec_tree_params_t const * p, void * stream );
int fd_ed25519_hip_launch_fec_scatter( fd_ed25519_fec_scatter_params_t const * p, void * stream );
/* the tree kernel's workgroup size as built (tools/fec_bench.py reports it) */
unsigned fd_ed25519_hip_private_fec_tree_block( void );

/* ---- the Reed-Solomon parity of a leader's FEC sets (fd_ed25519_reedsol.hip) ---- */

/* parity: workgroup k applies fd_fec_core.h's and fd_reedsol_core.h's rules
   to the shreds [set_first[k], set_first[k+1]) and, when they pass, writes
   bytes [0x59, 0x59 + P) of the set's code shreds and nothing else */
typedef struct {
  uint8_t *        shreds;     /* shred bytes, readable 16 B past each      */
  uint64_t const * shred_off;  /* [n]                                       */
  uint32_t const * shred_sz;   /* [n]                                       */
  uint64_t         n;
  uint32_t const * set_first;  /* [n_set+1]                                 */
  uint64_t         n_set;
  uint8_t const *  tab;        /* fd_reedsol_core_tables's block, 16-B aligned */
  int8_t *         set_out;    /* [n_set] out: 0, ERR_PARSE, UNSUPPORTED, ERR_SET */
} fd_ed25519_fec_parity_params_t;

int fd_ed25519_hip_launch_fec_parity( fd_ed25519_fec_parity_params_t const * p, void * stream );

/* ---- recovering received FEC sets (fd_ed25519_recover.hip) ---- */

/* recover: workgroup k applies fd_fec_core.h's and fd_reedsol_core.h's rules
   9-11 to the slots [set_first[k], set_first[k+1]) and, when they pass,
   writes what rule 12 names of the set's erased slots and nothing else */
typedef struct {
  uint8_t *        shreds;     /* slot bytes, readable 16 B past each       */
  uint64_t const * shred_off;  /* [n]                                       */
  uint32_t const * shred_sz;   /* [n]                                       */
  uint8_t const *  erased;     /* [n] 0: received, else erased (not read)   */
  uint64_t         n;
  uint32_t const * set_first;  /* [n_set+1]                                 */
  uint64_t         n_set;
  uint8_t const *  tab;        /* fd_reedsol_core_tables's block, 16-B aligned */
  int8_t *         set_out;    /* [n_set] out: 0, ERR_PARSE, UNSUPPORTED, ERR_SET, ERR_PARTIAL, ERR_CORRUPT */
} fd_ed25519_fec_recover_params_t;

int fd_ed25519_hip_launch_fec_recover( fd_ed25519_fec_recover_params_t const * p, void * stream );

/* ---- shredding entry batches (fd_ed25519_shredder.hip) ---- */

/* front: workgroup q < set_cnt lays out set set0 + q of the call -- it finds
   the batch that reserved the set in set_first_b, applies fd_shredder_core.h's
   rules and writes the set's data shreds, parity headers, shred_off, shred_sz
   and set_first entry; the workgroups behind them judge the batches, a lane
   each, and close set_first.  The arrays of shreds and sets are the
   launch's own: entry 0 is shred shred0 and set set0 of the call, so that a
   host wrapper's pass (a range of the call's sets) is the same launch. */
typedef struct {
  uint8_t const *  buf;            /* batch bytes, readable 16 B past buf_sz    */
  uint64_t         buf_sz;
  uint64_t const * batch_off;      /* [nb]                                      */
  uint32_t const * batch_sz;       /* [nb]                                      */
  void const *     desc;           /* [nb] fd_shredder_core_desc_t, 8-B aligned */
  uint32_t const * set_first_b;    /* [nb+1] sets of the call                   */
  uint32_t const * shred_first_b;  /* [nb+1] shreds of the call                 */
  uint64_t         nb;
  uint64_t         n_set, n;       /* the call's sets and shreds                */
  uint64_t         set0, set_cnt;  /* the launch's sets                         */
  uint64_t         shred0, m;      /* the launch's shreds [shred0, shred0 + m)  */
  uint64_t         skip_b, skip;   /* batch_off[skip_b] is where byte skip of that batch stands (a pass that continues a batch) */
  uint8_t *        shreds;         /* shred i of the launch at shreds + base_off + stride i */
  uint64_t         base_off, stride;
  uint64_t *       shred_off;      /* [m] out                                   */
  uint32_t *       shred_sz;       /* [m] preset to 0; out                      */
  uint32_t *       set_first;      /* [set_cnt+1] out                           */
  int8_t *         batch_out;      /* [nb] out, or NULL                         */
  uint8_t const *  privs;          /* [nb][32] 16-B aligned, or NULL            */
  uint8_t *        keys;           /* [set_cnt][32] out, 16-B aligned, with privs */
} fd_ed25519_shredder_params_t;

int fd_ed25519_hip_launch_shredder( fd_ed25519_shredder_params_t const * p, void * stream );

/* ---- a block's proof-of-history hash chain (fd_ed25519_poh.hip) ---- */

/* One parameter block for the three launches (fd_poh_core.h's rules):
   leaf   lane j < n_sig: leaves[j] = SHA-256( 0x00 || sig j ), zeros for a
          signature that leaves the buffer
   tree   workgroup i < n: roots[i] = the root of leaves [sig_first[i],
          sig_first[i+1]), reduced in place; pre[i] = 1 if a signature of the
          range leaves the buffer, else 0; nothing but pre[i] = 0 for a range
          that is empty, runs backwards or leaves [0, n_sig)
   chain  lane i < n: the judge, the k compressions, the mixin with roots[i],
          the comparison; out[i] and, if asked for, out_hash[i]
   tools/poh_bench.py mirrors this struct field for field (its Params): change both together. */
typedef struct {
  uint8_t const *  buf;        /* readable 16 B past buf_sz                 */
  uint64_t         buf_sz;
  uint64_t const * hdr_off;    /* [n]                                       */
  uint64_t const * in_off;     /* [n]                                       */
  uint32_t const * sig_first;  /* [n+1]                                     */
  uint64_t const * sig_off;    /* [n_sig]                                   */
  uint64_t         n;
  uint64_t         n_sig;
  uint64_t         hash_cnt_max;
  uint32_t *       leaves;     /* work: [n_sig][8] big-endian hash words    */
  uint32_t *       roots;      /* work: [n][8]                              */
  int8_t *         pre;        /* work: [n]                                 */
  int8_t *         out;        /* [n] out: 0, POH_ERR_PARSE, POH_UNSUPPORTED, POH_ERR_HASH */
  uint8_t *        out_hash;   /* [n][32] out, or NULL; 16-byte aligned     */
} fd_ed25519_poh_params_t;

int fd_ed25519_hip_launch_poh_leaf ( fd_ed25519_poh_params_t const * p, void * stream );
int fd_ed25519_hip_launch_poh_tree ( fd_ed25519_poh_params_t const * p, void * stream );
int fd_ed25519_hip_launch_poh_chain( fd_ed25519_poh_params_t const * p, void * stream );
unsigned fd_ed25519_hip_private_poh_params_bytes( void );   /* sizeof(fd_ed25519_poh_params_t), for tools/poh_bench.py */

/* ---- generator (fd_ed25519_gen.hip) ---- */

typedef struct {
  uint8_t const *  msgs;
  uint64_t const * msg_off;
  uint32_t const * msg_sz;
  uint8_t const *  privs;      /* [n][32], 16-byte aligned; NULL: derive from (seed, index_base+i) */
  uint8_t *        sigs;       /* [n][64] out */
  uint8_t *        pubs;       /* [n][32] out */
  uint64_t         n;
  uint64_t         seed;
  uint64_t         index_base;
  int32_t const *  btab;
} fd_ed25519_sign_params_t;

typedef struct {
  uint8_t *        msgs;
  uint64_t const * msg_off;
  uint32_t const * msg_sz;
  uint8_t *        sigs;
  uint8_t *        pubs;
  uint64_t         n;
  uint64_t         seed;
  uint64_t         index_base;
  uint32_t         ppm;        /* corrupted fraction, parts per million */
  int8_t *         expect;     /* [n] out (optional): reference AVX-512 code */
  uint8_t *        cls;        /* [n] out (optional): class 0..7 */
} fd_ed25519_corrupt_params_t;

int fd_ed25519_hip_launch_fill_random( uint8_t * d, uint64_t nbytes, uint64_t seed, void * stream );
int fd_ed25519_hip_launch_sign( fd_ed25519_sign_params_t const * p, void * stream );
int fd_ed25519_hip_launch_corrupt( fd_ed25519_corrupt_params_t const * p, void * stream );

#ifdef __cplusplus
}
#endif
#endif
