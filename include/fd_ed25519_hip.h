#ifndef HEADER_fd_ed25519_hip_h
#define HEADER_fd_ed25519_hip_h

/* libfd_ed25519_hip -- MI355X (gfx950) ed25519 signature verification for
   Firedancer, as a C-ABI shared library.

   Part 1 is a drop-in for the reference's verify API
   (tigarcia/firedancer src/ballet/ed25519/fd_ed25519.h:96-138): the same
   symbols, prototypes, argument meaning and return codes, so a binary that
   links libfd_ed25519_hip ahead of libfd_ballet.a resolves them here.

   Part 2 is the batch engine the drop-ins sit on.  A synchronous per-call
   API cannot feed a GPU; callers that batch (the verify
   tile, bench.py) use the SoA entry points below, either with host buffers
   (staged through pinned memory) or with device-resident buffers (enqueued
   asynchronously on a HIP stream).

   Verdicts and error codes are bit-identical to fd_ed25519_verify of the
   reference's AVX-512 backend (the production build); an engine created with
   FD_ED25519_HIP_FLAG_CODES_PORTABLE reproduces the portable backend's codes
   instead (they differ only in the code returned for an undecodable public
   key). */

#ifdef __cplusplus
extern "C" {
#endif

/* Reference codes, src/ballet/ed25519/fd_ed25519.h:11-14 */
#define FD_ED25519_SUCCESS    ( 0)
#define FD_ED25519_ERR_SIG    (-1)
#define FD_ED25519_ERR_PUBKEY (-2)
#define FD_ED25519_ERR_MSG    (-3)

/* The reference's sha512 calculator (src/ballet/sha512/fd_sha512.h:15-16,
   56-77: 256 bytes, 128-byte aligned) is opaque here: the drop-ins accept
   the caller's handle and do not touch it (the hash runs on the GPU). */
#ifndef FD_SHA512_ALIGN
typedef struct fd_sha512_private fd_sha512_t;
#endif

/* ---- Part 1: drop-in verify API ------------------------------------- */

/* Replaces fd_ed25519_verify (src/ballet/ed25519/fd_ed25519.h:96-101,
   implementation src/ballet/ed25519/fd_ed25519_user.c:134-229).  msg may be
   NULL if msg_sz==0.  Returns FD_ED25519_SUCCESS or FD_ED25519_ERR_*.
   Synchronous; runs on the process-wide default engine (device from
   $FD_ED25519_HIP_DEVICE, default 0; codes from $FD_ED25519_HIP_CODES =
   "avx512" (default) | "portable").  A failed launch is retried once on a
   re-created engine; a device that fails again is lost, and the process's
   policy decides (fd_ed25519_hip_dropin_set_on_lost below: abort with a
   message, the default, or fail closed); this path never falls back to
   the CPU.  Any
   msg_sz is accepted, as by the reference (2 GiB and more: the message is
   hashed on the host, fd_ed25519_hip_dropin_set_host_hash_min). */
int
fd_ed25519_verify( unsigned char const   msg[],
                   unsigned long         msg_sz,
                   unsigned char const   sig[ 64 ],
                   unsigned char const   public_key[ 32 ],
                   fd_sha512_t *         sha );

/* Replaces fd_ed25519_verify_batch_single_msg (src/ballet/ed25519/fd_ed25519.h:124-130,
   implementation src/ballet/ed25519/fd_ed25519_user.c:231-309), with the
   reference's parameter spellings (array bounds included, so the two
   headers compile together: tests/test_abi.py): batch_sz
   signatures (64 B each, contiguous) by batch_sz public keys (32 B each,
   contiguous) over one message.  batch_sz==0 or >16 -> FD_ED25519_ERR_SIG.
   Otherwise the first phase-1 error (bad S, undecodable or small-order key
   or R) in signature order wins, then FD_ED25519_ERR_MSG if any equation
   fails. */
int
fd_ed25519_verify_batch_single_msg( unsigned char const   msg[],
                                    unsigned long const   msg_sz,
                                    unsigned char const   signatures[ 64 ], /* 64 * batch_sz */
                                    unsigned char const   pubkeys[ 32 ],    /* 32 * batch_sz */
                                    fd_sha512_t *         shas[ 1 ],        /* batch_sz      */
                                    unsigned char const   batch_sz );

/* Replaces fd_ed25519_strerror (src/ballet/ed25519/fd_ed25519_user.c:311-321). */
char const *
fd_ed25519_strerror( int err );

/* The drop-ins above serve any number of calling threads: concurrent calls
   are coalesced into shared launches on the process's four drop-in engines
   (compact tables, 16K-signature chunks).  dropin_stats reports the
   launches made and the calls they carried; dropin_device_bytes the device
   memory the drop-ins hold (their engines plus the compact tables; it
   creates them if no call has yet). */
void
fd_ed25519_hip_dropin_stats( unsigned long * launches, unsigned long * requests );

/* A message of 2 GiB or more is past what the device hash takes
   (FD_ED25519_HIP_MSG_SZ_MAX below): the drop-ins hash it (R_j || A_j || M per signature) on the
   calling thread with the library's SHA-512 and verify the rest on the GPU
   from the digests (fd_ed25519_hip_verify_digests_dev); no message is ever
   truncated or refused.  Test hook: messages of at least `bytes` bytes take
   that path (0 restores 2 GiB, and so does a limit above it). */
void
fd_ed25519_hip_dropin_set_host_hash_min( unsigned long bytes );

/* A direct drop-in launch (one caller alone, at most a few signatures)
   computes each signature's scalars -- k = SHA-512(R||A||M) mod L, S < L,
   the half-size pair -- on the calling thread while the GPU decompresses A
   and R, instead of in one GPU lane before them (the latency path's
   longest chain).  Test hook: launches of at most `max_sigs` signatures
   take that path (0: never; the default is 4). */
void
fd_ed25519_hip_dropin_set_host_scalars( unsigned long max_sigs );

/* Test hook: the bound on |d| the calling thread's search uses (0 restores
   the engine's, 151).  A signature whose k has no pair within it sends the
   launch down the device path from its digest, whose own search runs at
   the engine's bound -- the fallback a test reaches with k that have no
   pair at 131 bits. */
void
fd_ed25519_hip_dropin_set_host_scalars_dbits( int dbits );

/* The fewest-signature host-scalar launches also decompress A and R on the
   calling thread (a few us a point on one core, against ~44 us for the
   GPU's decode blocks, whose one 16-lane row per point is a chain of ~265
   dependent field operations) and launch only the group equation, which
   reads the points in place.  Test hook: launches of at most `max_sigs`
   signatures take that path (0: never; the default is 2; at most the host
   scalars' bound). */
void
fd_ed25519_hip_dropin_set_host_decode( unsigned long max_sigs );

/* Host-decoded drop-in launches run the group equation split over
   `waves` waves (4 or 8; 2: dsm16's two) -- the calling thread also
   doubles A and R every 66 (4) or 33 (8) bits and splits the half-size
   scalars there and s' into 72- or 32-bit chunks, so each wave's chain is
   ~17 or ~9 windows instead of 33 -- from compact base tables at offsets
   2^(72 q) or 2^(32 q) (32 or 64 MiB per device, the default's made with
   the drop-in engines).  Test / A-B hook, process-wide (default 4: eight measured
   slower). */
void
fd_ed25519_hip_dropin_set_split_waves( int waves );

unsigned long
fd_ed25519_hip_dropin_device_bytes( void );

/* Failure policy of the drop-ins.  The reference's verify cannot fail: it
   returns only the codes above (src/ballet/ed25519/fd_ed25519_user.c:
   134-229), and its tile stops the process only on input it cannot trust
   (FD_LOG_ERR, src/app/fdctl/run/tiles/fd_verify.c:67-68).  Here the GPU
   can fail.  When a drop-in launch fails (a kernel launch, a copy, the
   completion wait) -- or a drop-in engine cannot be created -- the failing
   engine is deleted, created anew and the same launch run once more: a
   transient failure costs the callers of that launch one retry and shows
   only in fd_ed25519_hip_dropin_status's recovery count.  If the retry
   fails as well, the device is lost to the drop-ins and the policy set
   here decides:

     FD_ED25519_HIP_DROPIN_ON_LOST_ABORT (the default): a message on stderr
       naming the failure, then abort() -- fail-stop, as a tile that cannot
       do its work stops the validator;
     FD_ED25519_HIP_DROPIN_ON_LOST_REJECT: fail closed -- the calls of the
       failed launch, the calls queued behind it and every later call return
       FD_ED25519_ERR_SIG without touching the device, so no signature is
       ever accepted unverified; fd_ed25519_hip_dropin_status reports the
       loss, and the caller alerts, restarts the process or calls
       fd_ed25519_hip_dropin_reset.

   There is no CPU fallback in either case: the library has one verify
   implementation, the GPU's.

   set_on_lost returns the previous policy (FD_ED25519_HIP_ERR_INVAL for an
   unknown one, nothing changed).  dropin_status returns 0 while the
   drop-ins are usable, else the error code that lost the device (an
   FD_ED25519_HIP_ERR_* code; fd_ed25519_hip_last_error in the thread that
   lost it has the message), and the count of launches that succeeded on a
   re-created engine in *recoveries (optional).  dropin_reset waits for the
   launches in flight, deletes and re-creates every drop-in engine and, if
   that succeeds, makes the drop-ins usable again: 0, or the creation's
   error code (still lost).

   What a retry or a reset can recover: a failure that leaves the HIP
   context usable (an allocation or a launch refused, a queue that could
   not be made, an error the library raised itself).  A device fault inside
   a kernel (an illegal address, a memory violation, a hardware exception)
   is sticky on ROCm: the process's context stays failed, so the retry
   fails too, the device is lost, and dropin_reset keeps returning the
   context's error code.  Only a process restart recovers from that, and a
   caller that sees dropin_reset fail should restart the process (the
   ABORT policy's default does exactly that, by ending it). */
#define FD_ED25519_HIP_DROPIN_ON_LOST_ABORT  (0)
#define FD_ED25519_HIP_DROPIN_ON_LOST_REJECT (1)

int
fd_ed25519_hip_dropin_set_on_lost( int policy );

int
fd_ed25519_hip_dropin_status( unsigned long * recoveries );

int
fd_ed25519_hip_dropin_reset( void );

/* ---- Part 2: batch engine -------------------------------------------- */

typedef struct fd_ed25519_hip_engine fd_ed25519_hip_engine_t;

/* ABI version of the two headers (include/fd_ed25519_hip.h and
   include/fd_ed25519_hip_tile.h): bumped whenever a flag's meaning, a
   struct layout or a prototype changes (3: round 3 -- engine flags 64..256,
   vservice stats' device bytes, shlink liveness words; 4: a SUCCESS verdict
   frag carries the published frag's trailer only, the tile keeps the
   payload; 5: shlink protocol word and creator, vservice lifecycle and
   end codes; 6: vservice links_per_thread; 7: vservice link_cpus; 8:
   vservice stats' leaked_on_hang, the drop-ins' device-lost state, the
   dsm16 form and its flag; 9: shlink protocol 6, flock-owned links; 10:
   the drop-in's and the pipe's host-scalar, host-decode and split-waves
   setters, latency_set_cpus; 11: Part 2b, the Ed25519 precompile
   instructions of raw transactions; 12: Part 2c, the leader signatures of
   Merkle shreds; 13: Part 2d, signed gossip and repair control packets; 14:
   Part 2e, the CRDS values of gossip pull responses and push messages; 15:
   Part 2f, sealing a leader's FEC sets; 16: Part 2g, the Reed-Solomon
   parity of a leader's FEC sets; still 16 with Part 2h, recovering received
   FEC sets, Part 2i, a block's proof-of-history hash chain, and Part 2j,
   shredding entry batches: they only add entry points, codes and one
   structure of their own, and nothing a consumer of version 16 was built
   against has changed).
   A consumer checks
   the library it loaded against the header it was built with:
   fd_ed25519_hip_abi_check( FD_ED25519_HIP_ABI_VERSION,
   sizeof(fd_ed25519_hip_slot_t), sizeof(fd_ed25519_hip_info_t),
   sizeof(fd_ed25519_hip_vservice_stats_t) ) returns 0 when they agree,
   FD_ED25519_HIP_ERR_INVAL (with fd_ed25519_hip_last_error) when not. */
#define FD_ED25519_HIP_ABI_VERSION (16U)

unsigned
fd_ed25519_hip_abi_version( void );

int
fd_ed25519_hip_abi_check( unsigned version, unsigned long slot_sz, unsigned long info_sz,
                          unsigned long vservice_stats_sz );

/* Engine API status codes (not verdicts). */
#define FD_ED25519_HIP_OK          (0)
#define FD_ED25519_HIP_ERR_INVAL   (-22)   /* bad argument / misaligned device buffer */
#define FD_ED25519_HIP_ERR_NOMEM   (-12)   /* host or device allocation failed        */
#define FD_ED25519_HIP_ERR_TIMEOUT (-110)  /* the GPU did not complete a batch in time  */
#define FD_ED25519_HIP_ERR_HIP     (-1000) /* HIP runtime error: -1000 - hipError_t    */

#define FD_ED25519_HIP_FLAG_CODES_PORTABLE (1)  /* portable-backend error codes */
/* Half-size scalars with |d| < 2^131 only (the strict form): signatures
   whose k has no such pair take the full-length multiplication.  Default:
   |d| up to 2^151 with a few more windows, the full-length form only for
   ~1e-6 of random k.  Same verdicts either way; for tests and A/B. */
#define FD_ED25519_HIP_FLAG_HALF_STRICT    (2)
/* The dsm phase runs one signature per lane (throughput) or, for chunks of
   at most FD_ED25519_HIP_QUAD_MAX_DEFAULT signatures,
   one per quad of lanes (latency: each group operation in one
   multiplication's time), and for at most FD_ED25519_HIP_OCT_MAX_DEFAULT
   one per two quads (the two halves of the multi-scalar sum in parallel)
   (fd_ed25519_hip_engine_set_forms moves both thresholds).  These force
   one form (tests / A-B). */
#define FD_ED25519_HIP_FLAG_DSM_QUAD       (4)
#define FD_ED25519_HIP_FLAG_DSM_WIDE       (8)
#define FD_ED25519_HIP_FLAG_DSM_OCT        (16)
/* The engine keeps to its one stream (no side stream for the decode
   overlap): for engines whose batches overlap one another already (the
   pool's and the pipe's slots), where extra streams only crowd the
   device's few hardware queues. */
#define FD_ED25519_HIP_FLAG_ONE_STREAM     (32)
/* A large chunk's phases in sequence on the call's stream (no decode side
   stream, below), and a call of several chunks on one set of work arrays
   (no second lane, fd_ed25519_hip_verify_dev): same verdicts; A/B and
   tests.  FLAG_ONE_STREAM implies both.  The library reads no environment
   variable for its launch forms. */
#define FD_ED25519_HIP_FLAG_NO_OVERLAP     (64)
#define FD_ED25519_HIP_FLAG_NO_PIPELINE    (128)
/* The half-size form's two base tables at radix 2^16 ([0..2^16)B and
   [0..2^16)[2^144]B, 8 MiB each, shared by the process's compact engines
   of a device) instead of radix 2^24 (2 GiB each): 9 + 7 instead of 6 + 5
   mixed additions per signature, same verdicts.  For processes that verify
   little and should not hold 4 GiB of device memory; the drop-ins use it. */
#define FD_ED25519_HIP_FLAG_COMPACT_TABLES (256)
/* dsm16 at every chunk size (tests / A-B): the field arithmetic itself
   spread over 16 lanes, two waves per signature (fd25519_r16.h), the
   default for chunks of at most FD_ED25519_HIP_R16_MAX_DEFAULT signatures,
   where a batch's latency is one signature's chain of group operations
   (fd_ed25519_hip_engine_set_r16_max moves the threshold).  FLAG_DSM_QUAD,
   _OCT and _WIDE exclude it. */
#define FD_ED25519_HIP_FLAG_DSM_R16        (512)
#define FD_ED25519_HIP_QUAD_MAX_DEFAULT    (32768UL)
#define FD_ED25519_HIP_OCT_MAX_DEFAULT     (8192UL)
#define FD_ED25519_HIP_R16_MAX_DEFAULT     (512UL)
/* Overlap: a large chunk's decode phase (A and R need neither the hash nor
   the scalars) runs on a side stream beside its hash and scalar phases, dsm
   after both: +1% at 1M, measured.  Per-phase timing runs the phases in
   sequence.  (FD_ED25519_HIP_FLAG_NO_OVERLAP turns it off.) */
#define FD_ED25519_HIP_OVERLAP_DEFAULT     (1)

/* Creates an engine on HIP device `device`.  max_chunk is the number of
   signatures processed per kernel sequence (0 = default 1<<20); larger
   batches are processed in chunks.  Returns NULL on failure (reason via
   fd_ed25519_hip_last_error()). */
fd_ed25519_hip_engine_t *
fd_ed25519_hip_engine_new( int device, unsigned long max_chunk, int flags );

void
fd_ed25519_hip_engine_delete( fd_ed25519_hip_engine_t * engine );

/* Device memory this process shares between all its engines on `device`:
   the half-size form's two base tables while any engine holds them (2 x 2
   GiB; 2 x 8 MiB for FD_ED25519_HIP_FLAG_COMPACT_TABLES engines), else 0.  An engine's own memory is fd_ed25519_hip_engine_info's
   device_bytes. */
unsigned long
fd_ed25519_hip_shared_device_bytes( int device );

/* Moves the chunk sizes at which the engine switches from one quad of lanes
   per signature (chunks of at most quad_max) and two quads (at most
   oct_max) to one lane per signature.  FD_ED25519_HIP_ERR_INVAL if
   oct_max > quad_max or quad_max exceeds what the engine's lane tables
   hold.  For tests and tuning; the defaults are the measured crossovers. */
int
fd_ed25519_hip_engine_set_forms( fd_ed25519_hip_engine_t * engine, unsigned long quad_max, unsigned long oct_max );

/* Chunks of at most n signatures run dsm16 (0: never); n <= the oct
   threshold.  FD_ED25519_HIP_ERR_INVAL otherwise. */
int
fd_ed25519_hip_engine_set_r16_max( fd_ed25519_hip_engine_t * engine, unsigned long n );

typedef struct {
  int           device;
  int           cu_cnt;
  int           dsm_blocks_per_cu;
  unsigned      dsm_grid;
  unsigned long max_chunk;
  unsigned long device_bytes;   /* device memory held by the engine */
  int           flags;
  char          arch[ 64 ];
  int           pci_domain;     /* the device's PCI address (tells ranks' devices apart) */
  int           pci_bus;
  int           pci_device;
} fd_ed25519_hip_info_t;

int
fd_ed25519_hip_engine_info( fd_ed25519_hip_engine_t const * engine, fd_ed25519_hip_info_t * info );

/* The engine's HIP stream (a hipStream_t).  Engine streams are drawn from
   one per-device set of GPU_MAX_HW_QUEUES streams that the library creates
   once and every engine of the process shares (at most 32; 4 by default),
   so this stream may also carry other engines' work: waiting on it
   (hipStreamSynchronize, fd_ed25519_hip_engine_sync, events recorded on
   it) waits for theirs too.  Order your own work with events recorded
   right after it, not with whole-stream waits, when other engines run. */
void *
fd_ed25519_hip_engine_stream( fd_ed25519_hip_engine_t * engine );

/* Device-resident batch: every pointer is a device pointer.  Signature i
   is sigs[64 i .. 64 i + 64) = R || S over message msgs[msg_off[i] ..
   msg_off[i] + msg_sz[i]) by public key pubs[32 i .. 32 i + 32); out[i]
   receives its code.  sigs and pubs must be 16-byte aligned; messages may
   start at any byte, and the message buffer must stay readable at least 16
   bytes past the end of the last message (the SHA-512 loader reads aligned
   16-byte granules, up to 15 bytes beyond a message's last byte; the same
   holds for fd_ed25519_hip_sign_dev / _gen_dev).  Every msg_sz[i] must be
   at most FD_ED25519_HIP_MSG_SZ_MAX (2^31 - 1): the device hashes take a
   message's remaining byte count as a signed 32-bit value, and a larger
   size gives a wrong digest (a wrong verdict), never a wild read.  The
   sizes here are device memory, so this entry point and _sign_dev cannot
   check them: the bound is the caller's.  fd_ed25519_hip_verify_host and
   _verify_txns_host return FD_ED25519_HIP_ERR_INVAL for a larger size
   before they stage anything, the drop-ins hash such a message on the
   host, the raw-input fronts (Parts 2b-2f) hash at most a packet, a
   shred or a 32-byte root, and a pipe's or pool's messages lie inside the
   msg_cap its creator chose (keep that below 2 GiB).  Enqueued on `stream` (NULL = the engine's stream) and
   returns immediately; the engine's work arrays are reused by the next
   call, so calls on one engine must be ordered on one stream.  A call of
   more than max_chunk signatures alternates its chunks between two sets of
   work arrays on two streams (the second set, max_chunk x 280 B plus the
   dsm lane tables, allocated on the first such call), so a chunk's hash,
   scalar and decode phases fill the tail of the previous chunk's dsm; the
   call still completes in order on `stream` (FD_ED25519_HIP_FLAG_NO_PIPELINE
   or FD_ED25519_HIP_FLAG_ONE_STREAM keeps one set, per-phase timing too).
   An engine whose max_chunk exceeds FD_ED25519_HIP_QUAD_MAX_DEFAULT and that
   may pipeline allocates the second set with the first, in engine_new, so
   no call allocates device memory or fails for lack of it; a smaller
   engine allocates it on its first multi-chunk call (one hipMalloc, which
   may synchronise the device once). */
#define FD_ED25519_HIP_MSG_SZ_MAX 0x7fffffffU

int
fd_ed25519_hip_verify_dev( fd_ed25519_hip_engine_t * engine,
                           unsigned long             n,
                           unsigned char const *     msgs,
                           unsigned long const *     msg_off,
                           unsigned int const *      msg_sz,
                           unsigned char const *     sigs,
                           unsigned char const *     pubs,
                           signed char *             out,
                           void *                    stream );

/* The same verification from the caller's digests: signature i's
   challenge k = SHA-512(R || A || M) mod L is reduced from digests[64 i ..
   64 i + 64) (the SHA-512 of R || A || M, computed by the caller; 16-byte
   aligned device memory), everything else as fd_ed25519_hip_verify_dev.
   For messages the device path's 32-bit sizes cannot carry (the drop-ins
   use it for messages of 4 GiB and more, hashing them on the host). */
int
fd_ed25519_hip_verify_digests_dev( fd_ed25519_hip_engine_t * engine,
                                   unsigned long             n,
                                   unsigned char const *     digests,
                                   unsigned char const *     sigs,
                                   unsigned char const *     pubs,
                                   signed char *             out,
                                   void *                    stream );

/* SHA-512 on the host (FIPS 180-4; the library's own, used for the
   drop-ins' large messages). */
void
fd_ed25519_hip_sha512( void const * data, unsigned long sz, unsigned char out[ 64 ] );

/* Per-transaction combine on the device (fd_ed25519_verify_batch_single_msg
   priority), for transactions whose signatures were verified with
   fd_ed25519_hip_verify_dev: txn t owns signatures [txn_first[t],
   txn_first[t] + txn_cnt[t]). */
int
fd_ed25519_hip_txn_combine_dev( fd_ed25519_hip_engine_t * engine,
                                unsigned long             ntxn,
                                signed char const *       sig_codes,
                                unsigned int const *      txn_first,
                                unsigned int const *      txn_cnt,
                                signed char *             txn_out,
                                void *                    stream );

/* Host-buffer batch, synchronous: messages are packed into pinned staging
   memory (any offsets / aliasing allowed), copied, verified, and the codes
   copied back to out[0..n). */
int
fd_ed25519_hip_verify_host( fd_ed25519_hip_engine_t * engine,
                            unsigned long             n,
                            unsigned char const *     msgs,
                            unsigned long const *     msg_off,
                            unsigned int const *      msg_sz,
                            unsigned char const *     sigs,
                            unsigned char const *     pubs,
                            signed char *             out );

/* Host-buffer transactions (fd_ed25519_verify_batch_single_msg semantics
   for each): txn t has message msgs[txn_msg_off[t] .. + txn_msg_sz[t]) and
   signatures/keys [txn_first[t], txn_first[t] + txn_cnt[t]) of sigs/pubs.
   out_txn[t] receives the transaction's code; out_sig (optional, may be
   NULL) the per-signature codes. */
int
fd_ed25519_hip_verify_txns_host( fd_ed25519_hip_engine_t * engine,
                                 unsigned long             ntxn,
                                 unsigned char const *     msgs,
                                 unsigned long const *     txn_msg_off,
                                 unsigned int const *      txn_msg_sz,
                                 unsigned int const *      txn_first,
                                 unsigned int const *      txn_cnt,
                                 unsigned char const *     sigs,
                                 unsigned char const *     pubs,
                                 signed char *             out_txn,
                                 signed char *             out_sig );

/* ---- Part 2b: Ed25519 precompile instructions of raw transactions ---- */

/* Besides the signatures of its signature section, a Solana transaction
   carries the Ed25519 signatures its Ed25519SigVerify111... precompile
   instructions name.  The reference verifies those one fd_ed25519_verify
   call at a time (fd_precompile_ed25519_verify,
   src/flamenco/runtime/program/fd_precompiles.c:115-200); the entry points
   below take a batch of raw payloads and do the parse, the walk of every
   offsets table (cross-instruction lookups and their bounds included), the
   gather, the verification and the reference's error priority on the
   device.

   Per transaction: the payload is parsed as fd_ed25519_hip_txn_parse
   parses it (rejected: PRECOMPILE_PARSE_FAILED).  An instruction is an
   Ed25519 precompile instruction exactly when its program account key is
   the Ed25519 program id; every other instruction is ignored.  Those that
   count are judged in instruction order, each as the reference judges it
   (header: ERR_INSTR_DATA_SIZE; then entry by entry, a failed lookup
   ERR_DATA_OFFSET, a signature fd_ed25519_verify rejects -- whatever its
   code, so both code flavours agree -- ERR_SIGNATURE, the first failing
   entry ending the instruction).  The first instruction that fails gives
   the transaction's code and, in instr_out, its index; a transaction
   without a failure (or without such an instruction) gets 0 and 0xFF.

   The three reference codes are FD_EXECUTOR_PRECOMPILE_ERR_* of
   src/flamenco/runtime/fd_executor.h:93-95; the two others are this
   library's. */
#define FD_ED25519_HIP_PRECOMPILE_ERR_SIGNATURE       ( -3)
#define FD_ED25519_HIP_PRECOMPILE_ERR_DATA_OFFSET     ( -4)
#define FD_ED25519_HIP_PRECOMPILE_ERR_INSTR_DATA_SIZE ( -5)
#define FD_ED25519_HIP_PRECOMPILE_PARSE_FAILED        (-16)
/* the caller reserved another number of entries for the transaction than
   the device's walk of it found (precompile_dev) */
#define FD_ED25519_HIP_PRECOMPILE_BAD_RESERVATION     (-17)

/* The most entries one transaction can reserve: the headers that pass
   hold 14 bytes per entry inside a 1232-byte payload, (1232-2)/14. */
#define FD_ED25519_HIP_PRECOMPILE_ENT_MAX (87UL)

/* The entries to reserve for one payload: the sum of the entry counts of
   its precompile instructions whose header passes (0 for a payload the
   parser rejects), 0..FD_ED25519_HIP_PRECOMPILE_ENT_MAX.  Host only. */
unsigned
fd_ed25519_hip_precompile_count( unsigned char const * payload, unsigned long payload_sz );

/* One entry of a payload's staging plan: offsets relative to the payload;
   pre is 0, or ERR_DATA_OFFSET for an entry with a failed lookup (its
   offsets and msg_sz are 0 then). */
typedef struct {
  unsigned char  instr;    /* index of the precompile instruction that lists the entry */
  signed char    pre;
  unsigned short sig_off;
  unsigned short pub_off;
  unsigned short msg_off;
  unsigned short msg_sz;
} fd_ed25519_hip_precompile_ent_t;

/* The staging plan of one payload, host only (no GPU): what the device's
   stage kernel lays out, from the same source.  Writes the first cap of
   the payload's precompile_count entries, in instruction then entry order,
   and returns how many it wrote.  *parse_or_header_code (optional):
   PRECOMPILE_PARSE_FAILED, or ERR_INSTR_DATA_SIZE with the index of the
   first instruction whose header fails in *instr (optional; the entries of
   instructions before it are judged ahead of it), else 0 and 0xFF. */
int
fd_ed25519_hip_precompile_plan( unsigned char const *             payload,
                                unsigned long                     payload_sz,
                                fd_ed25519_hip_precompile_ent_t * ents,
                                unsigned long                     cap,
                                signed char *                     parse_or_header_code,
                                unsigned char *                   instr );

/* Device workspace of precompile_dev for ntxn transactions and n_ent
   entries: per entry the gathered signature (64) and key (32), the
   message's offset (8) and size (4), the verify code, the lookup code and
   the instruction index; per transaction three bytes of the walk's
   summary. */
#define FD_ED25519_HIP_PRECOMPILE_WORK_BYTES( ntxn, n_ent ) \
  ( 111UL*(unsigned long)(n_ent) + 3UL*(unsigned long)(ntxn) + 16UL )

/* Device-resident batch: every pointer but the engine is a device pointer.
   Transaction t is payloads[pay_off[t] .. pay_off[t] + pay_sz[t]); the
   caller reserved the entries [ent_first[t], ent_first[t+1]) for it from
   fd_ed25519_hip_precompile_count (ent_first[0]==0, ent_first[ntxn]==n_ent,
   n_ent given by value: the call reads nothing back).  A transaction whose
   reservation differs from what the device's walk of it finds gets
   PRECOMPILE_BAD_RESERVATION; nothing is written outside its reservation
   and no other transaction's result changes.  txn_out[t] and instr_out[t]
   receive the code and the failing instruction's index (0xFF: none);
   ent_out (optional) per entry 0, ERR_DATA_OFFSET or ERR_SIGNATURE on its
   own, whatever came before it (the transaction's status for the slots of
   a rejected payload or a bad reservation).  work: 16-byte aligned,
   FD_ED25519_HIP_PRECOMPILE_WORK_BYTES( ntxn, n_ent ) bytes.

   Messages are read in place, so the payload buffer must stay readable at
   least 16 bytes past the end of the last payload and start 4-byte
   aligned (the rule of fd_ed25519_hip_verify_dev's message buffer; the
   gather reads aligned words around unaligned signatures and keys).

   Asynchronous on `stream` (NULL: the engine's) like
   fd_ed25519_hip_verify_dev, whose phases it runs over the n_ent entries
   (chunked by the engine's max_chunk; none when n_ent is 0): it allocates
   nothing beyond what that call may (its second lane on an engine's first
   multi-chunk call) and does not synchronise. */
int
fd_ed25519_hip_precompile_dev( fd_ed25519_hip_engine_t * engine,
                               unsigned long             ntxn,
                               unsigned char const *     payloads,
                               unsigned long const *     pay_off,
                               unsigned int const *      pay_sz,
                               unsigned int const *      ent_first,
                               unsigned long             n_ent,
                               void *                    work,
                               signed char *             txn_out,
                               unsigned char *           instr_out,
                               signed char *             ent_out,
                               void *                    stream );

/* Host-buffer batch, synchronous: counts every payload while packing them
   into pinned staging memory, copies, runs precompile_dev on a workspace
   the engine owns and copies txn_out[0..ntxn) and instr_out[0..ntxn)
   back. */
int
fd_ed25519_hip_precompile_host( fd_ed25519_hip_engine_t * engine,
                                unsigned long             ntxn,
                                unsigned char const *     payloads,
                                unsigned long const *     pay_off,
                                unsigned int const *      pay_sz,
                                signed char *             txn_out,
                                unsigned char *           instr_out );

/* ---- Part 2c: the leader signatures of Merkle shreds -------------------- */

/* A validator checks every incoming Merkle shred that opens a FEC set
   against its slot leader's key before it reserves anything for the set
   (fd_fec_resolver_add_shred, src/disco/shred/fd_fec_resolver.c:283-440):
   it parses the shred (fd_shred_parse, src/ballet/shred/fd_shred.c:3-72),
   rejects impossible headers (:311-359), hashes about a kilobyte of the
   shred into a Merkle leaf, walks the shred's inclusion proof of 20-byte
   nodes up to the 32-byte root and calls fd_ed25519_verify( root, 32,
   shred->signature, leader_pubkey ).  The entry points below take a batch of
   raw shreds with their leaders' keys and do all of that on the device.

   Per shred: a shred fd_shred_parse rejects gets SHRED_ERR_PARSE.  The
   resolver of this reference handles unchained Merkle shreds only (variant
   0x8? data, 0x4? code); every other variant that parses (chained, resigned,
   legacy) gets SHRED_UNSUPPORTED and belongs on the caller's CPU path.  A
   judged shred with an all-zero signature, a code shred with data_cnt or
   code_cnt zero or above 67, an index inside its FEC set of 67 or more, or
   a proof too short for its index gets SHRED_ERR_HEADER; one whose derived
   root fd_ed25519_verify does not accept under the leader's key -- whatever
   its code, so both code flavours agree -- gets SHRED_ERR_SIGNATURE; every
   other shred gets 0.  SHRED_ERR_HEADER and SHRED_ERR_SIGNATURE are where
   the resolver returns FD_FEC_RESOLVER_SHRED_REJECTED for a shred that
   opens a set.  The resolver's state (its map of sets, duplicates,
   consistency with a set's earlier shreds, Reed-Solomon recovery) stays
   with the caller.  All five codes are this library's. */
#define FD_ED25519_HIP_SHRED_OK            (  0)
#define FD_ED25519_HIP_SHRED_ERR_PARSE     (-16)
#define FD_ED25519_HIP_SHRED_UNSUPPORTED   (-18)
#define FD_ED25519_HIP_SHRED_ERR_HEADER    (-19)
#define FD_ED25519_HIP_SHRED_ERR_SIGNATURE (-20)

/* The root one shred's leader signed, host only (no GPU), from the same
   source as the device's stage kernel: parses, applies the header rules,
   hashes the leaf and walks the proof.  Returns 0 with root[0..32) written,
   else SHRED_ERR_PARSE, SHRED_UNSUPPORTED or SHRED_ERR_HEADER (root
   untouched).  Reads shred[0..sz) only. */
int
fd_ed25519_hip_shred_root( unsigned char const * shred,
                           unsigned long         sz,
                           unsigned char *       root );

/* Device workspace of shreds_dev for n shreds: per shred the root as the
   verify message (32), the gathered signature (64), the message's offset
   (8) and size (4), the verify code and the stage's code. */
#define FD_ED25519_HIP_SHRED_WORK_BYTES( n ) ( 110UL*(unsigned long)(n) + 16UL )

/* Device-resident batch: every pointer but the engine is a device pointer.
   Shred i is shreds[shred_off[i] .. shred_off[i] + shred_sz[i]) and may
   start at any byte; leaders + 32 i is its slot leader's public key (the
   array 16-byte aligned: the verify phases read it in place).  out[i]
   receives the shred's code.  roots (optional, 16-byte aligned) receives
   the derived root of every judged shred that passed the header rules at
   roots + 32 i, 32 zero bytes for any other; sig_out (optional) fd_ed25519_verify's own code for
   the same shreds (in the engine's code flavour) and 0 for any other.
   work: 16-byte aligned, FD_ED25519_HIP_SHRED_WORK_BYTES( n ) bytes.

   The shred buffer must start 16-byte aligned and stay readable at least
   16 bytes past the end of the last shred (the rule of
   fd_ed25519_hip_verify_dev's message buffer: the stage reads aligned
   words around unaligned bytes).

   Asynchronous on `stream` (NULL: the engine's) like
   fd_ed25519_hip_verify_dev, whose phases it runs over the n roots
   (chunked by the engine's max_chunk): it allocates nothing beyond what
   that call may (its second lane on an engine's first multi-chunk call)
   and does not synchronise. */
int
fd_ed25519_hip_shreds_dev( fd_ed25519_hip_engine_t * engine,
                           unsigned long             n,
                           unsigned char const *     shreds,
                           unsigned long const *     shred_off,
                           unsigned int const *      shred_sz,
                           unsigned char const *     leaders,
                           void *                    work,
                           signed char *             out,
                           unsigned char *           roots,
                           signed char *             sig_out,
                           void *                    stream );

/* Host-buffer batch, synchronous: packs the shreds into pinned staging
   memory (in chunks, so any n fits), copies, runs shreds_dev on a
   workspace the engine owns and copies out[0..n) and, when roots is not
   NULL, roots[0..32 n) back. */
int
fd_ed25519_hip_shreds_host( fd_ed25519_hip_engine_t * engine,
                            unsigned long             n,
                            unsigned char const *     shreds,
                            unsigned long const *     shred_off,
                            unsigned int const *      shred_sz,
                            unsigned char const *     leaders,
                            signed char *             out,
                            unsigned char *           roots );

/* ---- Part 2d: signed gossip and repair control packets ------------------ */

/* A validator's gossip and repair ports take unauthenticated UDP packets;
   for each, the reference decodes the whole bincode message and calls
   fd_ed25519_verify before it decides whether to answer
   (fd_gossip_recv_packet, src/flamenco/gossip/fd_gossip.c:1858, with
   fd_gossip_handle_ping :646, _pong :912, _prune :1201;
   fd_repair_recv_serv_packet, src/flamenco/repair/fd_repair.c:1012).  The
   entry points below take a batch of raw packets of one protocol with the
   validator's own identity and do that on the device for the kinds of fixed
   or nearly fixed layout: gossip ping, pong and prune, and the repair
   requests window_index, highest_window_index and orphan.

   Per packet: one the reference's decode rejects, or that it decodes with
   bytes left over, gets PACKET_ERR_PARSE -- and so does one of fewer than 4
   or more than FD_ED25519_HIP_PACKET_MAX bytes (no larger UDP payload
   reaches the reference's handlers).  A gossip pull request, pull response
   or push message gets PACKET_UNSUPPORTED without a further look: the
   CRDS values of the last two are Part 2e's, and a pull request stays on
   the caller's CPU path; so do, where they decode, a repair pong (its signed message is a hash of the caller's own ping
   token), ancestor_hashes and the seven legacy request kinds.  A prune
   message whose destination, or a repair request whose recipient, is not
   self_key gets PACKET_NOT_FOR_SELF: the reference drops it unverified.  A
   judged packet that fd_ed25519_verify does not accept -- whatever its code,
   so both code flavours agree -- gets PACKET_ERR_SIGNATURE, every other one
   0.  A prune message is verified under data.pubkey over the bytes
   fd_gossip_prune_sign_data_encode produces, as the reference does; a
   gossip pong's active-table lookup and token comparison (fd_gossip.c:913-938,
   without side effect) stay with the caller.  All five codes are this
   library's. */
#define FD_ED25519_HIP_PROTO_GOSSIP      (0)   /* what fd_gossip_recv_packet takes      */
#define FD_ED25519_HIP_PROTO_REPAIR_SERV (1)   /* what fd_repair_recv_serv_packet takes */

#define FD_ED25519_HIP_PACKET_OK            (  0)
#define FD_ED25519_HIP_PACKET_ERR_PARSE     (-16)  /* the reference's decode fails or leaves bytes over */
#define FD_ED25519_HIP_PACKET_UNSUPPORTED   (-18)  /* decodes, not judged here: the caller's CPU path  */
#define FD_ED25519_HIP_PACKET_ERR_SIGNATURE (-20)
#define FD_ED25519_HIP_PACKET_NOT_FOR_SELF  (-21)  /* addressed to another identity: the reference drops it unverified */

#define FD_ED25519_HIP_PACKET_MAX (1232UL)         /* PACKET_DATA_SIZE, fd_gossip.c:17 */

/* The rules for one packet, host only (no GPU), from the same source as the
   device's stage kernel.  Returns 0 with the plan filled -- the key at
   pkt[key_off..+32), the signature at pkt[sig_off..+64), the signed message
   pkt[msg0_off..+msg0_sz) followed by pkt[msg1_off..+msg1_sz) (msg1_sz may be
   0) -- else PACKET_ERR_PARSE, PACKET_UNSUPPORTED or PACKET_NOT_FOR_SELF
   with every offset and size zero.  disc is the packet's discriminant
   wherever 4 <= sz <= FD_ED25519_HIP_PACKET_MAX.  An unknown proto, a NULL
   self_key or a NULL plan gives FD_ED25519_HIP_ERR_INVAL.  Reads pkt[0..sz)
   only. */
typedef struct {
  unsigned short key_off, sig_off, msg0_off, msg0_sz, msg1_off, msg1_sz;
  unsigned int   disc;
} fd_ed25519_hip_packet_plan_t;

int
fd_ed25519_hip_packet_plan( int                            proto,
                            unsigned char const *          pkt,
                            unsigned long                  sz,
                            unsigned char const            self_key[ 32 ],
                            fd_ed25519_hip_packet_plan_t * plan );

/* Device workspace of packets_dev for n packets in a buffer of pkt_bytes
   bytes: per packet the gathered signature (64) and key (32), the message's
   offset (8) and size (4), the verify code and the stage's code; and a
   mirror of the packet buffer that holds each message at its packet's
   place (pkt_bytes + 16, rounded up to 16). */
#define FD_ED25519_HIP_PACKET_WORK_BYTES( n, pkt_bytes ) \
  ( 110UL*(unsigned long)(n) + ( ( (unsigned long)(pkt_bytes) + 31UL ) & ~15UL ) )

/* Device-resident batch: every pointer but the engine and self_key is a
   device pointer.  Packet i is pkts[pkt_off[i] .. pkt_off[i] + pkt_sz[i])
   and may start at any byte.  Packets must not overlap one another in the
   buffer (each message is laid out at its packet's own place in the
   workspace), and pkt_off[i] + pkt_sz[i] <= pkt_bytes: a packet that leaves
   that range gets PACKET_ERR_PARSE and is not read.  self_key is the
   validator's identity on the host; it travels by value in the launch.
   out[i] receives the packet's code; sig_out (optional) fd_ed25519_verify's
   own code for every judged packet (in the engine's code flavour) and 0 for
   any other.  work: 16-byte aligned, FD_ED25519_HIP_PACKET_WORK_BYTES( n,
   pkt_bytes ) bytes.

   The packet buffer must start 16-byte aligned and stay readable at least
   16 bytes past pkt_bytes (the rule of fd_ed25519_hip_verify_dev's message
   buffer: the stage reads aligned words around unaligned bytes).

   Asynchronous on `stream` (NULL: the engine's) like
   fd_ed25519_hip_verify_dev, whose phases it runs over the n slots (chunked
   by the engine's max_chunk): it allocates nothing beyond what that call
   may (its second lane on an engine's first multi-chunk call) and does not
   synchronise.  An unknown proto or a NULL self_key gives
   FD_ED25519_HIP_ERR_INVAL; n==0 is a no-op. */
int
fd_ed25519_hip_packets_dev( fd_ed25519_hip_engine_t * engine,
                            int                       proto,
                            unsigned long             n,
                            unsigned char const *     pkts,
                            unsigned long const *     pkt_off,
                            unsigned int const *      pkt_sz,
                            unsigned long             pkt_bytes,
                            unsigned char const       self_key[ 32 ],
                            void *                    work,
                            signed char *             out,
                            signed char *             sig_out,
                            void *                    stream );

/* Host-buffer batch, synchronous: packs the packets back to back into
   pinned staging memory (in passes, so any n fits; here packets may
   overlap or repeat in the caller's buffer), copies, runs packets_dev on a
   workspace the engine owns and copies out[0..n) back.  A packet of more
   than FD_ED25519_HIP_PACKET_MAX bytes travels as its size alone. */
int
fd_ed25519_hip_packets_host( fd_ed25519_hip_engine_t * engine,
                             int                       proto,
                             unsigned long             n,
                             unsigned char const *     pkts,
                             unsigned long const *     pkt_off,
                             unsigned int const *      pkt_sz,
                             unsigned char const       self_key[ 32 ],
                             signed char *             out );

/* ---- Part 2e: the CRDS values of gossip pull responses and push messages -- */

/* Most of the signed traffic of a validator's gossip port is CRDS values: a
   pull response or a push message carries several, each with a signature of
   its own, and the reference verifies them one fd_ed25519_verify call at a
   time (fd_gossip_recv_crds_value, src/flamenco/gossip/fd_gossip.c:1020-1091,
   called for every value at :1420-1430).  The entry points below take a batch
   of raw gossip packets with the validator's own identity and do the bincode
   walk of every fd_crds_data variant, the choice of each value's key, the
   gather and the verification on the device.  The reservation model is Part
   2b's: the caller reserves each packet's value slots from crds_count.

   Per packet: one the reference's fd_gossip_msg_decode rejects, or decodes
   with bytes left over, gets CRDS_ERR_PARSE and none of its values a verdict
   (fd_gossip_recv_packet drops the packet whole, fd_gossip.c:1868-1877) --
   and so does one of fewer than 4 or more than FD_ED25519_HIP_PACKET_MAX
   bytes.  A pull request, prune, ping or pong gets CRDS_UNSUPPORTED unread:
   they are Part 2d's, or (the pull request, in which the reference verifies
   nothing) the caller's.  A pull response or push message that decodes gets
   0.

   Per value of a decoded packet: the key is the variant's own id / from for
   data discriminants 0..10 and the message's outer pubkey for 11
   (contact_info_v2: the reference's switch has no case for it,
   fd_gossip.c:1023-1071).  A value whose key is self_key gets CRDS_OWN: the
   reference drops it unverified (:1072).  The reference then signs over a
   re-encode of the decoded value (:1075-1082), not over the received bytes.
   For data discriminants 0..10 the two are equal for every encoding its
   decoders accept, and the signed message -- the value's data, discriminant
   and fields -- is read in place.  For contact_info_v2 they never are: the
   reference decodes version_v3's fields and the socket entries' offsets as
   compact-u16 and encodes them as plain u16 (fd_types.c:20626-20636 against
   :20703-20713, :21109 against :21162), so it verifies bytes no peer signed.
   Such a value gets CRDS_UNSUPPORTED and stays with the caller: this library
   gives no verdict over bytes the reference would not have hashed.  A value
   that fd_ed25519_verify does not accept -- whatever its code, so both code
   flavours agree -- gets CRDS_ERR_SIGNATURE, every other one 0.  All codes
   are this library's. */
#define FD_ED25519_HIP_CRDS_OK              (  0)
#define FD_ED25519_HIP_CRDS_ERR_PARSE       (-16)  /* the reference's decode fails or leaves bytes over */
/* the caller reserved another number of values for the packet than the
   device's walk of it found (crds_dev) */
#define FD_ED25519_HIP_CRDS_BAD_RESERVATION (-17)
#define FD_ED25519_HIP_CRDS_UNSUPPORTED     (-18)  /* a packet: no pull response or push message; a value: contact_info_v2 */
#define FD_ED25519_HIP_CRDS_ERR_SIGNATURE   (-20)
#define FD_ED25519_HIP_CRDS_OWN             (-21)  /* under the own identity: the reference drops it unverified */

/* The most values one packet can decode to.  The smallest encodable value
   is a version_v1 without commit: signature 64, data discriminant 4, from
   32, wallclock 8, three u16, option tag 1 = 115 bytes (every other variant
   is longer: slot_hashes 116, epoch_slots 117, version_v2 119,
   node_instance 124, contact_info_v2 126, duplicate_shred 133, lowest_slot
   141, incremental_snapshot_hashes 156, contact_info_v1 210, a vote more);
   the values follow 44 bytes (message discriminant 4, pubkey 32, crds_len 8)
   inside a 1232-byte packet: (1232-44)/115. */
#define FD_ED25519_HIP_CRDS_VAL_MAX (10UL)

/* The values to reserve for one packet: crds_len for a pull response or push
   message that decodes, 0 for any other packet, 0..FD_ED25519_HIP_CRDS_VAL_MAX.
   Host only. */
unsigned
fd_ed25519_hip_crds_count( unsigned char const * pkt, unsigned long sz );

/* One value of a packet's staging plan: offsets relative to the packet.
   The signature is pkt[sig_off..+64), the key pkt[key_off..+32), the signed
   message pkt[msg_off..+msg_sz), which starts with disc, the data
   discriminant; the value's own bytes, the ones hash_out hashes, are
   pkt[sig_off..msg_off+msg_sz).  pre is 0, CRDS_OWN or CRDS_UNSUPPORTED (the
   offsets are filled all the same; for CRDS_UNSUPPORTED they name the
   received bytes, which are not what the reference verifies). */
typedef struct {
  unsigned int   disc;
  unsigned short sig_off;
  unsigned short key_off;
  unsigned short msg_off;
  unsigned short msg_sz;
  signed char    pre;
} fd_ed25519_hip_crds_val_t;

/* The staging plan of one packet, host only (no GPU): what the device's
   stage kernel lays out, from the same source.  Writes the first cap of the
   packet's crds_count values (vals may be NULL with cap 0) and returns how
   many it wrote; *pkt_code (optional) receives the packet's code.  A NULL
   self_key gives FD_ED25519_HIP_ERR_INVAL.  Reads pkt[0..sz) only. */
int
fd_ed25519_hip_crds_plan( unsigned char const *       pkt,
                          unsigned long               sz,
                          unsigned char const         self_key[ 32 ],
                          fd_ed25519_hip_crds_val_t * vals,
                          unsigned long               cap,
                          signed char *               pkt_code );

/* Device workspace of crds_dev for n packets and n_val values: per value
   the gathered signature (64) and key (32), the message's offset (8) and
   size (4), the size of the value's data (4), the verify code and the
   stage's code; per packet its code.  No message area: messages are read in
   place. */
#define FD_ED25519_HIP_CRDS_WORK_BYTES( n, n_val ) \
  ( 114UL*(unsigned long)(n_val) + (unsigned long)(n) + 16UL )

/* Device-resident batch: every pointer but the engine and self_key is a
   device pointer.  Packet i is pkts[pkt_off[i] .. pkt_off[i] + pkt_sz[i])
   and may start at any byte; the caller reserved the values [val_first[i],
   val_first[i+1]) for it from fd_ed25519_hip_crds_count (val_first[0]==0,
   val_first[n]==n_val, n_val given by value: the call reads nothing back).
   A packet that decodes but whose reservation differs from what the
   device's walk of it finds gets CRDS_BAD_RESERVATION; nothing is written
   outside its reservation and no other packet's result changes.  A
   val_first that is no such prefix sum is survived: a packet whose range
   runs backwards or leaves [0, n_val) fills no slot, and a slot no packet
   fills gets CRDS_BAD_RESERVATION in val_out.
   pkt_off[i] + pkt_sz[i] <= pkt_bytes: a packet that leaves that range gets
   CRDS_ERR_PARSE and is not read.

   pkt_out[i] receives the packet's code.  val_out per value: 0,
   CRDS_ERR_SIGNATURE, CRDS_OWN or CRDS_UNSUPPORTED; for the slots of a packet
   whose code is not 0, that code.  sig_out (optional): fd_ed25519_verify's own code for
   every verified value (in the engine's code flavour) and 0 for any other.
   hash_out (optional, 32 bytes a value, 4-byte aligned): the SHA-256 of the
   value's own bytes, signature through end of data -- the key of the
   reference's value table (fd_gossip.c:1093-1105; the lookup stays with the
   caller) -- for every value of a packet whose code is 0, CRDS_OWN ones
   included, but for contact_info_v2 (the reference hashes a re-encode there
   too), and zero for the others; the pass that computes it runs only when it
   is asked for.  work: 16-byte aligned,
   FD_ED25519_HIP_CRDS_WORK_BYTES( n, n_val ) bytes.

   Messages are read in place, so the rules for the packet buffer are
   precompile_dev's: it starts 4-byte aligned and stays readable at least 16
   bytes past pkt_bytes, and packets do not overlap.

   Asynchronous on `stream` (NULL: the engine's) like
   fd_ed25519_hip_verify_dev, whose phases it runs over the n_val slots
   (chunked by the engine's max_chunk; none when n_val is 0): it allocates
   nothing beyond what that call may (its second lane on an engine's first
   multi-chunk call) and does not synchronise.  A NULL self_key gives
   FD_ED25519_HIP_ERR_INVAL; n==0 is a no-op. */
int
fd_ed25519_hip_crds_dev( fd_ed25519_hip_engine_t * engine,
                         unsigned long             n,
                         unsigned char const *     pkts,
                         unsigned long const *     pkt_off,
                         unsigned int const *      pkt_sz,
                         unsigned long             pkt_bytes,
                         unsigned char const       self_key[ 32 ],
                         unsigned int const *      val_first,
                         unsigned long             n_val,
                         void *                    work,
                         signed char *             pkt_out,
                         signed char *             val_out,
                         signed char *             sig_out,
                         unsigned char *           hash_out,
                         void *                    stream );

/* Host-buffer batch, synchronous: counts every packet while packing them
   back to back into pinned staging memory (in as many passes as the engine's
   staging needs, so any n fits; here packets may overlap or repeat in the
   caller's buffer), copies, runs crds_dev on a workspace the engine owns and
   copies the results back.  val_first_out[0..n] receives the prefix sums of
   the counts it used: the values of packet i are val_out[val_first_out[i] ..
   val_first_out[i+1]), and hash_out (optional) is indexed the same way.  The
   caller sizes val_out (and hash_out) for the sum of
   fd_ed25519_hip_crds_count over the batch, at most
   n*FD_ED25519_HIP_CRDS_VAL_MAX.  A packet of more than
   FD_ED25519_HIP_PACKET_MAX bytes travels as its size alone. */
int
fd_ed25519_hip_crds_host( fd_ed25519_hip_engine_t * engine,
                          unsigned long             n,
                          unsigned char const *     pkts,
                          unsigned long const *     pkt_off,
                          unsigned int const *      pkt_sz,
                          unsigned char const       self_key[ 32 ],
                          unsigned int *            val_first_out,
                          signed char *             pkt_out,
                          signed char *             val_out,
                          unsigned char *           hash_out );

/* ---- Part 2f: sealing a leader's FEC sets ------------------------------- */

/* The other half of the shred path.  A leader seals every FEC set before it
   leaves the box (fd_shredder_next_fec_set, src/disco/shred/fd_shredder.c:
   225-260): it hashes each data and parity shred into a Merkle leaf, builds
   the tree of 20-byte nodes over them (fd_bmtree_commit_*,
   src/ballet/bmtree/fd_bmtree.c:216-348), signs the 32-byte root and copies
   the signature and each shred's inclusion proof into the shreds -- the
   inverse of what Part 2c checks.  The entry points below take a batch of
   sets whose shreds are filled but for those two fields and do all of that
   on the device.

   A set is cnt shreds in tree order, the data shreds first, then the parity
   shreds; shred j of the set is leaf j.  A set of no shreds or of more than
   FEC_SET_MAX gets FEC_ERR_SET and none of its shreds is read.  Otherwise
   the first shred in set order that fails decides the set's code: one
   fd_shred_parse rejects gives FEC_ERR_PARSE; one that parses but is no
   unchained Merkle shred (variant 0x8? data, 0x4? code) FEC_UNSUPPORTED; one
   whose proof depth (variant & 0xf) is not the shredder's for cnt leaves
   (fd_bmtree_depth( cnt ) - 1, fd_shredder.c:158), a code shred with
   data_cnt or code_cnt zero or above 67, or a shred whose header places it
   elsewhere in the set than j (data: idx - fec_set_idx, code: data_cnt +
   code.idx) FEC_ERR_SET.  The signature field is an output: Part 2c's
   rejection of an all-zero signature does not apply.  A set with a code has
   no byte of any of its shreds written and does not affect any other set.
   A sealed set's shreds all get 0 from fd_ed25519_hip_shreds_dev under the
   key's public key.  All four codes are this library's; they reuse Part
   2c's numbering.

   The parity shreds come in filled, as fd_shredder.c:167-223 produces them
   before the tree: Part 2g fills them on the device.  Out of scope: the
   construction of shred headers, and chained and resigned variants, which
   the reference's shredder does not emit. */
#define FD_ED25519_HIP_FEC_OK          (  0)
#define FD_ED25519_HIP_FEC_ERR_PARSE   (-16)
#define FD_ED25519_HIP_FEC_UNSUPPORTED (-18)
#define FD_ED25519_HIP_FEC_ERR_SET     (-19)
#define FD_ED25519_HIP_FEC_SET_MAX     (134UL)   /* 67 data + 67 parity shreds */

/* The root of one set and, optionally, its proofs, host only (no GPU), from
   the same source as the device's tree kernel.  Shred j of the set is
   shreds[shred_off[j] .. shred_off[j] + shred_sz[j]), j < cnt.  Returns 0
   with root[0..32) written and, when proofs is not NULL, leaf j's proof
   nodes at proofs + 20 depth j (depth = 0 for cnt 1, else the bits of cnt-1);
   else the set's code, root and proofs untouched.  The shreds are only
   read, shred j its bytes [0, shred_sz[j]). */
int
fd_ed25519_hip_fec_root( unsigned char const * shreds,
                         unsigned long const * shred_off,
                         unsigned int const *  shred_sz,
                         unsigned long         cnt,
                         unsigned char *       root,
                         unsigned char *       proofs );

/* Device workspace of fec_seal_dev for n shreds in n_set sets: per set the
   signature (64), its public key (32), the root as the message signed (32),
   the message's offset (8) and size (4); per shred the set that sealed it
   (4). */
#define FD_ED25519_HIP_FEC_WORK_BYTES( n, n_set ) \
  ( 140UL*(unsigned long)(n_set) + 4UL*(unsigned long)(n) + 16UL )

/* Device-resident batch: every pointer but the engine is a device pointer.
   Shred i is shreds[shred_off[i] .. shred_off[i] + shred_sz[i]) and may
   start at any byte; shreds do not overlap.  Set k is the shreds
   [set_first[k], set_first[k+1]) in tree order (set_first[0]==0,
   set_first[n_set]==n).  A set_first that is no such prefix sum is
   survived: a set whose range runs backwards or leaves [0, n) gets
   FEC_ERR_SET and touches nothing.  privs + 32 k is the private key that
   signs set k (the array 16-byte aligned), or privs is NULL: then proofs and
   roots are produced and bytes [0, 64) of every shred are left as they were
   -- the reference's keyguard split, where the caller has the roots signed
   elsewhere.

   The shreds are written in place: in a set whose code is 0, bytes [0, 64)
   of every shred receive the signature of the set's root and the 20 depth
   bytes that end the shred (at 1203 for data, 1228 for code) its proof;
   no other byte of the buffer changes, whatever the shreds' alignment.
   set_out[k] receives the set's code.  roots (optional, 16-byte aligned)
   receives the root of every sealed set at roots + 32 k, zero for any other;
   sigs (optional, 16-byte aligned, needs privs) its signature at sigs + 64 k,
   zero for any other.  work: 16-byte aligned,
   FD_ED25519_HIP_FEC_WORK_BYTES( n, n_set ) bytes.

   The shred buffer must start 16-byte aligned and stay readable at least 16
   bytes past the end of the last shred, as for fd_ed25519_hip_shreds_dev.
   n < 2^32, n_set < 2^31.

   Asynchronous on `stream` (NULL: the engine's): three launches (the tree
   and the proofs, fd_ed25519_hip_sign_dev's kernel over the roots, the
   signatures into the shreds; the tree alone without privs); it allocates
   nothing and does not synchronise.  n_set==0 is a no-op. */
int
fd_ed25519_hip_fec_seal_dev( fd_ed25519_hip_engine_t * engine,
                             unsigned long             n,
                             unsigned char *           shreds,
                             unsigned long const *     shred_off,
                             unsigned int const *      shred_sz,
                             unsigned long             n_set,
                             unsigned int const *      set_first,
                             unsigned char const *     privs,
                             void *                    work,
                             signed char *             set_out,
                             unsigned char *           roots,
                             unsigned char *           sigs,
                             void *                    stream );

/* Host-buffer batch, synchronous: packs whole sets into pinned staging
   memory (in passes, so any n fits), copies, runs fec_seal_dev on a
   workspace the engine owns and copies back set_out[0..n_set), roots and
   sigs when not NULL, and into the caller's shreds the signature (with
   privs) and the proof of every shred of a sealed set -- nothing else.  No
   alignment is asked of any argument. */
int
fd_ed25519_hip_fec_seal_host( fd_ed25519_hip_engine_t * engine,
                              unsigned long             n,
                              unsigned char *           shreds,
                              unsigned long const *     shred_off,
                              unsigned int const *      shred_sz,
                              unsigned long             n_set,
                              unsigned int const *      set_first,
                              unsigned char const *     privs,
                              signed char *             set_out,
                              unsigned char *           roots,
                              unsigned char *           sigs );

/* ---- Part 2g: the Reed-Solomon parity of a leader's FEC sets ------------ */

/* The step before the seal.  fd_shredder_next_fec_set fills a set's parity
   shreds from its data shreds (fd_reedsol_encode_fini,
   src/disco/shred/fd_shredder.c:167-223) and only then builds the tree.  The
   entry points below take sets whose data shreds and parity headers (the
   first 0x59 bytes of a code shred) are filled and compute the parity.
   Followed by Part 2f over the same arrays they are fd_shredder_next_fec_set
   from line 167 on.

   The code is the reference's: over GF(2^8) with the polynomial 0x11D, byte
   b of parity shred j of a set of d data shreds is P_b( d + j ), P_b the
   polynomial of degree < d with P_b( i ) = byte b of data shred i.  The
   bytes it protects, with P = 1139 - 20 depth and depth the proof depth of
   the set's d + p shreds: [0x40, 0x40 + P) of a data shred, [0x59,
   0x59 + P) of a code shred -- both end where the proof begins.

   A set is judged as in Part 2f, with the same four codes, and then shred
   by shred, the first failing shred deciding as there: a data shred behind
   a code shred, a 68th data shred, a data shred as the set's last (no
   parity), a code shred at place 0 (no data), and a code shred whose
   data_cnt is not the set's number of data shreds or whose code_cnt is not
   its number of code shreds get FEC_ERR_SET (Part 2f takes a code shred's
   counts as they come; the parity cannot).  In a set with code 0 exactly
   the bytes [0x59, 0x59 + P) of every code shred are written; a set with a
   code has no byte of any of its shreds written. */

/* One set, host only (no GPU), from the same source as the device's kernel.
   Shred j of the set is shreds[shred_off[j] .. shred_off[j] + shred_sz[j]),
   j < cnt; shreds do not overlap.  Returns 0 with the parity regions of the
   set's code shreds written in place, else the set's code with nothing
   written. */
int
fd_ed25519_hip_fec_parity( unsigned char *       shreds,
                           unsigned long const * shred_off,
                           unsigned int const *  shred_sz,
                           unsigned long         cnt );

/* Device-resident batch: every pointer but the engine is a device pointer,
   with fd_ed25519_hip_fec_seal_dev's rules for them: shred i is
   shreds[shred_off[i] .. shred_off[i] + shred_sz[i]) and may start at any
   byte; shreds do not overlap; the buffer starts 16-byte aligned and stays
   readable at least 16 bytes past the end of the last shred; set k is the
   shreds [set_first[k], set_first[k+1]) in tree order, and a range that
   runs backwards or leaves [0, n) gets FEC_ERR_SET and touches nothing.
   n < 2^32, n_set < 2^31.  set_out[k] receives the set's code.

   Asynchronous on `stream` (NULL: the engine's): one launch, whose tables
   the engine made when it was created; no workspace, no allocation, no
   synchronisation.  n_set==0 is a no-op. */
int
fd_ed25519_hip_fec_parity_dev( fd_ed25519_hip_engine_t * engine,
                               unsigned long             n,
                               unsigned char *           shreds,
                               unsigned long const *     shred_off,
                               unsigned int const *      shred_sz,
                               unsigned long             n_set,
                               unsigned int const *      set_first,
                               signed char *             set_out,
                               void *                    stream );

/* Host-buffer batch, synchronous: packs whole sets into pinned staging
   memory (in passes, so any n fits) -- a code shred travels as its first
   0x59 bytes and its size, since the device writes the rest --, copies, runs
   fec_parity_dev and copies back set_out[0..n_set) and, into the caller's
   code shreds of every set with code 0, the parity region -- nothing else.
   No alignment is asked of any argument. */
int
fd_ed25519_hip_fec_parity_host( fd_ed25519_hip_engine_t * engine,
                                unsigned long             n,
                                unsigned char *           shreds,
                                unsigned long const *     shred_off,
                                unsigned int const *      shred_sz,
                                unsigned long             n_set,
                                unsigned int const *      set_first,
                                signed char *             set_out );

/* ---- Part 2h: recovering received FEC sets ------------------------------ */

/* The other direction of Part 2g, the step every validator but the leader
   runs on every FEC set: the second half of fd_fec_resolver_add_shred
   (src/disco/shred/fd_fec_resolver.c:474-594).  Once data_cnt shreds of a
   set are in, the resolver regenerates the missing ones
   (fd_reedsol_recover_fini), fills their signatures and headers, rebuilds
   the tree and keeps the set only if everything agrees.  The entry points
   below do the first two steps; followed by Part 2f without keys (which
   writes the proofs and leaves the signatures alone) and Part 2c under the
   leader's key over the same arrays, they are the resolver from line 474
   on: Part 2c gives 0 for every shred exactly when the rebuilt tree's root
   is the one the leader signed.

   A set is cnt = d + p slots in tree order, each shred_sz[j] bytes at
   shred_off[j], with one erased byte per slot: 0, the slot holds a received
   shred; nonzero, it is erased and nothing of it is read.  The first d
   received slots in set order are the basis (as in fd_reedsol_recover_fini)
   and determine the protected region (Part 2g) of every other slot: an
   erased one is written, a received one is compared.

   A received slot is judged as in Part 2f.  d is the data_cnt of the set's
   first received code shred that passes Part 2f's rules (no header byte is
   read that the parser has not proved present).  The first failing slot in
   set order decides:
   an erased slot of fewer than 1203 bytes at a place below d, or fewer than
   1228 at or behind it, gets FEC_ERR_PARSE; a received data shred at a place
   >= d, and a received code shred whose data_cnt is not d or whose code_cnt
   is not cnt - d, get FEC_ERR_SET.  Then the set: no received code shred,
   FEC_ERR_SET (the resolver learns data_cnt only from one); fewer than d
   received, FEC_ERR_PARTIAL; a received slot beyond the basis that differs
   from its recomputed region in any byte, FEC_ERR_CORRUPT; then, on the set
   as it would stand (fd_fec_resolver.c:546-572), a recovered data shred
   that Part 2f's rules do not pass at its place, a data shred whose slot,
   version, fec_set_idx or parent_off is not data shred 0's, and a received
   code shred whose slot, version or fec_set_idx is not data shred 0's,
   FEC_ERR_SET.

   A set with a nonzero code has no byte of any slot written.  In a set with
   code 0 nothing of a received slot is written; an erased data slot gets
   bytes [0, 64), the signature of the set's first received shred (which the
   caller has verified with Part 2c), and [0x40, 0x40 + P); an erased code
   slot d + i gets [0, 64) likewise, the header of fd_fec_resolver.c:515-524
   in [0x40, 0x59) -- variant 0x40 | depth; slot, version and fec_set_idx of
   the first received code shred; idx = that shred's idx - its code.idx + i;
   data_cnt d, code_cnt p, code.idx i -- and [0x59, 0x59 + P).  The proof
   bytes are Part 2f's; bytes beyond 1203 or 1228 of a larger slot are not
   written.

   Out of scope: the resolver's bookkeeping (the sets in progress,
   duplicates, eviction), a combined recover + tree + verify entry point,
   chained and resigned variants, and error correction, which the reference
   does not do either. */
#define FD_ED25519_HIP_FEC_ERR_PARTIAL (-23)   /* fewer shreds received than the set has data shreds */
#define FD_ED25519_HIP_FEC_ERR_CORRUPT (-24)   /* a received shred is not on the polynomial of the first d */

/* One set, host only (no GPU), from the same source as the device's kernel.
   Slots do not overlap; erased is cnt bytes.  Returns 0 with the set's
   erased slots written in place as said above, else the set's code with
   nothing written. */
int
fd_ed25519_hip_fec_recover( unsigned char *       shreds,
                            unsigned long const * shred_off,
                            unsigned int const *  shred_sz,
                            unsigned char const * erased,
                            unsigned long         cnt );

/* Device-resident batch: every pointer but the engine is a device pointer,
   with fd_ed25519_hip_fec_seal_dev's rules for them: slot i is
   shreds[shred_off[i] .. shred_off[i] + shred_sz[i]) and may start at any
   byte; slots do not overlap; the buffer starts 16-byte aligned and stays
   readable at least 16 bytes past the end of the last slot; erased is n
   bytes; set k is the slots [set_first[k], set_first[k+1]) in tree order,
   and a range that runs backwards or leaves [0, n) gets FEC_ERR_SET and
   touches nothing.  n < 2^32, n_set < 2^31.  set_out[k] receives the set's
   code.

   Asynchronous on `stream` (NULL: the engine's): one launch, whose tables
   the engine made when it was created; no workspace, no allocation, no
   synchronisation.  n_set==0 is a no-op. */
int
fd_ed25519_hip_fec_recover_dev( fd_ed25519_hip_engine_t * engine,
                                unsigned long             n,
                                unsigned char *           shreds,
                                unsigned long const *     shred_off,
                                unsigned int const *      shred_sz,
                                unsigned char const *     erased,
                                unsigned long             n_set,
                                unsigned int const *      set_first,
                                signed char *             set_out,
                                void *                    stream );

/* Host-buffer batch, synchronous: packs whole sets into pinned staging
   memory (in passes, so any n fits) -- a received shred travels whole, an
   erased slot as its size alone --, copies, runs fec_recover_dev and copies
   back set_out[0..n_set) and, into the caller's erased slots of every set
   with code 0, the bytes named above -- nothing else.  No alignment is asked
   of any argument. */
int
fd_ed25519_hip_fec_recover_host( fd_ed25519_hip_engine_t * engine,
                                 unsigned long             n,
                                 unsigned char *           shreds,
                                 unsigned long const *     shred_off,
                                 unsigned int const *      shred_sz,
                                 unsigned char const *     erased,
                                 unsigned long             n_set,
                                 unsigned int const *      set_first,
                                 signed char *             set_out );

/* ---- Part 2i: a block's proof-of-history hash chain ---------------------- */

/* What a validator does with the bytes that come out of its recovered FEC
   sets, beside verifying the transactions' signatures: the data shreds'
   payloads laid end to end are a block's entry batches, and every
   microblock's proof-of-history hash is checked (fd_runtime_block_verify /
   fd_runtime_poh_verify_wide_task, src/flamenco/runtime/fd_runtime.c:
   2007-2106).

   A microblock is given by offsets into one byte buffer buf[0, buf_sz): its
   48-byte header at hdr_off (hash_cnt u64 at 0x00, hash[32] at 0x08, txn_cnt
   u64 at 0x28, little-endian), the 32-byte state it starts from at in_off (a
   chained microblock's is its predecessor's hdr_off + 8; a block's first is
   wherever the caller put the parent's hash), and the 64-byte signatures of
   its transactions in transaction order at sig_off[sig_first[i] ..
   sig_first[i+1]).  Every field may stand at any byte address.

     txn_cnt == 0: k = hash_cnt, no mixin;
     txn_cnt  > 0: k = hash_cnt ? hash_cnt - 1 : 0, then a mixin (so hash_cnt
                   0 and 1 give the same result, as in the reference);
     state = in, k times state = SHA256( state ) (fd_poh_append), then the
     mixin state = SHA256( state || root ) (fd_poh_mixin), root the
     fd_wbmtree32 root over the signatures: leaf SHA256( 0x00 || sig ), node
     SHA256( 0x01 || left || right ), a layer of odd size duplicates its last
     node, a single leaf is the root (fd_bmtree_commit with 32-byte nodes and
     the 1-byte prefix gives the same root);
     0 if state equals the header's hash, else POH_ERR_HASH.

   POH_ERR_PARSE for a descriptor fd_runtime_block_prepare cannot produce: a
   signature range that runs backwards or leaves [0, n_sig), txn_cnt > 0 with
   no signatures, txn_cnt == 0 with some, an offset whose field leaves the
   buffer.  POH_UNSUPPORTED if k > hash_cnt_max.  Parse comes before
   unsupported, unsupported before hash.

   The bound is the one deliberate difference from the reference: hash_cnt is
   64 attacker-chosen bits and the reference would simply hash for years
   (its TODO about hashes_per_slot is the same gap).  Every entry point takes
   hash_cnt_max, at most FD_ED25519_HIP_POH_HASH_CNT_CEIL (above it the call
   is ERR_INVAL); a microblock over it is not hashed at all, and the kernel's
   loop bound is the minimum of k and hash_cnt_max besides, so no descriptor
   makes a launch longer than the ceiling allows.  fd_ed25519_hip_poh is a
   caller's CPU path for an UNSUPPORTED microblock it believes.

   One lane runs one chain: a lone microblock is far slower here than on a
   CPU core with SHA extensions.  The calls pay where many microblocks are
   verified together -- ledger replay, catch-up, repair of many slots
   (with the measurement).

   Out of scope: a deshredder, a combined PoH + signature-verify call, the
   tick-count and hashes_per_slot consensus checks, and a sub-wave tree for
   tiny microblocks. */
#define FD_ED25519_HIP_POH_ERR_PARSE     (-16)   /* a descriptor the block walk cannot produce */
#define FD_ED25519_HIP_POH_UNSUPPORTED   (-18)   /* more hashes than hash_cnt_max */
#define FD_ED25519_HIP_POH_ERR_HASH      (-25)   /* the computed state is not the header's hash */
#define FD_ED25519_HIP_POH_HASH_CNT_CEIL (1UL<<17)   /* twice a mainnet tick (62,500) */

/* The block walk, host only (no GPU): fd_runtime_block_prepare
   (fd_runtime.c:349-580) over one raw block -- batches until the buffer
   ends, each a u64 microblock_cnt and that many microblocks, each a header
   and txn_cnt transactions (fd_txn_parse_core's payload-size form on at
   most 1,232 of the bytes that remain).  Counts are believed only as far as
   bytes remain.  POH_ERR_PARSE: junk at the end, a short header, a failed
   transaction parse, and a batch with microblock_cnt == 0 (the reference's
   collect step reads microblock -1 of such a batch: undefined there,
   refused here).

   prepare_count returns 0 with the block's microblocks in *n and signatures
   in *n_sig, else POH_ERR_PARSE (both 0).  prepare fills hdr_off[n],
   in_off[n] (first_in_off for microblock 0, else the predecessor's hdr_off +
   8, across batch boundaries too), sig_first[n+1] and sig_off[n_sig], every
   offset relative to the block's first byte; n and n_sig are the capacities,
   and ERR_INVAL comes back if the block needs more of either. */
int
fd_ed25519_hip_poh_prepare_count( unsigned char const * block,
                                  unsigned long         block_sz,
                                  unsigned long *       n,
                                  unsigned long *       n_sig );

int
fd_ed25519_hip_poh_prepare( unsigned char const * block,
                            unsigned long         block_sz,
                            unsigned long         first_in_off,
                            unsigned long         n,
                            unsigned long         n_sig,
                            unsigned long *       hdr_off,
                            unsigned long *       in_off,
                            unsigned int *        sig_first,
                            unsigned long *       sig_off );

/* n microblocks, host only (no GPU), from the same rules as the device's
   kernels and the portable SHA-256 of fd_ed25519_hip_shred_root.  out[i]
   receives microblock i's code; out_hash (optional) its computed state at
   out_hash + 32 i, zeros for POH_ERR_PARSE and POH_UNSUPPORTED.  Returns
   ERR_INVAL for hash_cnt_max above the ceiling or a missing array. */
int
fd_ed25519_hip_poh( unsigned char const * buf,
                    unsigned long         buf_sz,
                    unsigned long         n,
                    unsigned long const * hdr_off,
                    unsigned long const * in_off,
                    unsigned int const *  sig_first,
                    unsigned long         n_sig,
                    unsigned long const * sig_off,
                    unsigned long         hash_cnt_max,
                    signed char *         out,
                    unsigned char *       out_hash );

/* Device workspace of poh_dev: a leaf hash per signature (32), which the
   tree reduces in place; per microblock its root (32) and one flag. */
#define FD_ED25519_HIP_POH_WORK_BYTES( n, n_sig ) \
  ( 32UL*(unsigned long)(n_sig) + 33UL*(unsigned long)(n) + 16UL )

/* Device-resident batch: every pointer but the engine is a device pointer.
   buf may start at any byte of a device allocation and must stay readable
   at least 16 bytes past buf + buf_sz; no alignment is asked of any field
   in it.  sig_first has n+1 elements; a sig_first that is not
   non-decreasing is survived (a range that runs backwards is
   POH_ERR_PARSE; microblocks whose ranges of more than 128 signatures
   overlap get an unspecified one of 0 and POH_ERR_HASH) and nothing is read
   or written outside the arrays.  out[i] receives the code; out_hash
   (optional, 16-byte aligned) the state as for fd_ed25519_hip_poh.  work:
   16-byte aligned, FD_ED25519_HIP_POH_WORK_BYTES( n, n_sig ) bytes.
   n < 2^31, n_sig < 2^32.

   Asynchronous on `stream` (NULL: the engine's): three launches (a lane per
   signature for the leaves, a wave per microblock for its tree, a lane per
   microblock for the chain; the chain alone when n_sig is 0); it allocates
   nothing and does not synchronise.  n==0 is a no-op. */
int
fd_ed25519_hip_poh_dev( fd_ed25519_hip_engine_t * engine,
                        unsigned long             n,
                        unsigned char const *     buf,
                        unsigned long             buf_sz,
                        unsigned long const *     hdr_off,
                        unsigned long const *     in_off,
                        unsigned int const *      sig_first,
                        unsigned long             n_sig,
                        unsigned long const *     sig_off,
                        unsigned long             hash_cnt_max,
                        signed char *             out,
                        unsigned char *           out_hash,
                        void *                    work,
                        void *                    stream );

/* Host-buffer batch, synchronous: orders the microblocks by descending k so
   that the lanes of a wave run alike, packs each one's header, in state and
   signatures into pinned staging memory (in passes, so any n fits), copies,
   runs poh_dev and returns out[0..n) and out_hash (optional, n x 32) in the
   caller's order.  A microblock with POH_ERR_PARSE is judged on the host
   and does not travel.  No alignment is asked of any argument. */
int
fd_ed25519_hip_poh_host( fd_ed25519_hip_engine_t * engine,
                         unsigned long             n,
                         unsigned char const *     buf,
                         unsigned long             buf_sz,
                         unsigned long const *     hdr_off,
                         unsigned long const *     in_off,
                         unsigned int const *      sig_first,
                         unsigned long             n_sig,
                         unsigned long const *     sig_off,
                         unsigned long             hash_cnt_max,
                         signed char *             out,
                         unsigned char *           out_hash );

/* nb raw blocks, block b the bytes blocks[block_off[b] .. block_off[b] +
   block_sz[b]) and in_hash + 32 b the hash its first microblock starts from:
   the walk, poh_host over the microblocks of every block that walked, and
   fd_runtime_block_verify_tpool's reduction.  block_out[b]: POH_ERR_PARSE if
   the walk failed or found no microblock (nothing of the block is verified);
   else POH_ERR_HASH if any microblock mismatched; else POH_UNSUPPORTED if any
   was over hash_cnt_max; else 0.  first_bad[b]: the block's first
   microblock with a nonzero code, 0xFFFFFFFF if none.  out_hash + 32 b: the
   last microblock's header hash (fd_runtime.c:2097), zeros for a block that
   did not walk.  Synchronous. */
int
fd_ed25519_hip_poh_blocks_host( fd_ed25519_hip_engine_t * engine,
                                unsigned long             nb,
                                unsigned char const *     blocks,
                                unsigned long const *     block_off,
                                unsigned long const *     block_sz,
                                unsigned char const *     in_hash,
                                unsigned long             hash_cnt_max,
                                signed char *             block_out,
                                unsigned int *            first_bad,
                                unsigned char *           out_hash );

/* ---- Part 2j: shredding entry batches ----------------------------------- */

/* The front of the leader's shred path: fd_shredder_init_batch and lines
   145-221 of fd_shredder_next_fec_set (src/disco/shred/fd_shredder.c) with
   the fd_shredder_count_* arithmetic (fd_shredder.h:116-145).  An entry
   batch goes in as its bytes; out come its data shreds and the headers of
   its parity shreds, laid out as Parts 2g and 2f take them, so that front,
   parity and seal are fd_shredder as a whole and only the batch bytes ever
   cross to the device.

   A batch of sz > 0 bytes becomes max( sz, 63679 ) / 31840 FEC sets.  Every
   set but the last takes 31,840 bytes as 32 data and 32 parity shreds; the
   last takes the r bytes that remain, 1 <= r <= 63679, as d data shreds --
   max( 1, ceil( r/1015 ) ) for r <= 9135, ceil( r/995 ) for r <= 31840,
   ceil( r/975 ) for r <= 62400, else ceil( r/955 ) -- and p parity shreds:
   the protocol's table of d (17 for 1 ... 32 for 32) in the first two cases,
   d in the last two.  With depth the proof depth of d + p shreds a data
   shred carries up to 1115 - 20 depth bytes, and only the batch's last data
   shred can carry fewer.

   With D the slot index of a set's first data shred and C that of its first
   parity shred -- the batch's data_idx and parity_idx plus the d and p of
   the sets before it, mod 2^32; the caller chains them over a slot's batches
   with shredder_count, which is what fd_shredder_skip_batch does --:
   data shred i has variant 0x80 | depth, slot, idx D + i, version,
   fec_set_idx D, parent_off, flags = reference_tick & 0x3f (on the set's last
   data shred also 0x40 when the set is the batch's last and 0x80 when
   besides block_complete & 1), size 0x58 + its bytes, the bytes at 0x58 and
   zeros up to 1203; parity shred j has variant 0x40 | depth, slot, idx
   C + j, version, fec_set_idx D, data_cnt d, code_cnt p, code.idx j.

   Written, exactly: of a data shred every byte [0, 1203), the signature and
   proof fields zero; of a parity shred [0, 0x59), the signature zero, and its
   proof field [1228 - 20 depth, 1228), zero.  The parity region [0x59,
   0x59 + P) is Part 2g's and is not touched; after parity and seal every
   byte of every shred is defined.  The leaf prefix the reference parks in
   the signature field on the way is overwritten by its own signature copy
   and is not reproduced.  Out of scope: the deshredder, chained and resigned
   variants, fusing the front into the parity kernel, fd_shred_dest. */
#define FD_ED25519_HIP_SHREDDER_OK              (  0)
#define FD_ED25519_HIP_SHREDDER_ERR_BATCH       (-19)   /* sz == 0, or a batch that leaves buf */
#define FD_ED25519_HIP_SHREDDER_BAD_RESERVATION (-17)   /* the reserved sets and shreds are not shredder_count's */

typedef struct {
  unsigned long  slot;
  unsigned int   data_idx;        /* slot index of the batch's first data shred */
  unsigned int   parity_idx;      /* ... and of its first parity shred */
  unsigned short version;
  unsigned short parent_off;
  unsigned char  reference_tick;
  unsigned char  block_complete;
  unsigned char  pad[ 2 ];
} fd_ed25519_hip_shredder_batch_t;   /* 24 bytes */

/* The sets, data shreds and parity shreds of a batch of sz bytes, host only
   (fd_shredder_count_fec_sets / _data_shreds / _parity_shreds); zeros for
   sz == 0.  Returns ERR_INVAL for a missing pointer. */
int
fd_ed25519_hip_shredder_count( unsigned long   sz,
                               unsigned long * n_set,
                               unsigned long * n_data,
                               unsigned long * n_parity );

/* One batch, host only (no GPU), from the same source as the device's
   kernel.  The caller gives shred_off[ i ] for the n_data + n_parity shreds
   of the batch, in tree order set by set; the call writes shred i at shreds +
   shred_off[ i ] as said above, shred_sz[ i ] (1203 or 1228) and set_first[ 0
   .. n_set ].  SHREDDER_ERR_BATCH for sz == 0, nothing written. */
int
fd_ed25519_hip_shredder( unsigned char const *                   batch,
                         unsigned long                           sz,
                         fd_ed25519_hip_shredder_batch_t const * desc,
                         unsigned char *                         shreds,
                         unsigned long const *                   shred_off,
                         unsigned int *                          shred_sz,
                         unsigned int *                          set_first );

/* Device-resident batches: every pointer but the engine is a device pointer.
   Batch b is buf[batch_off[b] .. batch_off[b] + batch_sz[b]) at any byte
   address; buf must stay readable 16 bytes past buf + buf_sz.  desc is 8-byte
   aligned.  The caller reserved, from shredder_count, the sets
   [set_first_b[b], set_first_b[b+1]) of the call's n_set and the shreds
   [shred_first_b[b], shred_first_b[b+1]) of its n for batch b (both arrays
   nb + 1 elements): sets in tree order, sets in batch order, batches in call
   order.  Shred i of the call is written at shreds + base_off + stride i,
   stride >= 1228, at any alignment, and no byte between shreds changes.  The
   call also writes shred_off[n] (base_off + stride i), shred_sz[n] and
   set_first[n_set + 1], so that fec_parity_dev and fec_seal_dev take the
   same arrays unchanged (their rules for the shred buffer hold: it starts
   16-byte aligned and stays readable 16 bytes past the last shred).
   n < 2^32, n_set < 2^31, nb < 2^31.

   batch_out[b] receives SHREDDER_ERR_BATCH for sz == 0 or a batch that
   leaves buf, else SHREDDER_BAD_RESERVATION for a reservation that runs
   backwards, leaves [0, n_set) or [0, n) or is not what shredder_count gives
   for batch_sz[b], else 0.  A batch with a code has no shred written, its
   shreds' shred_sz are 0 and their shred_off are left alone; of its reserved
   sets the first gets the whole shred reservation as its range and the
   others an empty one.  Parts 2g and 2f then give such a set a code without
   touching anything: FEC_ERR_SET for an empty range and for one of more
   than FEC_SET_MAX shreds, FEC_ERR_PARSE for the first set of a reservation
   of 1 to FEC_SET_MAX shreds (set_first is one array of boundaries, so a
   reservation between two good batches cannot vanish from it).  No other
   batch's result changes.  A set_first_b or shred_first_b that is no prefix
   sum is survived: nothing is read or written outside the arrays, a set no
   batch owns gets the range [n, ...), and a shred no set wrote has
   shred_sz 0.  Each batch is judged on its own range alone: reservations
   that are each what shredder_count gives but overlap (shred_first_b
   0, 18, 0, 18: the first and the third batch, of 1 byte each, both hold
   [0, 18)) all get code 0 and write the same shreds, whose bytes are then an unspecified mix of theirs -- in bounds,
   but no such set is fit to send.  Keeping ranges apart is the caller's.

   Asynchronous on `stream` (NULL: the engine's): one launch, behind a
   memset of shred_sz; no workspace, no allocation, no synchronisation.
   nb == 0 is a no-op. */
int
fd_ed25519_hip_shredder_front_dev( fd_ed25519_hip_engine_t *               engine,
                                   unsigned long                           nb,
                                   unsigned char const *                   buf,
                                   unsigned long                           buf_sz,
                                   unsigned long const *                   batch_off,
                                   unsigned int const *                    batch_sz,
                                   fd_ed25519_hip_shredder_batch_t const * desc,
                                   unsigned int const *                    set_first_b,
                                   unsigned int const *                    shred_first_b,
                                   unsigned long                           n_set,
                                   unsigned long                           n,
                                   unsigned char *                         shreds,
                                   unsigned long                           base_off,
                                   unsigned long                           stride,
                                   unsigned long *                         shred_off,
                                   unsigned int *                          shred_sz,
                                   unsigned int *                          set_first,
                                   signed char *                           batch_out,
                                   void *                                  stream );

/* Device workspace of shredder_dev: the seal's, a private key per set (32)
   and the parity's code per set (1). */
#define FD_ED25519_HIP_SHREDDER_WORK_BYTES( n, n_set ) \
  ( FD_ED25519_HIP_FEC_WORK_BYTES( n, n_set ) + 33UL*(unsigned long)(n_set) + 16UL )

/* Front, parity and seal on one stream: shredder_front_dev's arguments, then
   privs + 32 b, the private key that signs batch b's sets (the array 16-byte
   aligned; the front hands each set its batch's key), or NULL for the
   keyguard split of Part 2f; work, 16-byte aligned,
   FD_ED25519_HIP_SHREDDER_WORK_BYTES( n, n_set ) bytes; and the seal's
   set_out, roots and sigs.  Asynchronous, no allocation, no
   synchronisation. */
int
fd_ed25519_hip_shredder_dev( fd_ed25519_hip_engine_t *               engine,
                             unsigned long                           nb,
                             unsigned char const *                   buf,
                             unsigned long                           buf_sz,
                             unsigned long const *                   batch_off,
                             unsigned int const *                    batch_sz,
                             fd_ed25519_hip_shredder_batch_t const * desc,
                             unsigned int const *                    set_first_b,
                             unsigned int const *                    shred_first_b,
                             unsigned long                           n_set,
                             unsigned long                           n,
                             unsigned char *                         shreds,
                             unsigned long                           base_off,
                             unsigned long                           stride,
                             unsigned long *                         shred_off,
                             unsigned int *                          shred_sz,
                             unsigned int *                          set_first,
                             signed char *                           batch_out,
                             unsigned char const *                   privs,
                             void *                                  work,
                             signed char *                           set_out,
                             unsigned char *                         roots,
                             unsigned char *                         sigs,
                             void *                                  stream );

/* Host-buffer batches, synchronous, no alignment asked of any argument:
   batch b is batches[batch_off[b] .. + batch_sz[b]).  Only the batch bytes
   and the descriptors go up; the finished shreds, roots and signatures come
   down.  The call makes the reservation itself: shred i of the call, in
   tree order set by set, batch by batch, is written whole at shreds_out +
   stride i (stride >= 1228; bytes behind a data shred's 1203 are left
   alone), shred_sz_out[ i ] is 1203 or 1228, set_first_out has one element
   more than the call has sets, and batch_out[b] is 0, or SHREDDER_ERR_BATCH
   for sz == 0: such a batch takes no set and no shred, and a call of such
   batches alone returns 0 with set_first_out[0] == 0.  The parity's and the
   seal's codes of every set come down with the shreds and any of them fails
   the call (they are 0 on sets the front made).  privs as for shredder_dev (NULL: signature fields zero, sigs
   must be NULL); roots (32 a set) and sigs (64 a set) are optional.  It runs
   in passes cut at set boundaries (16,384 shreds a pass), so any nb and any
   batch size fit; a batch larger than a pass is continued in the next. */
int
fd_ed25519_hip_shredder_host( fd_ed25519_hip_engine_t *               engine,
                              unsigned long                           nb,
                              unsigned char const *                   batches,
                              unsigned long const *                   batch_off,
                              unsigned int const *                    batch_sz,
                              fd_ed25519_hip_shredder_batch_t const * desc,
                              unsigned char const *                   privs,
                              unsigned char *                         shreds_out,
                              unsigned long                           stride,
                              unsigned int *                          shred_sz_out,
                              unsigned int *                          set_first_out,
                              signed char *                           batch_out,
                              unsigned char *                         roots,
                              unsigned char *                         sigs );

/* ---- Part 3: batched signing and the synthetic workload generator ------ */

/* Batched fd_ed25519_public_from_private + fd_ed25519_sign on the device
   (src/ballet/ed25519/fd_ed25519_user.c:4-132): for each i, pubs[32 i..]
   and sigs[64 i..] receive the public key of privs[32 i..] and its
   signature of msgs[msg_off[i] .. + msg_sz[i]).  Device pointers; privs,
   sigs and pubs 16-byte aligned.  Async on `stream` (NULL = engine). */
int
fd_ed25519_hip_sign_dev( fd_ed25519_hip_engine_t * engine,
                         unsigned long             n,
                         unsigned char const *     msgs,
                         unsigned long const *     msg_off,
                         unsigned int const *      msg_sz,
                         unsigned char const *     privs,
                         unsigned char *           sigs,
                         unsigned char *           pubs,
                         void *                    stream );

/* Deterministic synthetic workload (bench.py): fills
   msgs[0..msg_bytes) with bytes derived from `seed`, derives the private
   key of signature g = index_base + i from (seed, g) and writes its public
   key and signature of message i.  Same (seed, g) -> same bytes on any GPU
   (firedancer_amd/workload.py recomputes them on the host). */
int
fd_ed25519_hip_gen_dev( fd_ed25519_hip_engine_t * engine,
                        unsigned long             n,
                        unsigned long             seed,
                        unsigned long             index_base,
                        unsigned char *           msgs,
                        unsigned long             msg_bytes,
                        unsigned long const *     msg_off,
                        unsigned int const *      msg_sz,
                        unsigned char *           sigs,
                        unsigned char *           pubs,
                        void *                    stream );

/* Corrupts about ppm/10^6 of the signatures in place with the invalid
   classes of SURVEY.md §8(d) C2 (bad S, small-order A/R, undecodable A/R,
   non-canonical A, flipped message bit); expect[i] (optional) receives the
   code the reference's AVX-512 build returns, cls[i] (optional) the class. */
int
fd_ed25519_hip_corrupt_dev( fd_ed25519_hip_engine_t * engine,
                            unsigned long             n,
                            unsigned long             seed,
                            unsigned long             index_base,
                            unsigned int              ppm,
                            unsigned char *           msgs,
                            unsigned long const *     msg_off,
                            unsigned int const *      msg_sz,
                            unsigned char *           sigs,
                            unsigned char *           pubs,
                            signed char *             expect,
                            unsigned char *           cls,
                            void *                    stream );

/* ---- Part 4: measurement and device-memory helpers ------------------ */

/* Phase timing: while enabled, fd_ed25519_hip_verify_dev brackets each of
   its phases (0 hash, 1 scalar, 2 decode, 3 dsm) with HIP events on the stream
   they run on (up to 256 chunk launches); _timing_read waits for them and
   returns the summed milliseconds per phase and the number of chunk
   launches, then resets.  Enabling resets too. */
#define FD_ED25519_HIP_PHASE_CNT (4)

int
fd_ed25519_hip_engine_timing( fd_ed25519_hip_engine_t * engine, int enable );

int
fd_ed25519_hip_engine_timing_read( fd_ed25519_hip_engine_t * engine,
                                   double * phase_ms /* [FD_ED25519_HIP_PHASE_CNT] */, unsigned long * launches );

/* The half-size form's base tables (generated on the device, shared by the
   engines of a device): table 0 holds [e]B, table 1 [e][2^SHIFT]B, for
   0 <= e < 2^BITS, as (y+x, y-x, 2dxy) in ten radix-2^25.5 limbs each.
   check_base_tables counts, per table (bad[2]: the full-length form's
   [0..2^15]B table), the entries e with entry e+1 != entry e + entry 1 (or
   entry 0 not the identity); together with a few
   entries compared against an independent [s]B (base_entry), a zero count
   proves the whole table.  base_entry copies entry `index` of table
   `which` (30 int32) to the host.  An engine with
   FD_ED25519_HIP_FLAG_COMPACT_TABLES has the 2^FD_ED25519_HIP_COMPACT_TABLE_BITS-entry
   pair instead. */
#define FD_ED25519_HIP_BASE_TABLE_BITS  24
#define FD_ED25519_HIP_COMPACT_TABLE_BITS 16
#define FD_ED25519_HIP_BASE_TABLE_SHIFT 144

int
fd_ed25519_hip_engine_check_base_tables( fd_ed25519_hip_engine_t * engine, unsigned long bad[3] );

int
fd_ed25519_hip_engine_base_entry( fd_ed25519_hip_engine_t * engine, int which, unsigned long index, int out[30] );

/* Device memory from the engine's HIP runtime (so callers need not link a
   second runtime).  memcpy is synchronous on the engine's stream. */
#define FD_ED25519_HIP_H2D (0)
#define FD_ED25519_HIP_D2H (1)
#define FD_ED25519_HIP_D2D (2)

void *
fd_ed25519_hip_dev_alloc( fd_ed25519_hip_engine_t * engine, unsigned long bytes );

int
fd_ed25519_hip_dev_free( fd_ed25519_hip_engine_t * engine, void * ptr );

int
fd_ed25519_hip_memcpy( fd_ed25519_hip_engine_t * engine, void * dst, void const * src, unsigned long bytes, int dir );

/* Number of visible HIP devices (0 if none / no driver). */
int
fd_ed25519_hip_device_count( void );

/* Peak shader clock of the engine's device in MHz (hipDeviceProp clockRate). */
int
fd_ed25519_hip_device_clock_mhz( fd_ed25519_hip_engine_t * engine );

/* Waits for all work enqueued on the engine's stream -- which other
   engines of the device may share (fd_ed25519_hip_engine_stream). */
int
fd_ed25519_hip_engine_sync( fd_ed25519_hip_engine_t * engine );

/* Diagnostic: the verify kernels' half-size scalar search
   (csrc/fd25519_half.h) run on the device for n scalars k (8 little-endian
   32-bit words each, k < L), host buffers in and out.  out[12*i]: 1 if a
   pair was found, out[12*i+1]: d < 0, out[12*i+2..6]: c, out[12*i+7..11]:
   |d| (5 words each).  Synchronous.  For tests: the device search must
   agree with the host build of the same header. */
int
fd_ed25519_hip_diag_half_scalars( fd_ed25519_hip_engine_t * engine,
                                  unsigned int const *      k,
                                  unsigned long             n,
                                  unsigned int *            out );

/* Human-readable form of an engine status code / of the last failure. */
char const *
fd_ed25519_hip_strerror( int status );

char const *
fd_ed25519_hip_last_error( void );

#ifdef __cplusplus
}
#endif

#endif /* HEADER_fd_ed25519_hip_h */
