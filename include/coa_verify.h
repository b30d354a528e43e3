/*
 * coa_verify.h -- C ABI of the MI355X (gfx950) ed25519 / SHA-512 verification
 * engine for the Narwhal/Tusk fork pwang200/xrpl-coa-prototype.
 *
 * This is the drop-in boundary for the reference's `crypto` crate hot path.
 * Every entry point names the reference interface it replaces.  Plain
 * pointers and sizes only: no HIP or torch types in the signatures (device
 * streams are passed as `void*` = hipStream_t).
 *
 * Conventions
 *   - Verdict bytes: 0 = Ok, 1 = Err (the reference's Result<(), CryptoError>;
 *     CryptoError = ed25519::Error is opaque, crypto/src/lib.rs:18, so callers
 *     only branch Ok/Err -- primary/src/error.rs:28 maps it to
 *     DagError::InvalidSignature).
 *   - Return codes: COA_OK (0) / COA_REJECT (1) for single verdicts; COA_OK for
 *     a completed many-call; a negative COA_E* on internal failure.  There is
 *     NO implicit CPU fallback: with no usable GPU every GPU call returns
 *     COA_ENODEVICE.  The engine's own CPU path (coa_cpu_*, below) answers
 *     only when a caller calls it explicitly.
 *   - Host-pointer calls: inputs are caller-owned and only read during the
 *     call; outputs are caller-allocated.  Nothing is retained after return.
 *   - Thread safety: every call takes the engine lock of the devices it uses;
 *     calls from several threads are serialised per device.
 *   - Multi-GPU: host-pointer "many" calls shard items by contiguous index
 *     range over the devices opened by coa_init (no cross-GPU exchange).
 */
#ifndef COA_VERIFY_H
#define COA_VERIFY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COA_OK 0
#define COA_REJECT 1
#define COA_EINVAL (-1)
#define COA_ENODEVICE (-2)
#define COA_EHIP (-3)
#define COA_ENOMEM (-4)

/* ---------------------------------------------------------------- lifecycle
 * No reference counterpart (dalek is stateless).  Opens `n_gpus` devices
 * (0 = all visible), builds the fixed-base tables on each.  Idempotent; the
 * other calls initialise lazily with n_gpus = 0 when it was not called. */
int coa_init(int n_gpus);
/* Opens exactly the listed HIP devices (one process per GPU: each rank opens
 * its own).  Idempotent like coa_init; host-pointer calls shard over the
 * opened devices in list order. */
int coa_init_devices(const int* device_ids, int n);
int coa_shutdown(void);
int coa_device_count(void);
/* HIP device id of each opened context, in the order host-pointer calls
 * shard over them (a device opened k times appears k times).  Returns the
 * number of contexts; copies min(count, cap) ids. */
int coa_device_ids(int* ids_out, int cap);
/* Self-test of device `device`'s fixed-base tables (no reference
 * counterpart): checks every entry of the wide HBM comb of B against its
 * neighbours (m*2^(Wj)*B = (m-1)*2^(Wj)*B + 2^(Wj)*B, 2^(W(j+1))*B =
 * [2^W] 2^(Wj)*B, entry (0,1) = B, canonical encodings).  *bad_entries gets
 * the number of failing entries (0 when the table is absent: COA_WCOMB=0). */
int coa_self_test(int device, uint64_t* bad_entries);
/* Self-test of the row-parallel field arithmetic (no reference counterpart):
 * for each of the n 32-byte values d_in[i] (device memory, any value below
 * 2^256) compares, on the device, the 16-lane-row versions of z^((p-5)/8),
 * z^(p-2), z * d_in[i+1], z + d_in[i+1], z - d_in[i+1] and decompression (of
 * d_in[i] as an encoding) with
 * the one-lane versions.  d_out[i] (uint32) gets a bit per mismatch: 0 = agree.
 * stream NULL = the engine's stream (the call then waits). */
int coa_fe_rows_check_device(int device, const uint8_t* d_in, size_t n, uint32_t* d_out, void* stream);
/* Human-readable description of the last error on this thread. */
const char* coa_last_error(void);
/* Engine-failure recovery of the host-pointer calls since the library
 * loaded (no reference counterpart: dalek cannot fail for a reason other
 * than the input).  A shard whose device work fails (a HIP error or an
 * allocation failure) has its context rebuilt -- a new stream, per-call
 * buffers released, in the same process -- and is re-run on the next
 * contexts in turn; the call returns an error only when every context
 * failed it.  *contexts_rebuilt / *shards_rerun (either may be NULL) get the
 * counts.  The aggregation queue counts its own in coa_queue_metrics. */
int coa_engine_recoveries(uint64_t* contexts_rebuilt, uint64_t* shards_rerun);
/* Library / ABI version string. */
const char* coa_version(void);

/* ------------------------------------------------------- Signature::verify
 * Replaces crypto::Signature::verify (crypto/src/lib.rs:200-204):
 *   ed25519::Signature::from_bytes(sig)            (:201)
 *   ed25519_dalek::PublicKey::from_bytes(pk)       (:202)
 *   PublicKey::verify_strict(msg, sig)             (:203)
 * called by Header::verify (primary/src/messages.rs:64-66) and Vote::verify
 * (primary/src/messages.rs:139-141).  msg is the 32-byte Digest.
 * Returns COA_OK, COA_REJECT or a negative error (latency path). */
int coa_ed25519_verify_strict(const uint8_t msg[32], const uint8_t pk[32], const uint8_t sig[64]);

/* n independent (msg, pk, sig) triples; msgs are n * msg_len bytes (msg_len
 * 32 for the crypto API, any length supported), pks n * 32, sigs n * 64
 * (R || s).  verdicts_out[i] = 0 Ok / 1 Err.  Sharded over all devices. */
int coa_ed25519_verify_strict_many(const uint8_t* msgs, size_t msg_len, const uint8_t* pks, const uint8_t* sigs,
                                   size_t n, uint8_t* verdicts_out);

/* Same, with every buffer already resident in the HBM of `device` and the
 * work enqueued on `stream` (hipStream_t; NULL = the engine's stream for that
 * device).  Asynchronous: returns after enqueue.  `workspace` may be NULL
 * (engine-owned) -- otherwise at least coa_verify_workspace_bytes(n) bytes of
 * device memory on `device`. */
size_t coa_verify_workspace_bytes(size_t n);
int coa_ed25519_verify_strict_many_device(int device, const uint8_t* d_msgs, size_t msg_len, const uint8_t* d_pks,
                                          const uint8_t* d_sigs, size_t n, uint8_t* d_verdicts, void* workspace,
                                          void* stream);

/* The two device stages of the call above, for callers that already hold k
 * (e.g. a digest stage fused upstream) and for per-kernel timing:
 *   challenge:  d_k_out[i] = SHA-512(R_i || A_i || M_i) mod l, 32 bytes LE
 *               (Scalar::from_hash inside dalek verify_strict)
 *   prehashed:  verdicts from (k, A, R || s); workspace as above (may be NULL). */
int coa_ed25519_challenge_many_device(int device, const uint8_t* d_msgs, size_t msg_len, const uint8_t* d_pks,
                                      const uint8_t* d_sigs, size_t n, uint8_t* d_k_out, void* stream);
int coa_ed25519_verify_prehashed_many_device(int device, const uint8_t* d_k, const uint8_t* d_pks,
                                             const uint8_t* d_sigs, size_t n, uint8_t* d_verdicts, void* workspace,
                                             void* stream);

/* ------------------------------------------------- Signature::verify_batch
 * Replaces crypto::Signature::verify_batch (crypto/src/lib.rs:206-219) ->
 * ed25519_dalek::verify_batch (:218), called by Certificate::verify
 * (primary/src/messages.rs:214).  One group = one certificate: all its votes
 * sign the same 32-byte digest.
 *   msgs           n_groups * 32 bytes
 *   pks, sigs      concatenated votes, group g = [group_offsets[g], group_offsets[g+1])
 *   group_offsets  n_groups + 1 entries, group_offsets[0] = 0
 *   group_verdicts_out[g] = 0 Ok / 1 Err
 * The 128-bit random weights z_i are derived from rng_seed (0 = fresh OS
 * entropy per call, the dalek behaviour; any other value is reproducible).
 * Ok iff every s_i < l, every A_i and R_i decompresses and the random linear
 * combination is the identity -- no small-order rejection, no cofactor,
 * exactly dalek 1.0.1. */
int coa_ed25519_verify_batch(const uint8_t msg[32], const uint8_t* pks, const uint8_t* sigs, size_t n,
                             uint64_t rng_seed);
int coa_ed25519_verify_batch_groups(const uint8_t* msgs, const uint8_t* pks, const uint8_t* sigs,
                                    const uint64_t* group_offsets, size_t n_groups, uint8_t* group_verdicts_out,
                                    uint64_t rng_seed);
/* Parity-test form: the z_i are given explicitly (16 little-endian bytes per
 * signature, in the order of pks/sigs). */
int coa_ed25519_verify_batch_groups_z(const uint8_t* msgs, const uint8_t* pks, const uint8_t* sigs,
                                      const uint64_t* group_offsets, size_t n_groups, const uint8_t* zs,
                                      uint8_t* group_verdicts_out);

/* Pippenger form of the call above for ONE group whose buffers are resident
 * in the HBM of `device` (dalek's verify_batch switches to Pippenger above
 * 190 points; the host-pointer entries above route here the groups of a
 * call with one or two groups, and groups of at least COA_MSM_MIN
 * signatures, default 16384).
 *   d_msg        32 bytes, the digest every signature signs
 *   d_pks        n * 32, d_sigs n * 64
 *   d_zs         n * 16 explicit weights (parity tests) or NULL = derived
 *                from rng_seed (0 = fresh OS entropy)
 *   *d_verdict   0 Ok / 1 Err, same rules as coa_ed25519_verify_batch
 * `workspace` NULL = engine-owned (the call then waits for the stream), else
 * `workspace_bytes` bytes on `device`, at least
 * coa_verify_batch_workspace_bytes(n) evaluated under the same environment
 * (COA_MSM_RUN changes the layout); a smaller buffer is refused with
 * COA_EINVAL.  With a workspace the call only enqueues. */
size_t coa_verify_batch_workspace_bytes(size_t n);
int coa_ed25519_verify_batch_device(int device, const uint8_t* d_msg, const uint8_t* d_pks, const uint8_t* d_sigs,
                                    size_t n, const uint8_t* d_zs, uint64_t rng_seed, uint8_t* d_verdict,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ Digest
 * Replaces Sha512::digest at worker/src/processor.rs:38 (500 KB batch
 * digests) and the Header/Vote/Certificate digests
 * (primary/src/messages.rs:70-84,145-153,226-234).  Message i is
 * data[offsets[i] .. offsets[i+1]); offsets has n + 1 entries.
 * coa_sha512_many writes 64 bytes per message, coa_sha512_trunc32_many the
 * 32-byte crypto::Digest prefix. */
int coa_sha512_many(const uint8_t* data, const uint64_t* offsets, size_t n, uint8_t* out64);
int coa_sha512_trunc32_many(const uint8_t* data, const uint64_t* offsets, size_t n, uint8_t* out32);
int coa_sha512_many_device(int device, const uint8_t* d_data, const uint64_t* d_offsets, size_t n, uint8_t* d_out64,
                           void* stream);

/* ------------------------------------------------ committee key cache (f2)
 * No reference counterpart: the reference decompresses every voter key on
 * every call (crypto/src/lib.rs:202,216) although the keys are fixed per
 * config::Committee (config/src/lib.rs:140-143, loaded once in
 * node/src/main.rs).  Registers the committee's n public keys (32 B each;
 * duplicates collapse) on every device: decompression verdict, small-order
 * and torsion flags and a 384 KiB comb of -A per key, so certificate checks
 * need no doubling.  Replaces any previous committee; n = 0 clears it.
 * Verdict-neutral: keys outside the committee still verify, through the
 * uncached kernels.  Returns the number of distinct keys registered or a
 * negative error. */
int coa_committee_register(const uint8_t* pks, size_t n);
/* Key flags of the registered committee in its internal (sorted) order:
 * bit0 decompresses, bit1 small order, bit2 torsion free.  Returns the
 * committee size; copies min(size, cap) words.  Diagnostics / tests. */
int coa_committee_key_flags(uint32_t* flags_out, size_t cap);

/* --------------------------------------- Certificate::verify crypto (f3)
 * The crypto of Certificate::verify (primary/src/messages.rs:189-215) in one
 * fused launch for registered committees:
 *   COA_CERT_BAD_HEADER_ID   SHA-512(header digest bytes)[..32] != header.id
 *                            (Header::verify, messages.rs:49-51; the bytes are
 *                            Header::digest's input, messages.rs:70-84)
 *   COA_CERT_BAD_HEADER_SIG  Signature::verify(header.id, author) fails
 *                            (messages.rs:64-66, dalek verify_strict)
 *   COA_CERT_BAD_VOTES       Signature::verify_batch(Certificate::digest,
 *                            votes) fails (messages.rs:214; the digest is
 *                            SHA-512(id || round u64 LE || origin)[..32],
 *                            messages.rs:226-234, computed on the device)
 * These calls leave the non-crypto checks (genesis, stake, worker ids,
 * quorum) to the caller, which applies them in the reference's order with
 * these bits; coa_certificate_verdict_many below decides them too
 * (INTEGRATION.md).  Votes are checked per signature with the committee
 * combs; when every vote holds its own cofactorless equation and every key is
 * torsion free, dalek's batch verdict is Ok for any weights.  Any other
 * well-formed outcome is re-decided by the exact random-linear-combination
 * kernels (weights from rng_seed, 0 = OS entropy, as verify_batch), and
 * certificates with keys outside the committee take the uncached kernels:
 * the verdict is always dalek's.
 *   header_data/header_offsets  n + 1 offsets into the concatenated headers
 *   ids, origins                n * 32 (header.id, header.author)
 *   header_sigs                 n * 64;  rounds: n
 *   vote_pks, vote_sigs         concatenated votes; certificate c owns
 *                               [vote_offsets[c], vote_offsets[c+1])
 *   status_out[c]               0 = all crypto Ok, else COA_CERT_* bits */
#define COA_CERT_BAD_HEADER_ID 1
#define COA_CERT_BAD_HEADER_SIG 2
#define COA_CERT_BAD_VOTES 4
int coa_certificate_verify_many(const uint8_t* header_data, const uint64_t* header_offsets, const uint8_t* ids,
                                const uint8_t* origins, const uint8_t* header_sigs, const uint64_t* rounds,
                                const uint8_t* vote_pks, const uint8_t* vote_sigs, const uint64_t* vote_offsets,
                                size_t n, uint64_t rng_seed, uint8_t* status_out);
/* One certificate (the latency path: one H2D, one launch with one wavefront
 * per signature, one D2H).  Returns the COA_CERT_* bits (>= 0) or a negative
 * error. */
int coa_certificate_verify(const uint8_t* header_data, size_t header_len, const uint8_t id[32],
                           const uint8_t origin[32], const uint8_t header_sig[64], uint64_t round,
                           const uint8_t* vote_pks, const uint8_t* vote_sigs, size_t n_votes, uint64_t rng_seed);
/* Device-resident form (asynchronous on `stream`): d_status[c] receives the
 * raw status word -- COA_CERT_* bits plus 8 = votes need the exact RLC check
 * (coa_ed25519_verify_batch_groups) and 16 = a key is not registered (use the
 * uncached entry points).  The host-pointer calls above resolve both.
 * `workspace`: NULL (engine-owned; the call then waits for its stream) or
 * coa_certificate_workspace_bytes(n, n_votes) bytes of device memory.  A
 * call of >= 16,384 jobs (certificates + votes) takes its jobs in committee-key
 * order, and the size then includes the sort's area (~4.2 MB + 8 B per job). */
size_t coa_certificate_workspace_bytes(size_t n, size_t n_votes);
int coa_certificate_verify_many_device(int device, const uint8_t* d_header_data, const uint64_t* d_header_offsets,
                                       const uint8_t* d_ids, const uint8_t* d_origins, const uint8_t* d_header_sigs,
                                       const uint64_t* d_rounds, const uint8_t* d_vote_pks,
                                       const uint8_t* d_vote_sigs, const uint64_t* d_vote_offsets, size_t n,
                                       size_t n_votes, uint32_t* d_status, void* workspace, void* stream);

/* ------------------------------- Header::verify / Vote::verify crypto
 * The crypto of Header::verify (primary/src/messages.rs:48-67: the digest
 * check :49-51 and Signature::verify(header.id, author) :64-66) and of
 * Vote::verify (:131-142: Signature::verify(Vote::digest, author) :139-141,
 * Vote::digest = SHA-512(id || round u64 LE || origin)[..32], :145-153) for
 * many messages in ONE launch with the registered committee's key combs (no
 * doubling, no decompression of A or R).  The reference checks
 * committee.stake(author) > 0 before either signature, so every signature
 * that matters is by a registered key; the others are re-decided through the
 * uncached entry points (SHA-512 + coa_ed25519_verify_strict_many), so the
 * answer is always dalek's verify_strict, registered or not, and with no
 * committee registered every item takes that route.  The non-crypto checks
 * (stake, worker ids, round) stay with the caller.
 * The arrays are what coa_wire_decode_headers / coa_wire_decode_votes fill:
 *   header_data/header_offsets  n + 1 offsets into the concatenated
 *                               Header::digest inputs
 *   ids, authors                n * 32;  sigs n * 64 (R || s)
 *   rounds, origins             n, n * 32 (votes: the voted header's round
 *                               and author)
 *   status_out[i]   (headers)   0, or COA_CERT_BAD_HEADER_ID |
 *                               COA_CERT_BAD_HEADER_SIG
 *   verdicts_out[i] (votes)     0 Ok / 1 Err
 * Host forms shard by contiguous index range over the opened devices; n = 0
 * returns COA_OK. */
int coa_header_verify_many(const uint8_t* header_data, const uint64_t* header_offsets, const uint8_t* ids,
                           const uint8_t* authors, const uint8_t* sigs, size_t n, uint8_t* status_out);
int coa_vote_verify_many(const uint8_t* ids, const uint64_t* rounds, const uint8_t* origins, const uint8_t* authors,
                         const uint8_t* sigs, size_t n, uint8_t* verdicts_out);
/* Device-resident forms (asynchronous on `stream`; NULL = the engine's
 * stream): d_status[i], zeroed by the call, receives the raw word -- bit 1
 * (headers) the digest differs from ids[i], bit 2 the signature fails
 * verify_strict, bit 16 the author is not registered and nothing else was
 * decided for the item (use the uncached entry points).  `workspace`: NULL
 * (engine-owned; the call then waits for its stream) or at least
 * coa_message_workspace_bytes(n) bytes of device memory. */
size_t coa_message_workspace_bytes(size_t n);
int coa_header_verify_many_device(int device, const uint8_t* d_header_data, const uint64_t* d_header_offsets,
                                  const uint8_t* d_ids, const uint8_t* d_authors, const uint8_t* d_sigs, size_t n,
                                  uint32_t* d_status, void* workspace, void* stream);
int coa_vote_verify_many_device(int device, const uint8_t* d_ids, const uint64_t* d_rounds, const uint8_t* d_origins,
                                const uint8_t* d_authors, const uint8_t* d_sigs, size_t n, uint32_t* d_status,
                                void* workspace, void* stream);

/* ------------- Certificate::verify / Header::verify / Vote::verify verdicts
 * The whole of Certificate::verify (primary/src/messages.rs:189-215),
 * Header::verify (:48-67) and Vote::verify (:131-142) decided by the engine:
 * the crypto bits of the calls above merged on the device with the protocol
 * checks (genesis, stake, worker ids, reuse, quorum) in the reference's
 * order, so a caller gets the reference's DagResult as one word per item
 * instead of interleaving bits and checks itself.
 *
 * coa_committee_register_authorities mirrors config::Committee
 * (config/src/lib.rs:130-143; Stake and WorkerId are u32): authority i has
 * key pks[32 i ..], stake stakes[i] and the worker ids
 * worker_ids[worker_offsets[i] .. worker_offsets[i+1]).  It does everything
 * coa_committee_register does and builds, in the same key-cache generation,
 * the protocol table the verdict calls read: stakes and sorted worker ids in
 * the engine's key order, and quorum = 2 * total / 3 + 1
 * (Committee::quorum_threshold, config/src/lib.rs:168-173).  A call or queue
 * window that pinned a generation reads that generation's stakes.  Rejected
 * with COA_EINVAL (text in coa_last_error): duplicate keys (a BTreeMap holds
 * none), a total stake of 2^31 or more (the reference's 2 * total_votes
 * overflows there), more than COA_MAX_AUTHORITIES keys (the reuse table of
 * the certificate kernel is COA_MAX_AUTHORITIES words of LDS per wavefront).
 * Stake 0 is legal: the key is cached, and the reference answers
 * UnknownAuthority for it.  Returns the number of keys or a negative error.
 * After plain coa_committee_register the generation has no protocol table
 * and the verdict calls return COA_EINVAL. */
#define COA_MAX_AUTHORITIES 1024
int coa_committee_register_authorities(const uint8_t* pks, const uint32_t* stakes, const uint32_t* worker_ids,
                                       const uint64_t* worker_offsets, size_t n);
/* A verdict is a uint32_t: bits 0-7 the code, the first check of the
 * reference that fails; for COA_DAG_AUTHORITY_REUSE and COA_DAG_UNKNOWN_VOTER
 * bits 8-31 hold the index of the offending vote within its certificate (the
 * key the reference's error names). */
#define COA_DAG_OK 0                /* Ok; also genesis, messages.rs:190-193 */
#define COA_DAG_INVALID_HEADER_ID 1 /* messages.rs:50 */
#define COA_DAG_UNKNOWN_AUTHOR 2    /* :53-54, :133-136: the author's stake is 0 */
#define COA_DAG_MALFORMED_HEADER 3  /* :57-61: a worker id the author does not have */
#define COA_DAG_INVALID_SIGNATURE 4 /* :64-66, :139-141 */
#define COA_DAG_AUTHORITY_REUSE 5   /* :202 */
#define COA_DAG_UNKNOWN_VOTER 6     /* :203-204 */
#define COA_DAG_REQUIRES_QUORUM 7   /* :208-211 */
#define COA_DAG_INVALID_VOTES 8     /* :214 */
#define COA_DAG_VOTES_OPEN 9        /* device-resident form only: every earlier check passed and the votes need
                                       the exact check, as raw status bit 8: coa_certificate_votes_resolve_device
                                       decides it on the device (or coa_ed25519_verify_batch_groups on the host) */
#define COA_DAG_CODE(v) ((v) & 0xffu)
#define COA_DAG_VOTE_INDEX(v) ((v) >> 8)
/* Semantics, exactly the reference's:
 *   - genesis (:190-193): id is 32 zero bytes, round 0 and origin a MEMBER of
 *     the committee, whatever its stake (Certificate::genesis iterates
 *     authorities.keys(); PartialEq, :249-256, compares id, round and origin
 *     only) is COA_DAG_OK whatever else the certificate holds;
 *   - the vote loop (:201-207) reports the first failing vote in vote order,
 *     reuse tested before stake at each vote; the weight is summed in 64 bits;
 *   - worker id k of a header is the u32 LE at byte 40 + 36 k + 32 of its
 *     digest input; payload_counts[i] (what the wire decoders fill) is the
 *     number of payload entries.  A count that overruns its header is
 *     COA_EINVAL for a host-pointer call; the device-resident forms, which
 *     cannot see it before they return, answer COA_DAG_MALFORMED_HEADER.
 * Host-pointer forms: the arguments of coa_certificate_verify_many /
 * coa_header_verify_many / coa_vote_verify_many plus payload_counts; sharded
 * by index range like them.  COA_DAG_VOTES_OPEN is resolved through the exact
 * path (rng_seed as there); nothing else goes to a resolver: an item whose
 * author or voter is outside the committee is answered by the protocol word
 * alone. */
int coa_certificate_verdict_many(const uint8_t* header_data, const uint64_t* header_offsets, const uint8_t* ids,
                                 const uint8_t* origins, const uint8_t* header_sigs, const uint64_t* rounds,
                                 const uint8_t* vote_pks, const uint8_t* vote_sigs, const uint64_t* vote_offsets,
                                 size_t n, uint64_t rng_seed, const uint32_t* payload_counts,
                                 uint32_t* verdicts_out);
int coa_header_verdict_many(const uint8_t* header_data, const uint64_t* header_offsets, const uint8_t* ids,
                            const uint8_t* authors, const uint8_t* sigs, size_t n, const uint32_t* payload_counts,
                            uint32_t* verdicts_out);
int coa_vote_verdict_many(const uint8_t* ids, const uint64_t* rounds, const uint8_t* origins, const uint8_t* authors,
                          const uint8_t* sigs, size_t n, uint32_t* verdicts_out);
/* Device-resident forms (asynchronous on `stream`; NULL = the engine's
 * stream): the crypto launch of the *_verify_many_device call, the protocol
 * kernel and the merge, all on `stream`.  d_verdicts[c] may hold
 * COA_DAG_VOTES_OPEN (coa_certificate_votes_resolve_device closes it).
 * `workspace`: NULL (engine-owned; the call then waits for its stream) or at
 * least coa_*_verdict_workspace_bytes bytes of device memory (the crypto
 * call's workspace plus two words per item). */
size_t coa_certificate_verdict_workspace_bytes(size_t n, size_t n_votes);
int coa_certificate_verdict_many_device(int device, const uint8_t* d_header_data, const uint64_t* d_header_offsets,
                                        const uint8_t* d_ids, const uint8_t* d_origins, const uint8_t* d_header_sigs,
                                        const uint64_t* d_rounds, const uint8_t* d_vote_pks,
                                        const uint8_t* d_vote_sigs, const uint64_t* d_vote_offsets, size_t n,
                                        size_t n_votes, const uint32_t* d_payload_counts, uint32_t* d_verdicts,
                                        void* workspace, void* stream);
/* Closes the COA_DAG_VOTES_OPEN words of coa_certificate_verdict_many_device
 * on the device, so a device-resident caller gets the whole of
 * Certificate::verify without a copy to the host.  The arrays are that call's;
 * d_verdicts holds its output and is updated in place: every word whose code
 * is COA_DAG_VOTES_OPEN becomes COA_DAG_OK or COA_DAG_INVALID_VOTES -- exactly
 * what dalek 1.0.1 verify_batch answers over (Certificate::digest, votes) with
 * the weights below -- and every other word stays bit for bit.  The call reads
 * no key cache and needs no registered committee: it is a pure function of its
 * arguments (the exact random-linear-combination kernels over the open
 * certificates' votes, found, compacted and counted on the device).
 *   open_votes_cap  the most open votes the call resolves (0 = n_votes); it
 *                   sizes the workspace (the term's scratch is 2 KiB per lane,
 *                   up to 131,072 lanes).  Open certificates are taken in
 *                   ascending index order while the votes of all of them so
 *                   far fit; from the first that does not fit on they keep
 *                   COA_DAG_VOTES_OPEN, and a further call resolves them (a
 *                   certificate with more votes than the cap never fits it).
 *   d_zs            n_votes * 16 explicit weights, indexed by a vote's position
 *                   in d_vote_pks / d_vote_sigs (the parity form of
 *                   coa_cpu_certificate_verify_many_z), or NULL: derived on the
 *                   device from rng_seed (0 = fresh OS entropy per call, drawn
 *                   on the host) by coa_ed25519_verify_batch's block with the
 *                   certificate's index as the group and the vote's position
 *                   in the call as i -- independent of which other
 *                   certificates are open and of open_votes_cap
 *   d_counts        NULL, or three words: open certificates found, open
 *                   certificates resolved, open votes resolved
 * `workspace`: at least coa_certificate_votes_resolve_workspace_bytes(n,
 * n_votes, open_votes_cap) bytes of device memory -- the call then only
 * enqueues on `stream` (no host synchronisation, no copy, no allocation) -- or
 * NULL: engine-owned, and the call waits for its stream.  n = 0 returns
 * COA_OK; a null array COA_EINVAL. */
size_t coa_certificate_votes_resolve_workspace_bytes(size_t n, size_t n_votes, size_t open_votes_cap);
int coa_certificate_votes_resolve_device(int device, const uint8_t* d_ids, const uint8_t* d_origins,
                                         const uint64_t* d_rounds, const uint8_t* d_vote_pks,
                                         const uint8_t* d_vote_sigs, const uint64_t* d_vote_offsets, size_t n,
                                         size_t n_votes, size_t open_votes_cap, const uint8_t* d_zs, uint64_t rng_seed,
                                         uint32_t* d_verdicts, uint32_t* d_counts, void* workspace, void* stream);
size_t coa_message_verdict_workspace_bytes(size_t n);
int coa_header_verdict_many_device(int device, const uint8_t* d_header_data, const uint64_t* d_header_offsets,
                                   const uint8_t* d_ids, const uint8_t* d_authors, const uint8_t* d_sigs, size_t n,
                                   const uint32_t* d_payload_counts, uint32_t* d_verdicts, void* workspace,
                                   void* stream);
int coa_vote_verdict_many_device(int device, const uint8_t* d_ids, const uint64_t* d_rounds, const uint8_t* d_origins,
                                 const uint8_t* d_authors, const uint8_t* d_sigs, size_t n, uint32_t* d_verdicts,
                                 void* workspace, void* stream);

/* ------------------------------------------------------- wire decode (f4)
 * bincode 1.3 decode of PrimaryMessage frames, as
 * PrimaryReceiverHandler::dispatch does (primary/src/primary.rs:223-244),
 * straight into the arrays of the batched entry points above.  Host-only
 * parsing (no device work).  frames[frame_offsets[i] .. frame_offsets[i+1])
 * is frame i.
 *   coa_wire_scan: kind_out[i] = COA_MSG_* or a negative COA_WIRE_E* (the
 *     reference drops such frames); header_bytes_out[i] = length of the
 *     Header::digest input (Header and Certificate frames), votes_out[i] =
 *     number of votes (Certificate frames); both optional.
 *   coa_wire_decode_certificates: every frame must be a Certificate; fills
 *     the coa_certificate_verify_many arguments (header_data sized by the
 *     scan's header bytes, vote arrays by its vote counts); payload_counts
 *     (optional) = entries of header.payload, whose worker ids sit at
 *     header_data + 40 + 36 k + 32 (the MalformedHeader check).
 *   coa_wire_decode_votes / _headers: Vote / Header frames (Vote::digest
 *     input = id || round LE || origin; Header::digest input as above).
 * Header::digest input = author | round LE | (digest | worker id LE)* in key
 * order | parents* in order (primary/src/messages.rs:70-84). */
#define COA_MSG_HEADER 0
#define COA_MSG_VOTE 1
#define COA_MSG_CERTIFICATE 2
#define COA_MSG_CERT_REQUEST 3
#define COA_WIRE_ETRUNC (-10)  /* frame ends inside a field / length prefix too large */
#define COA_WIRE_EFORMAT (-11) /* unknown variant or non-UTF-8 string */
#define COA_WIRE_EKEY (-12)    /* PublicKey string is not base64 of >= 32 bytes */
int coa_wire_scan(const uint8_t* frames, const uint64_t* frame_offsets, size_t n, int32_t* kind_out,
                  uint64_t* header_bytes_out, uint64_t* votes_out);
int coa_wire_decode_certificates(const uint8_t* frames, const uint64_t* frame_offsets, size_t n, uint8_t* header_data,
                                 uint64_t* header_offsets, uint8_t* ids, uint8_t* origins, uint8_t* header_sigs,
                                 uint64_t* rounds, uint8_t* vote_pks, uint8_t* vote_sigs, uint64_t* vote_offsets,
                                 uint32_t* payload_counts);
int coa_wire_decode_votes(const uint8_t* frames, const uint64_t* frame_offsets, size_t n, uint8_t* ids,
                          uint64_t* rounds, uint8_t* origins, uint8_t* authors, uint8_t* sigs);
int coa_wire_decode_headers(const uint8_t* frames, const uint64_t* frame_offsets, size_t n, uint8_t* header_data,
                            uint64_t* header_offsets, uint8_t* ids, uint8_t* authors, uint8_t* sigs,
                            uint64_t* rounds, uint32_t* payload_counts);

/* ---------------------------------------- wire decode on the device (f4)
 * The same decode with the frames in device memory, bit-identical to the
 * host decoder above, written straight into the arrays of the *_many_device
 * calls.  d_frames[d_frame_offsets[i] .. d_frame_offsets[i+1]) is frame i;
 * frame_bytes is the size of d_frames.  A frame whose range is not inside
 * [0, frame_bytes), or whose offsets decrease, is COA_WIRE_ETRUNC and none of
 * its bytes are read; no length prefix is trusted before it has been checked
 * against the frame's end.
 *
 * Three passes, all enqueued on `stream`: a scan (one wavefront per frame:
 * kind or error, digest-input length 40 + 36 |distinct payload keys| + 32
 * |distinct parents|, vote and payload counts), exclusive prefix sums of the
 * header bytes and votes (block totals, a scan of the totals, the add: three
 * launches, no kernel waits for another workgroup), and the decode and
 * scatter.
 *
 * The decode calls are index-aligned with the frames: item i belongs to
 * frame i.  Where frame i is a valid message of the call's kind every output
 * equals the host decoder's for that frame and d_kinds[i] is the kind.  For
 * any other frame d_kinds[i] is what the scan says -- another kind, a negative
 * COA_WIRE_E*, or COA_WIRE_ECAPACITY -- and item i is an empty placeholder:
 * zeroed id, keys, signature, round and payload count, no header bytes and no
 * votes (offsets[i+1] == offsets[i]).  The caller reads d_kinds before it
 * trusts item i.  Sorting frames into per-kind batches is the caller's (it
 * needs a frame's first four bytes only and no decode), or the mixed mode's
 * below, which partitions one batch by kind on the device.
 *   COA_WIRE_ECAPACITY  a Header or Certificate frame the host decoder
 *       accepts whose wire count of payload entries or of parents exceeds
 *       COA_WIRE_DEV_MAX_ENTRIES (every host error takes precedence); the
 *       caller decodes such a frame on the host.  Votes are not sorted and
 *       have no cap.
 *   d_header_offsets[0] = d_vote_offsets[0] = 0.
 *   d_totals: four words -- header bytes, votes, frames decoded as the call's
 *       kind, frames not decoded as it.
 * Output capacities are the caller's to provide: d_header_data frame_bytes +
 * 16 bytes (a digest input is never longer than its frame, and the verify
 * kernels read up to 16 bytes past the last input), the vote arrays
 * COA_WIRE_VOTES_BOUND(frame_bytes) entries, every per-frame array n (offsets
 * n + 1).  Outputs must not alias the frames.
 * `workspace`: at least coa_wire_workspace_bytes(n, frame_bytes) bytes of
 * device memory -- the call then only enqueues (no host synchronisation, no
 * copy, no allocation) -- or NULL: engine-owned, and the call waits for its
 * stream.  n = 0 returns COA_OK; a null required array or an n or frame_bytes
 * too large for one call COA_EINVAL; no device COA_ENODEVICE.
 * coa_wire_scan_device: d_header_bytes and d_votes are optional. */
#define COA_WIRE_ECAPACITY (-13)
#define COA_WIRE_DEV_MAX_ENTRIES 1024 /* per set: payload entries, parents */
#define COA_WIRE_VOTES_BOUND(frame_bytes) ((frame_bytes) / 115) /* 8 + 43 + 64: the shortest vote that decodes */
size_t coa_wire_workspace_bytes(size_t n, size_t frame_bytes);
int coa_wire_scan_device(int device, const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n,
                         size_t frame_bytes, int32_t* d_kinds, uint64_t* d_header_bytes, uint64_t* d_votes,
                         void* workspace, void* stream);
int coa_wire_decode_certificates_device(int device, const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n,
                                        size_t frame_bytes, uint8_t* d_header_data, uint64_t* d_header_offsets,
                                        uint8_t* d_ids, uint8_t* d_origins, uint8_t* d_header_sigs, uint64_t* d_rounds,
                                        uint8_t* d_vote_pks, uint8_t* d_vote_sigs, uint64_t* d_vote_offsets,
                                        uint32_t* d_payload_counts, int32_t* d_kinds, uint64_t* d_totals,
                                        void* workspace, void* stream);
int coa_wire_decode_headers_device(int device, const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n,
                                   size_t frame_bytes, uint8_t* d_header_data, uint64_t* d_header_offsets,
                                   uint8_t* d_ids, uint8_t* d_authors, uint8_t* d_sigs, uint32_t* d_payload_counts,
                                   uint64_t* d_rounds, int32_t* d_kinds, uint64_t* d_totals, void* workspace,
                                   void* stream);
int coa_wire_decode_votes_device(int device, const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n,
                                 size_t frame_bytes, uint8_t* d_ids, uint64_t* d_rounds, uint8_t* d_origins,
                                 uint8_t* d_authors, uint8_t* d_sigs, int32_t* d_kinds, uint64_t* d_totals,
                                 void* workspace, void* stream);
/* Frames to verdicts, host pointers: the drop-in for "dispatch, then verify".
 * One H2D of the frames and their offsets through the engine's page-locked
 * staging, the device decode, the *_verdict_many_device call over the decoded
 * arrays (for certificates followed by coa_certificate_votes_resolve_device,
 * so no COA_DAG_VOTES_OPEN remains) and one D2H of kinds and words, on one
 * context.  kinds_out[i] is the scan's answer for frame i; where it is not the
 * call's kind verdicts_out[i] = COA_DAG_NO_MESSAGE.  The certificate form reads
 * d_totals back (32 bytes) between the decode and the verdict call, which
 * takes its vote count as a host argument.  rng_seed as
 * coa_certificate_verdict_many.  A generation without a protocol table gives
 * COA_EINVAL, as for the verdict calls. */
#define COA_DAG_NO_MESSAGE 255u /* fused calls: frame i is not a decodable message of the call's kind */
int coa_wire_certificate_verdict_many(const uint8_t* frames, const uint64_t* frame_offsets, size_t n,
                                      uint64_t rng_seed, int32_t* kinds_out, uint32_t* verdicts_out);
int coa_wire_header_verdict_many(const uint8_t* frames, const uint64_t* frame_offsets, size_t n, int32_t* kinds_out,
                                 uint32_t* verdicts_out);
int coa_wire_vote_verdict_many(const uint8_t* frames, const uint64_t* frame_offsets, size_t n, int32_t* kinds_out,
                               uint32_t* verdicts_out);

/* ------------------------------- mixed frame batches on the device (f4)
 * One batch in which headers, votes, certificates and certificate requests
 * arrive interleaved, as PrimaryReceiverHandler::dispatch receives them:
 * a stable partition of the batch by kind on the device, so the caller neither
 * sorts the frames nor pays a placeholder's signature job.
 *
 * coa_wire_decode_mixed_device: frames, offsets, frame_bytes and the range
 * rule as the decoders above (no frame byte outside its checked range is
 * read).  The scan is theirs; the prefix sums then run over six quantities
 * (headers: frames, header bytes; votes: frames; certificates: frames, header
 * bytes, votes) in the same three launches.  d_slots[i] is the rank of frame
 * i among the frames of its kind, in frame order, where d_kinds[i] is
 * COA_MSG_HEADER, COA_MSG_VOTE or COA_MSG_CERTIFICATE, and COA_WIRE_NO_SLOT
 * for every other frame (a certificate request, a negative COA_WIRE_E*,
 * COA_WIRE_ECAPACITY).  Frame i of kind k is decoded into item d_slots[i] of
 * kind k's array set: the d_h_* arrays are coa_wire_decode_headers_device's,
 * the d_v_* arrays coa_wire_decode_votes_device's and the d_c_* arrays
 * coa_wire_decode_certificates_device's, each at the capacity that call
 * states (n per-item entries, n + 1 offsets, frame_bytes + 16 header bytes,
 * COA_WIRE_VOTES_BOUND(frame_bytes) vote rows).  With n_k frames of kind k,
 * items [0, n_k) of its set and its offsets on [0, n_k] (offsets[0] = 0) are
 * exactly what the single-kind decoder gives for the batch's frames of that
 * kind alone, in order; there are no placeholders, and nothing at or above
 * n_k (offsets: above n_k) is written.
 *   d_totals: eight words -- headers, header bytes of headers, votes,
 *       certificates, header bytes of certificates, votes of certificates,
 *       frames without a slot, 0.
 * `workspace`: at least coa_wire_mixed_workspace_bytes(n, frame_bytes) bytes
 * of device memory -- the call then only enqueues (no host synchronisation, no
 * copy, no allocation) -- or NULL: engine-owned, and the call waits for its
 * stream.  n = 0 returns COA_OK; a null required array or an n or frame_bytes
 * too large for one call COA_EINVAL; no device COA_ENODEVICE. */
#define COA_WIRE_NO_SLOT 0xFFFFFFFFu
size_t coa_wire_mixed_workspace_bytes(size_t n, size_t frame_bytes);
int coa_wire_decode_mixed_device(int device, const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n,
                                 size_t frame_bytes, uint8_t* d_h_header_data, uint64_t* d_h_header_offsets,
                                 uint8_t* d_h_ids, uint8_t* d_h_authors, uint8_t* d_h_sigs,
                                 uint32_t* d_h_payload_counts, uint64_t* d_h_rounds, uint8_t* d_v_ids,
                                 uint64_t* d_v_rounds, uint8_t* d_v_origins, uint8_t* d_v_authors, uint8_t* d_v_sigs,
                                 uint8_t* d_c_header_data, uint64_t* d_c_header_offsets, uint8_t* d_c_ids,
                                 uint8_t* d_c_origins, uint8_t* d_c_header_sigs, uint64_t* d_c_rounds,
                                 uint8_t* d_c_vote_pks, uint8_t* d_c_vote_sigs, uint64_t* d_c_vote_offsets,
                                 uint32_t* d_c_payload_counts, int32_t* d_kinds, uint32_t* d_slots,
                                 uint64_t* d_totals, void* workspace, void* stream);
/* Mixed frames to verdicts, host pointers: one H2D of the frames and their
 * offsets, the mixed decode, one 64-byte read-back of d_totals (the verdict
 * calls take their counts, the certificate call its vote count, as host
 * arguments), then on the same stream and over the compacted arrays at their
 * own counts coa_header_verdict_many_device, coa_vote_verdict_many_device and
 * coa_certificate_verdict_many_device + coa_certificate_votes_resolve_device
 * (a kind with no frame launches nothing), the scatter of the words back to
 * frame order and one D2H of kinds and words, on one context.  kinds_out[i] is
 * the scan's answer; verdicts_out[i] is frame i's COA_DAG_* word -- for each
 * kind exactly what the single-kind call above answers on the batch's frames
 * of that kind alone, in order, with the same rng_seed -- and
 * COA_DAG_NO_MESSAGE for a frame without a slot; never COA_DAG_VOTES_OPEN.
 * Arguments are accepted and rejected as by the calls above; a generation
 * without a protocol table gives COA_EINVAL. */
int coa_wire_verdict_many(const uint8_t* frames, const uint64_t* frame_offsets, size_t n, uint64_t rng_seed,
                          int32_t* kinds_out, uint32_t* verdicts_out);

/* --------------------------------------------------------------- signing
 * RFC 8032 signing == crypto::Signature::new (crypto/src/lib.rs:185-191) /
 * generate_keypair (:167-175) from 32-byte seeds.  Not on the verification
 * hot path; used to synthesise benchmark and test inputs on the device. */
int coa_ed25519_public_keys(const uint8_t* seeds, size_t n, uint8_t* pks_out);
int coa_ed25519_sign_many(const uint8_t* seeds, const uint8_t* msgs, size_t msg_len, size_t n, uint8_t* pks_out,
                          uint8_t* sigs_out);
int coa_ed25519_sign_many_device(int device, const uint8_t* d_seeds, const uint8_t* d_msgs, size_t msg_len, size_t n,
                                 uint8_t* d_pks_out, uint8_t* d_sigs_out, void* stream);

/* ------------------------------------------ the engine's own CPU path
 * The same checks as the GPU entry points above, on the host's cores
 * (csrc/coa_cpu.cpp; dalek 1.0.1 acceptance rules, verdict for verdict).
 * NEVER called implicitly: a GPU entry point that cannot answer returns a
 * negative COA_E*.  A caller that must keep answering calls these explicitly
 * -- the Rust binding does under COA_ON_ENGINE_FAILURE=cpu
 * (rust/crypto/src/degrade.rs), so verdicts do not depend on device health
 * (SURVEY.md §5).  nthreads <= 0: min(16, hardware threads).  Same return
 * conventions as the GPU forms; no coa_init needed.
 *   coa_cpu_ed25519_verify_strict      crypto/src/lib.rs:200-204
 *   coa_cpu_ed25519_verify_batch[_groups_z]  crypto/src/lib.rs:206-219
 *                                      (rng_seed as coa_ed25519_verify_batch)
 *   coa_cpu_sha512_many                worker/src/processor.rs:38,
 *                                      primary/src/messages.rs:70-84,226-234
 *   coa_cpu_certificate_verify_many[_z]  primary/src/messages.rs:189-215
 *                                      (status_out: COA_CERT_* bits; _z takes
 *                                      the votes' 16-byte weights)
 *   coa_cpu_header_verify_many         primary/src/messages.rs:49-51,64-66
 *   coa_cpu_vote_verify_many           primary/src/messages.rs:139-153
 *                                      (arguments and outputs as the GPU host
 *                                      forms above) */
int coa_cpu_ed25519_verify_strict(const uint8_t* msg, size_t msg_len, const uint8_t pk[32], const uint8_t sig[64]);
int coa_cpu_ed25519_verify_strict_many(const uint8_t* msgs, size_t msg_len, const uint8_t* pks, const uint8_t* sigs,
                                       size_t n, uint8_t* verdicts_out, int nthreads);
int coa_cpu_ed25519_verify_batch(const uint8_t msg[32], const uint8_t* pks, const uint8_t* sigs, size_t n,
                                 uint64_t rng_seed);
int coa_cpu_ed25519_verify_batch_groups_z(const uint8_t* msgs, const uint8_t* pks, const uint8_t* sigs,
                                          const uint64_t* group_offsets, size_t n_groups, const uint8_t* zs,
                                          uint8_t* group_verdicts_out, int nthreads);
int coa_cpu_sha512_many(const uint8_t* data, const uint64_t* offsets, size_t n, uint8_t* out64, int nthreads);
int coa_cpu_certificate_verify_many(const uint8_t* header_data, const uint64_t* header_offsets, const uint8_t* ids,
                                    const uint8_t* origins, const uint8_t* header_sigs, const uint64_t* rounds,
                                    const uint8_t* vote_pks, const uint8_t* vote_sigs, const uint64_t* vote_offsets,
                                    size_t n, uint64_t rng_seed, uint8_t* status_out, int nthreads);
int coa_cpu_certificate_verify_many_z(const uint8_t* header_data, const uint64_t* header_offsets, const uint8_t* ids,
                                      const uint8_t* origins, const uint8_t* header_sigs, const uint64_t* rounds,
                                      const uint8_t* vote_pks, const uint8_t* vote_sigs, const uint64_t* vote_offsets,
                                      size_t n, const uint8_t* zs, uint8_t* status_out, int nthreads);
int coa_cpu_header_verify_many(const uint8_t* header_data, const uint64_t* header_offsets, const uint8_t* ids,
                               const uint8_t* authors, const uint8_t* sigs, size_t n, uint8_t* status_out,
                               int nthreads);
int coa_cpu_vote_verify_many(const uint8_t* ids, const uint64_t* rounds, const uint8_t* origins, const uint8_t* authors,
                             const uint8_t* sigs, size_t n, uint8_t* verdicts_out, int nthreads);
/* The verdict calls on the CPU path: COA_DAG_* words, never
 * COA_DAG_VOTES_OPEN.  Stateless like the calls above: the committee arrays
 * of coa_committee_register_authorities are passed in each call and rejected
 * by the same rules.
 *   coa_cpu_certificate_verdict_many   primary/src/messages.rs:189-215
 *   coa_cpu_header_verdict_many        primary/src/messages.rs:48-67
 *   coa_cpu_vote_verdict_many          primary/src/messages.rs:131-142
 *   coa_cpu_certificate_verdict_from_status  the protocol checks and the merge
 *                                      alone, for a caller that holds the
 *                                      COA_CERT_* bits of each certificate
 *                                      (status: n bytes) */
int coa_cpu_certificate_verdict_many(const uint8_t* header_data, const uint64_t* header_offsets, const uint8_t* ids,
                                     const uint8_t* origins, const uint8_t* header_sigs, const uint64_t* rounds,
                                     const uint8_t* vote_pks, const uint8_t* vote_sigs, const uint64_t* vote_offsets,
                                     size_t n, uint64_t rng_seed, const uint32_t* payload_counts,
                                     const uint8_t* committee_pks, const uint32_t* stakes, const uint32_t* worker_ids,
                                     const uint64_t* worker_offsets, size_t n_authorities, uint32_t* verdicts_out,
                                     int nthreads);
int coa_cpu_certificate_verdict_from_status(const uint8_t* header_data, const uint64_t* header_offsets,
                                            const uint8_t* ids, const uint8_t* origins, const uint64_t* rounds,
                                            const uint8_t* vote_pks, const uint64_t* vote_offsets, size_t n,
                                            const uint32_t* payload_counts, const uint8_t* status,
                                            const uint8_t* committee_pks, const uint32_t* stakes,
                                            const uint32_t* worker_ids, const uint64_t* worker_offsets,
                                            size_t n_authorities, uint32_t* verdicts_out, int nthreads);
int coa_cpu_header_verdict_many(const uint8_t* header_data, const uint64_t* header_offsets, const uint8_t* ids,
                                const uint8_t* authors, const uint8_t* sigs, size_t n, const uint32_t* payload_counts,
                                const uint8_t* committee_pks, const uint32_t* stakes, const uint32_t* worker_ids,
                                const uint64_t* worker_offsets, size_t n_authorities, uint32_t* verdicts_out,
                                int nthreads);
int coa_cpu_vote_verdict_many(const uint8_t* ids, const uint64_t* rounds, const uint8_t* origins,
                              const uint8_t* authors, const uint8_t* sigs, size_t n, const uint8_t* committee_pks,
                              const uint32_t* stakes, const uint32_t* worker_ids, const uint64_t* worker_offsets,
                              size_t n_authorities, uint32_t* verdicts_out, int nthreads);
/* coa_wire_verdict_many on the CPU path: coa_wire_scan, the partition by kind
 * on the host, the three host decoders, the three calls above and the scatter
 * back to frame order.  kinds_out and verdicts_out as coa_wire_verdict_many,
 * but for one case: the host decoder has no entry cap, so a frame the device
 * reports as COA_WIRE_ECAPACITY is answered here as its real kind with a real
 * word. */
int coa_cpu_wire_verdict_many(const uint8_t* frames, const uint64_t* frame_offsets, size_t n, uint64_t rng_seed,
                              const uint8_t* committee_pks, const uint32_t* stakes, const uint32_t* worker_ids,
                              const uint64_t* worker_offsets, size_t n_authorities, int32_t* kinds_out,
                              uint32_t* verdicts_out, int nthreads);

/* ------------------------------------------------ aggregation queue (f1)
 * Pre-verification stage for Core::run (primary/src/core.rs:349-389), which
 * verifies one message at a time: producers submit header/vote signatures,
 * vote batches, certificates and worker batch digests; the queue coalesces
 * them into launches (when max_batch items are pending, when the oldest
 * request is max_delay_us old, or on flush) and replies per request through
 * the callback -- the SignatureService request/oneshot idiom of
 * crypto/src/lib.rs:222-250.  Inputs are copied at submission (into one of
 * a fixed pool of intake shards, chosen by the calling thread).  Two lanes,
 * each with its own collector, device slots and completion thread: one for
 * signatures, vote batches and certificates, one for digests (a digest
 * window is a 14 ms serial chain; it never delays a verdict).  A lane's
 * collector launches each window on a free slot (four per GPU for verdicts,
 * eight for digests, COA_QUEUE_SLOTS / COA_QUEUE_DIGEST_SLOTS; pinned staging, its own stream
 * on its own hardware queue, COA_QUEUE_STREAMS) without waiting for the
 * previous window, and its completion thread answers windows in order: the
 * callback runs there with status (COA_OK or a negative engine error) and
 * the request's verdict byte(s).  The requests a window's kernels cannot
 * decide alone -- certificates with a key outside the registered committee
 * or with votes that failed their own equation, and bare vote batches -- are
 * answered later, by the lane's resolver thread (the exact path), so they
 * never hold back the rest of their window; answers are therefore not in
 * submission order across requests.  Windows that read the committee key cache
 * pin the generation they launched with; coa_committee_register builds the
 * next generation beside it, so registration neither waits for nor holds
 * back a window and stays verdict-neutral under load. */
typedef struct coa_queue coa_queue;
typedef void (*coa_verdict_cb)(void* user, int status, const uint8_t* verdicts, size_t n);
coa_queue* coa_queue_create(size_t max_batch, uint32_t max_delay_us);
int coa_queue_submit_verify(coa_queue* q, const uint8_t msg[32], const uint8_t pk[32], const uint8_t sig[64],
                            coa_verdict_cb cb, void* user);
/* n independent triples in one request (one copy, one lock, one callback
 * with the n verdict bytes in order): for producers that already hold a
 * group of messages, e.g. a window of received votes. */
int coa_queue_submit_verify_many(coa_queue* q, const uint8_t* msgs, const uint8_t* pks, const uint8_t* sigs, size_t n,
                                 coa_verdict_cb cb, void* user);
int coa_queue_submit_batch(coa_queue* q, const uint8_t msg[32], const uint8_t* pks, const uint8_t* sigs, size_t n,
                           coa_verdict_cb cb, void* user);
/* Whole certificates (the fused Certificate::verify crypto, f3): the
 * callback receives one status byte of COA_CERT_* bits (0 = all Ok). */
int coa_queue_submit_certificate(coa_queue* q, const uint8_t* header_data, size_t header_len, const uint8_t id[32],
                                 const uint8_t origin[32], const uint8_t header_sig[64], uint64_t round,
                                 const uint8_t* vote_pks, const uint8_t* vote_sigs, size_t n_votes, coa_verdict_cb cb,
                                 void* user);
/* The same without the copy: the arrays are read in place -- packed by the
 * launch that takes the request straight into the device staging, and read
 * again by the resolver if the certificate needs the exact re-decision -- so
 * they must stay valid and unchanged until the callback has run.  For callers
 * that hold each request's bytes until its answer anyway
 * (rust/crypto/src/service.rs boxes them with the reply sender): the
 * producer's copy, one of the streamed path's two host copies, is gone. */
int coa_queue_submit_certificate_borrowed(coa_queue* q, const uint8_t* header_data, size_t header_len,
                                          const uint8_t id[32], const uint8_t origin[32], const uint8_t header_sig[64],
                                          uint64_t round, const uint8_t* vote_pks, const uint8_t* vote_sigs,
                                          size_t n_votes, coa_verdict_cb cb, void* user);
/* Worker batch digests (worker/src/processor.rs:38, Processor::spawn): the
 * callback receives the 32-byte Digest (n = 32). */
int coa_queue_submit_digest(coa_queue* q, const uint8_t* data, size_t len, coa_verdict_cb cb, void* user);
/* Whole headers: Header::verify's crypto (primary/src/messages.rs:49-51, the
 * id check, and 64-66, the author's signature over the id), with
 * coa_header_verify_many's semantics.  The callback receives one status byte
 * of COA_CERT_BAD_HEADER_ID | COA_CERT_BAD_HEADER_SIG bits (0 = both Ok).
 * Inputs are copied at submission. */
int coa_queue_submit_header(coa_queue* q, const uint8_t* header_data, size_t header_len, const uint8_t id[32],
                            const uint8_t author[32], const uint8_t sig[64], coa_verdict_cb cb, void* user);
/* Whole votes: Vote::verify's crypto (primary/src/messages.rs:145-153,
 * Vote::digest, and 139-141, the author's signature over it), with
 * coa_vote_verify_many's semantics: Vote::digest is hashed on the device.  The
 * callback receives one verdict byte, 0 Ok / 1 Err. */
int coa_queue_submit_vote(coa_queue* q, const uint8_t id[32], uint64_t round, const uint8_t origin[32],
                          const uint8_t author[32], const uint8_t sig[64], coa_verdict_cb cb, void* user);
/* Both kinds live on the verdict lane, count one item each towards max_batch
 * and one signature each in coa_queue_stats / coa_queue_metrics, and run on
 * the registered committee's key combs: a window of at most
 * COA_QUEUE_MSG_LAT_MAX messages (read at coa_queue_create) takes the latency
 * kernel (one workgroup per message; alone in its window and at most 64, its
 * verdict words are published to page-locked memory, no copy back), a larger
 * one the throughput kernels of coa_header_verify_many_device /
 * coa_vote_verify_many_device.  A message whose author is not registered is
 * decided by the resolver thread through the uncached path, so the answer is
 * dalek's verify_strict plus the digest check with any committee or none.
 * No reference counterpart: requests and windows of each route since creation
 * or the last coa_queue_metrics_reset (any pointer may be null). */
int coa_queue_message_stats(coa_queue* q, uint64_t* headers, uint64_t* votes, uint64_t* latency_windows,
                            uint64_t* throughput_windows);
/* Verdict requests: the reference's whole DagResult of Certificate::verify /
 * Header::verify / Vote::verify, decided in the window that carries the
 * request.  The arguments are those of the crypto requests above plus
 * payload_count (the header's payload entries, as in the *_verdict_many
 * calls); the callback receives n = 4, one little-endian uint32_t verdict
 * word (COA_DAG_*), with exactly the meaning of coa_certificate_verdict_many /
 * coa_header_verdict_many / coa_vote_verdict_many and never
 * COA_DAG_VOTES_OPEN.  A payload_count with 40 + 36 * count > header_len is
 * refused at submission with COA_EINVAL.
 *   - The committee must have been registered with
 *     coa_committee_register_authorities.  A window pins its key-cache
 *     generation and reads that generation's protocol table; if it has none
 *     (plain coa_committee_register, or no registration), the window's verdict
 *     requests are answered with status COA_EINVAL and the word
 *     COA_DAG_INVALID_SIGNATURE.  That is no engine failure: nothing is
 *     retried, no failure counter moves, and the rest of the window is
 *     answered as usual.
 *   - With a negative status (an engine error, or COA_EINVAL as above) the
 *     word is COA_DAG_INVALID_SIGNATURE.
 *   - Who answers: an item whose author or a voter is outside the committee
 *     is answered by the protocol word alone, in its window -- it never goes
 *     to the resolver thread.  Only a certificate whose every earlier check
 *     passed and whose votes need the exact check (COA_DAG_VOTES_OPEN on the
 *     device) is left to the resolver, which answers COA_DAG_INVALID_VOTES or
 *     COA_DAG_OK.
 *   - Verdict requests live on the verdict lane and share windows, intake
 *     shards, slots, retry and ordering rules with the crypto requests; a
 *     window may mix both, and the crypto requests' answers and routes are
 *     what they are without them.  A header or vote verdict request counts one
 *     item towards max_batch and one signature in coa_queue_stats /
 *     coa_queue_metrics; a certificate verdict request counts as a
 *     certificate request does.
 *   - One kernel (k_window_verdict) after the window's crypto launches
 *     decides the protocol checks of all its certificates, headers and votes
 *     and merges them with the crypto status words; its words come back with
 *     the window's one device-to-host copy.  A window that holds a verdict
 *     request takes the staged route -- except a window of header and vote
 *     verdicts alone of at most COA_QUEUE_MSG_LAT_MAX messages: the message
 *     latency kernel decides their protocol checks itself (k_msg_verdict_lat),
 *     on the routes of the crypto messages (alone and at most 64: the words
 *     published, no copy back) and with no further launch.
 * coa_queue_verdict_stats: verdict requests answered by kind and the windows
 * that held one, since creation or the last coa_queue_metrics_reset (any
 * pointer may be null).  No reference counterpart. */
int coa_queue_submit_certificate_verdict(coa_queue* q, const uint8_t* header_data, size_t header_len,
                                         const uint8_t id[32], const uint8_t origin[32], const uint8_t header_sig[64],
                                         uint64_t round, const uint8_t* vote_pks, const uint8_t* vote_sigs,
                                         size_t n_votes, uint32_t payload_count, coa_verdict_cb cb, void* user);
int coa_queue_submit_certificate_verdict_borrowed(coa_queue* q, const uint8_t* header_data, size_t header_len,
                                                  const uint8_t id[32], const uint8_t origin[32],
                                                  const uint8_t header_sig[64], uint64_t round,
                                                  const uint8_t* vote_pks, const uint8_t* vote_sigs, size_t n_votes,
                                                  uint32_t payload_count, coa_verdict_cb cb, void* user);
int coa_queue_submit_header_verdict(coa_queue* q, const uint8_t* header_data, size_t header_len, const uint8_t id[32],
                                    const uint8_t author[32], const uint8_t sig[64], uint32_t payload_count,
                                    coa_verdict_cb cb, void* user);
int coa_queue_submit_vote_verdict(coa_queue* q, const uint8_t id[32], uint64_t round, const uint8_t origin[32],
                                  const uint8_t author[32], const uint8_t sig[64], coa_verdict_cb cb, void* user);
int coa_queue_verdict_stats(coa_queue* q, uint64_t* certificates, uint64_t* headers, uint64_t* votes,
                            uint64_t* verdict_windows);
int coa_queue_flush(coa_queue* q);
/* Window policy (no reference counterpart): with windows_in_flight = k > 0 a
 * window also closes at once while fewer than k windows are in flight, so a
 * request reaching an idle queue launches without waiting out max_delay_us;
 * under load requests still coalesce behind the windows in flight.  0 (the
 * default; COA_QUEUE_IDLE_LAUNCH=k at creation sets k) keeps the deadline
 * policy alone.  For latency-bound stages (the primary's pre-verification:
 * committee-100 round mix p50 0.31-0.39 -> 0.07-0.26 ms) rather than
 * throughput streams (worker batch digests). */
int coa_queue_set_idle_launch(coa_queue* q, uint32_t windows_in_flight);
/* items = signatures answered (a coa_queue_submit_verify_many request of n
 * counts n); groups = vote batches + certificates. */
int coa_queue_stats(coa_queue* q, uint64_t* launches, uint64_t* items, uint64_t* groups);
int coa_queue_digest_count(coa_queue* q, uint64_t* digests);
/* Queue metrics since creation.  A window is the set of requests one launch
 * takes; windows are pipelined (the next window is packed and its copies and
 * kernels enqueued while the previous one runs).  wait_us_* is the time from
 * a request's submission to the start of its callback (percentiles from a
 * log-spaced histogram, +-6 %).
 * Engine-failure recovery: a window whose launch fails (a HIP error) is
 * re-run on the recovery context of each device in turn (the failed slot's
 * stream, event and buffers rebuilt meanwhile, in the same process); its
 * callbacks get a negative status only when every attempt failed. */
typedef struct {
  uint64_t requests;      /* requests answered */
  uint64_t windows;       /* launch windows */
  uint64_t signatures;    /* signatures answered (verify requests x their n) */
  uint64_t batches;       /* vote-batch requests */
  uint64_t certificates;  /* certificate requests */
  uint64_t digests;       /* digest requests */
  uint64_t max_window;    /* most items (signatures + votes + digests) in one window */
  uint64_t max_in_flight; /* most windows launched and not yet answered at once */
  uint64_t max_pending;   /* most items waiting for a window at once */
  double wait_us_mean, wait_us_p50, wait_us_p99, wait_us_max;
  uint64_t retried_windows;   /* windows whose launch failed and were re-run */
  uint64_t recovered_windows; /* ... of which a re-run succeeded */
  uint64_t failed_windows;    /* windows answered with an engine error */
  /* where a tail comes from: the slowest window from its launch call (the
   * collector hands it to a slot) to its outputs in host memory, with its
   * size and kinds; the longest a launch waited for a free slot; staging
   * reallocations (page-locked or device allocations on the launch path) */
  double window_us_max;
  uint64_t window_max_items;
  uint32_t window_max_kinds;  /* COA_QUEUE_KIND_* bits */
  int32_t stream_kind;        /* COA_QUEUE_STREAM_*: how the slots' streams were made */
  double slot_wait_us_max;
  uint64_t staging_grows;     /* windows that had to enlarge a slot's staging or workspace (warm-up not counted) */
  uint32_t slots_verify, slots_digest; /* device slots of each lane, over all devices */
  /* Two-step answers: certificates the fused kernel could not decide alone
   * (a key outside the registered committee, an inconclusive vote) and bare
   * vote batches go to the lane's resolver thread, which decides them exactly
   * (coa_certificate_verify_many's semantics); the rest of their window is
   * answered at once.  So one open certificate never holds back the requests
   * it shares a window with, nor the windows behind it. */
  uint64_t deferred_requests; /* requests answered by the resolver */
  uint64_t resolver_passes;   /* resolver passes (each decides every open request queued by then) */
  double resolve_us_max;      /* the longest resolver pass */
  /* Where the time goes, summed over every window (microseconds, COA_QSTAGE_*
   * indices; divide by `windows` for a mean per window). */
  double stage_us[12];
  /* When the slowest window (window_us_max) was launched, in milliseconds
   * since the queue's creation or its last coa_queue_metrics_reset, and how
   * much of it was spent waiting for its device work (COA_QSTAGE_DEVICE_WAIT):
   * a one-off tail at a run's start points at set-up costs, one in the
   * device wait at the device. */
  double window_max_at_ms;
  double window_max_device_us;
} coa_queue_metrics_t;
#define COA_QSTAGE_INTAKE 0      /* producers: shard lock + copy of the request into the shard */
#define COA_QSTAGE_GATHER 1      /* collector: taking the shards' windows */
#define COA_QSTAGE_SLOT_WAIT 2   /* launch: waiting for a free device slot */
#define COA_QSTAGE_PACK 3        /* launch: parts -> page-locked staging */
#define COA_QSTAGE_ENQUEUE 4     /* launch: H2D copy, kernels and D2H copy enqueued */
#define COA_QSTAGE_DEVICE_WAIT 5 /* completer: blocked on the window's event */
#define COA_QSTAGE_SCATTER 6     /* completer: outputs -> the parts' verdicts */
#define COA_QSTAGE_CALLBACKS 7   /* completer (and helpers): the callbacks */
#define COA_QSTAGE_RESOLVE 8     /* resolver: exact decision of the deferred requests */
#define COA_QSTAGES 9
#define COA_QUEUE_KIND_SIGNATURES 1u
#define COA_QUEUE_KIND_BATCHES 2u
#define COA_QUEUE_KIND_CERTIFICATES 4u
#define COA_QUEUE_KIND_DIGESTS 8u
#define COA_QUEUE_KIND_HEADERS 16u
#define COA_QUEUE_KIND_VOTES 32u
/* COA_QUEUE_STREAMS=plain|cumask|priority (read at the first launch): plain
 * streams share the process's GPU_MAX_HW_QUEUES hardware queues (HIP's
 * default 4) with every other stream of the process; CU-masked streams (all
 * CUs enabled) get a hardware queue each, whatever GPU_MAX_HW_QUEUES says;
 * priority streams come from the high-priority pool (verify lane) */
#define COA_QUEUE_STREAM_PLAIN 0
#define COA_QUEUE_STREAM_CUMASK 1
#define COA_QUEUE_STREAM_PRIORITY 2
int coa_queue_metrics(coa_queue* q, coa_queue_metrics_t* out);
/* Zeroes the counters, maxima, stage times and the wait histogram (not the
 * slot counts): the next coa_queue_metrics covers only what happens after,
 * e.g. a steady-state interval after a warm-up.  No reference counterpart. */
int coa_queue_metrics_reset(coa_queue* q);
int coa_queue_destroy(coa_queue* q);

#ifdef __cplusplus
}
#endif
#endif /* COA_VERIFY_H */
