/*
 * blsgpu.h — C-ABI of the MI355X batch BLS12-381 signature-set verifier
 * (libblsgpu.so).  Drop-in engine behind Lodestar's IBlsVerifier:
 *
 *   packages/beacon-node/src/chain/bls/interface.ts:20-46
 *     verifySignatureSets(sets: ISignatureSet[], opts?: VerifySignatureOpts): Promise<boolean>
 *     close(): Promise<void>
 *
 * Each entry point below names the reference function it replaces.  The
 * reference holds no native code of its own: the arithmetic lives in the
 * un-vendored dependency @chainsafe/bls@7.1.1 -> @chainsafe/blst@0.2.4 ->
 * supranational blst (yarn.lock:458-473), which this library re-implements as
 * HIP kernels for gfx950.
 *
 * Conventions: plain C, no exceptions cross the boundary, every function
 * returns an int status (BGV_OK = 0, negative = call failed, see bgv_strerror).
 * Verdict codes per job are 1 (valid), 0 (invalid) or -code where code is one
 * of the BLST-numbered errors below.  One context per process; calls on one
 * context are serialised internally.
 */
#ifndef BLSGPU_H
#define BLSGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Error codes.  1..8 follow blst's BLST_ERROR enum (the message of the
 * rejected Promise contains the name, e.g. "BLST_INVALID_SIZE",
 * beacon-node/test/e2e/chain/bls/multithread.test.ts:86-103). */
enum {
  BGV_OK = 0,
  BGV_BLST_BAD_ENCODING = 1,
  BGV_BLST_POINT_NOT_ON_CURVE = 2,
  BGV_BLST_POINT_NOT_IN_GROUP = 3,
  BGV_BLST_AGGR_TYPE_MISMATCH = 4,
  BGV_BLST_VERIFY_FAIL = 5,
  BGV_BLST_PK_IS_INFINITY = 6,
  BGV_BLST_BAD_SCALAR = 7,
  BGV_BLST_INVALID_SIZE = 8,
  BGV_E_EMPTY_AGGREGATE = 20, /* PublicKey.aggregate([]) — "EMPTY_AGGREGATE_ARRAY" (chain/bls/utils.ts:11) */
  BGV_E_EMPTY_SET = 21,       /* "Empty signature set" (chain/bls/maybeBatch.ts:29-31) */
  BGV_E_BAD_INDEX = 22,       /* validator index not in the device pubkey cache */
  BGV_E_ARG = 23,             /* malformed call */
  BGV_E_DEVICE = 30,          /* HIP error: never reported as a verdict */
  BGV_E_NOMEM = 31,
  BGV_E_CLOSED = 32           /* QueueError QUEUE_ABORTED after close() (multithread/index.ts:176-186,239-241) */
};

/* Verification modes of bgv_verify. */
enum {
  /* BlsMultiThreadWorkerPool worker semantics (multithread/worker.ts:32-108):
   * batchable jobs are verified together, and when a device group that mixes
   * jobs fails, every job in it is re-verified alone; non-batchable jobs are
   * verified alone (no retry). */
  BGV_MODE_WORKER = 0,
  /* every job verified alone (verifySignatureSetsMaybeBatch per job,
   * maybeBatch.ts:16-39; also BlsSingleThreadVerifier, singleThread.ts:14-36) */
  BGV_MODE_PER_JOB = 1
};

/* Pubkey record formats for bgv_pubkeys_put. */
enum { BGV_PK_COMPRESSED = 48, BGV_PK_UNCOMPRESSED = 96 };

typedef struct bgv_ctx bgv_ctx;

/* One signature set: ISignatureSet (state-transition/src/util/signatureSets.ts:5-22).
 * single     -> n_pk = 1
 * aggregate  -> n_pk = pubkeys.length (0 rejects with BGV_E_EMPTY_AGGREGATE)
 * Pubkeys are trusted (already subgroup/infinity checked, interface.ts:33-36) and are
 * given either as validator indices into the device cache (pk_indices) or, for keys
 * not in the cache, as n_pk x 96-byte uncompressed records (pk_bytes, the
 * SerializedSet.publicKey format of multithread/types.ts:8-12). */
typedef struct {
  uint32_t n_pk;
  uint32_t sig_len;           /* length of sig as received; 96 is the only valid size */
  const uint32_t* pk_indices; /* n_pk indices, or NULL */
  const uint8_t* pk_bytes;    /* n_pk * 96 bytes when pk_indices is NULL */
  const uint8_t* msg;         /* 32-byte signing root */
  const uint8_t* sig;         /* compressed G2 signature, untrusted wire bytes */
} bgv_set;

/* One verifySignatureSets job (BlsWorkReq, multithread/types.ts:14-17): a
 * contiguous run of sets and its VerifySignatureOpts.batchable flag. */
typedef struct {
  uint32_t first_set;
  uint32_t n_sets;
  uint32_t batchable;
} bgv_job;

/* Counters mirroring BlsWorkResult (multithread/types.ts:24-36) plus device timing. */
typedef struct {
  uint64_t batch_retries;      /* mixed-job device groups that failed and were retried per job */
  uint64_t batch_sigs_success; /* sets verified valid in mixed-job groups */
  uint64_t device_groups;      /* device groups launched (each one final exponentiation) */
  uint64_t sets_verified;      /* slots launched, retries included */
  double device_ms;            /* HIP-event time of the kernels of this call */
  double wall_ms;              /* host wall time of the call */
} bgv_stats;

/* Create a context on the given HIP devices (NULL/0 = device 0).  Replaces the
 * pool constructor, multithread/index.ts:114-132. */
int bgv_init(const int* devices, int ndev, bgv_ctx** out);

/* Release all device memory.  After bgv_close() every call returns BGV_E_CLOSED. */
int bgv_close(bgv_ctx* ctx);
int bgv_destroy(bgv_ctx* ctx);

/* Upload validator pubkeys [first_index, first_index + n) into the device-resident
 * cache (replicated on every device).  fmt = BGV_PK_COMPRESSED (48-byte ZCash, as in
 * the beacon state) or BGV_PK_UNCOMPRESSED (96 bytes).  Keys are trusted: decoded
 * without a subgroup check, as Index2PubkeyCache does
 * (state-transition/src/cache/pubkeyCache.ts:56-77, epochContext.ts:702-705).
 * Appending (first_index == bgv_pubkeys_count) does not wait for running verifies: the keys
 * are decoded into staging memory and published once every device holds them.  A gap
 * (first_index > count) returns -BGV_E_ARG and writes nothing.  Undecodable records do not
 * stop the run: every index of it is committed, the undecodable ones are marked (a set that
 * names one rejects with BGV_E_BAD_INDEX) and -code of the first undecodable key is
 * returned; a later put over the same index replaces the mark. */
int bgv_pubkeys_put(bgv_ctx* ctx, uint32_t first_index, const uint8_t* keys, size_t n, int fmt);
size_t bgv_pubkeys_count(const bgv_ctx* ctx);

/* Verify njobs jobs over nsets sets; out_job_codes[j] receives 1, 0 or -error.
 * Replaces BlsMultiThreadWorkerPool.verifySignatureSets + the worker's
 * verifyManySignatureSets + verifySignatureSetsMaybeBatch
 * (multithread/index.ts:134-174, worker.ts:32-108, maybeBatch.ts:16-39).
 * stats may be NULL. */
int bgv_verify(bgv_ctx* ctx, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets, int mode,
               int32_t* out_job_codes, bgv_stats* stats);

/* Asynchronous form for the N-API addon (napi_async_work): the call runs on the
 * context's worker thread and `done(user, rc)` is invoked there when out_job_codes
 * and stats are filled.  The caller keeps every buffer alive until then. */
typedef void (*bgv_done_fn)(void* user, int rc);
int bgv_verify_async(bgv_ctx* ctx, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets, int mode,
                     int32_t* out_job_codes, bgv_stats* stats, bgv_done_fn done, void* user);

/* Committee-bitfield signature sets ------------------------------------------
 * The beacon node never starts from a list of attesting validators: it holds a committee
 * (an epoch shuffling's, or the 512-member sync committee) and a participation bitfield and
 * expands them with bits.intersectValues(committeeIndices)
 * (state-transition/src/cache/epochContext.ts:620-622, block/processSyncCommittee.ts:16,77,
 * block/processAttestationsAltair.ts:50).  Here a committee is uploaded once and a set names
 * (committee, bitfield): the device keeps the committee's index table and its full pubkey sum
 * and adds whichever side is shorter -- the participants, or the absentees subtracted from the
 * total.  The aggregate is the same group element, so verdicts are those of the expanded list.
 *
 * bgv_committee_put stores indices[0, n) (1 <= n <= 65536) under id < BGV_MAX_COMMITTEES on every
 * device of the context and computes their pubkey sum there.  Every index must be below
 * bgv_pubkeys_count and not marked undecodable (-BGV_E_BAD_INDEX, nothing stored); a put on an id
 * that is still live returns -BGV_E_ARG.  A put never waits for running verifies unless the
 * device's index pool has to grow.  A bgv_pubkeys_put (or bgv_keygen) over existing indices
 * recomputes the sums of the live committees that hold one of them before it returns; a committee
 * that then holds a marked key makes every set naming it reject with BGV_E_BAD_INDEX.  A dropped
 * committee that a queued call still names is recomputed the same way.
 * bgv_committee_drop frees the id for reuse at once (-BGV_E_BAD_INDEX: no such committee); the
 * device storage is reused only after the calls laid out before the drop have finished. */
#define BGV_MAX_COMMITTEES 16384 /* ids 0..16383: 3 epochs x 2048 committees + sync committees */
#define BGV_NO_COMMITTEE 0xFFFFFFFFu
int bgv_committee_put(bgv_ctx* ctx, uint32_t id, const uint32_t* indices, size_t n);
int bgv_committee_drop(bgv_ctx* ctx, uint32_t id);

/* All committees of one epoch in one call: the device computes the epoch's shuffling and cuts it
 * into count = slots * committees_per_slot committees, ids first_id .. first_id + count - 1.
 * Replaces computeEpochShuffling with unshuffleList (state-transition/src/util/epochShuffling.ts:59-97,
 * util/shuffle.ts) and the bgv_committee_put per committee that would follow it:
 *   shuffling[i] = active_indices[p(i)], p(i) the spec's compute_shuffled_index(i, n_active, seed)
 *   over `rounds` swap-or-not rounds r = 0 .. rounds - 1 (pivot = LE64(sha256(seed | r)[0:8]) mod n,
 *   flip = (pivot + n - i) mod n, pos = max(i, flip), src = sha256(seed | r | LE32(pos >> 8)),
 *   i = flip iff (src[(pos & 255) >> 3] >> (pos & 7)) & 1);
 *   committee k = slot * committees_per_slot + index is
 *   shuffling[floor(n k / count), floor(n (k + 1) / count)).
 * The host passes the preset: slots (SLOTS_PER_EPOCH), committees_per_slot (computeCommitteeCount)
 * and rounds (SHUFFLE_ROUND_COUNT; at most 255); rounds == 0 or n_active == 1 leave the list as it
 * is.  out_shuffling (may be NULL) receives the n_active shuffled indices, IEpochShuffling.shuffling.
 * A non-empty committee is a committee in every respect (sets, bgv_aggregate_committee_bits,
 * bgv_committee_drop, recomputed after a bgv_pubkeys_put over a member); an empty one
 * (n_active < count) gets no id.  All or nothing: on an error no id of the range exists.
 * -BGV_E_ARG: n_active < 1 or > 2^22, slots or committees_per_slot 0, first_id + count >
 * BGV_MAX_COMMITTEES, rounds > 255, a committee longer than 65536, an id of the range still live;
 * -BGV_E_BAD_INDEX: an index at or past bgv_pubkeys_count, or a marked one; -BGV_E_NOMEM: fewer
 * free handles than non-empty committees.  Like bgv_committee_put it waits for running verifies
 * only when the index pool has to grow.
 * bgv_committee_drop_range drops the live ids of [first_id, first_id + count) and returns how
 * many there were (>= 0); storage is reused as after bgv_committee_drop. */
int bgv_shuffling_put(bgv_ctx* ctx, uint32_t first_id, const uint8_t seed[32], const uint32_t* active_indices,
                      size_t n_active, uint32_t slots, uint32_t committees_per_slot, uint32_t rounds,
                      uint32_t* out_shuffling);
int bgv_committee_drop_range(bgv_ctx* ctx, uint32_t first_id, uint32_t count);

/* Balance-weighted sampling on the device: computeProposerIndex and getNextSyncCommittee
 * (state-transition/src/util/seed.ts:22-126, util/syncCommittee.ts:21-38).  For a 32-byte seed,
 * n_active active indices and candidate i = 0, 1, 2, ...:
 *   v_i    = active_indices[compute_shuffled_index(i mod n_active, n_active, seed)]  (rounds rounds,
 *            as bgv_shuffling_put)
 *   byte_i = sha256(seed | LE64(i div 32))[i mod 32]
 *   candidate i is accepted iff eff_incr[v_i] * 255 >= max_incr * byte_i
 * eff_incr is EffectiveBalanceIncrements (one byte per validator index, n_eff of them) and max_incr
 * the preset's MAX_EFFECTIVE_BALANCE / EFFECTIVE_BALANCE_INCREMENT.  At most BGV_SAMPLE_MAX_TRIES
 * candidates of a seed are examined, which bounds every call.
 *
 * bgv_proposers: out_proposers[s] = the first accepted v_i of seeds32[32 s ..), for n_seeds seeds
 * (1..1024; the caller hashes epochSeed | LE64(slot) per slot as computeProposers does), or
 * BGV_NO_PROPOSER when all n_active candidates were rejected (the reference's -1).  The pubkey
 * cache is not involved.  -BGV_E_ARG, and nothing written: a null pointer, n_seeds out of range,
 * n_active 0 or > 2^22, rounds > 255, max_incr 0 or > 255, an active index >= n_eff, or a seed whose
 * first BGV_SAMPLE_MAX_TRIES candidates were all rejected while n_active is larger than that.
 *
 * bgv_sync_committee_put: the first `size` accepted v_i (1..65536; in order, repeats kept: i runs
 * past n_active) become committee `id`, a committee in every respect exactly as after a
 * bgv_committee_put of the same list.  out_indices (may be NULL) receives the list, out_agg48 (may
 * be NULL) the members' pubkey sum, repeats counted, as 48 compressed bytes
 * (SyncCommittee.aggregatePubkey).  -BGV_E_ARG: the argument checks above, an id that is live or
 * >= BGV_MAX_COMMITTEES, or fewer than `size` acceptances within BGV_SAMPLE_MAX_TRIES candidates
 * (where the reference's loop would go on; a zero balance is accepted on a random byte of 0
 * only); -BGV_E_BAD_INDEX: an active index at or past
 * bgv_pubkeys_count, or a marked one.  All or nothing: on any error the id does not exist.
 *
 * bgv_proposers_electra, bgv_sync_committee_put_electra: the same two calls under the acceptance
 * rule of Electra (EIP-7251: the consensus spec's compute_proposer_index and
 * get_next_sync_committee_indices draw 16 bits per candidate from that fork on).  v_i as above;
 *   rand_i = LE16(sha256(seed | LE64(i div 16))[2 (i mod 16) .. 2 (i mod 16) + 2))
 *   candidate i is accepted iff eff_incr16[v_i] * 65535 >= max_incr * rand_i
 * eff_incr16 is EffectiveBalanceIncrements from Electra on (a Uint16Array: one uint16_t per
 * validator index, n_eff of them) and max_incr MAX_EFFECTIVE_BALANCE_ELECTRA /
 * EFFECTIVE_BALANCE_INCREMENT (2048 on mainnet), 1..65535.  Everything said of bgv_proposers and
 * bgv_sync_committee_put above holds for them -- the argument checks, BGV_NO_PROPOSER, the
 * BGV_SAMPLE_MAX_TRIES cap, all or nothing, -BGV_E_BAD_INDEX, the committee being a committee in
 * every respect on every device -- with "max_incr 0 or > 65535" in place of "0 or > 255" and a
 * zero balance accepted on a random value of 0 only. */
#define BGV_NO_PROPOSER 0xFFFFFFFFu
#define BGV_SAMPLE_MAX_TRIES 65536u
int bgv_proposers(bgv_ctx* ctx, const uint8_t* seeds32, uint32_t n_seeds, const uint32_t* active_indices,
                  size_t n_active, const uint8_t* eff_incr, size_t n_eff, uint32_t max_incr, uint32_t rounds,
                  uint32_t* out_proposers);
int bgv_sync_committee_put(bgv_ctx* ctx, uint32_t id, const uint8_t seed[32], const uint32_t* active_indices,
                           size_t n_active, const uint8_t* eff_incr, size_t n_eff, uint32_t max_incr, uint32_t size,
                           uint32_t rounds, uint32_t* out_indices, uint8_t out_agg48[48]);
int bgv_proposers_electra(bgv_ctx* ctx, const uint8_t* seeds32, uint32_t n_seeds, const uint32_t* active_indices,
                          size_t n_active, const uint16_t* eff_incr16, size_t n_eff, uint32_t max_incr,
                          uint32_t rounds, uint32_t* out_proposers);
int bgv_sync_committee_put_electra(bgv_ctx* ctx, uint32_t id, const uint8_t seed[32], const uint32_t* active_indices,
                                   size_t n_active, const uint16_t* eff_incr16, size_t n_eff, uint32_t max_incr,
                                   uint32_t size, uint32_t rounds, uint32_t* out_indices, uint8_t out_agg48[48]);

/* The pubkeys of one set as committee members: member k takes part iff
 * (bits[k >> 3] >> (k & 7)) & 1 (SSZ bit order); bits holds ceil(n_bits / 8) bytes.
 * committee == BGV_NO_COMMITTEE: the set's own pk_indices / pk_bytes count. */
typedef struct {
  uint32_t committee;
  uint32_t n_bits;
  const uint8_t* bits;
} bgv_pkbits;

/* bgv_verify / bgv_verify_async with pkbits[i] beside sets[i] (pkbits may be NULL: bgv_verify).
 * Where pkbits[i].committee != BGV_NO_COMMITTEE, set i's n_pk, pk_indices and pk_bytes are
 * ignored.  The host's argument checks give the job of a malformed set its code, as for index
 * sets: an unknown or dropped id -BGV_E_BAD_INDEX, n_bits other than the committee's length
 * -BGV_E_ARG, a set bit at or past n_bits in the last byte -BGV_E_ARG, no bit set
 * -BGV_E_EMPTY_AGGREGATE.  Everything else is the call with the expanded index list. */
int bgv_verify_bits(bgv_ctx* ctx, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                    const bgv_pkbits* pkbits, int mode, int32_t* out_job_codes, bgv_stats* stats);
int bgv_verify_bits_async(bgv_ctx* ctx, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                          const bgv_pkbits* pkbits, int mode, int32_t* out_job_codes, bgv_stats* stats,
                          bgv_done_fn done, void* user);

/* Parity hook beside bgv_aggregate_pubkeys: the aggregate of a committee's selected members
 * through the verify path's own kernel (k_pk_agg_bits, the side the layout would take),
 * 96-byte uncompressed encoding (0x40 for infinity).  Codes as the set checks above. */
int bgv_aggregate_committee_bits(bgv_ctx* ctx, uint32_t id, const uint8_t* bits, uint32_t n_bits, uint8_t out96[96]);

/* One bitfield over several committees: the attestation format since EIP-7549, where
 * committee_bits selects up to MAX_COMMITTEES_PER_SLOT committees of a slot and aggregation_bits is
 * laid over them, concatenated in ascending committee order (the spec's get_attesting_indices:
 * a running committee_offset, member i of a committee takes part iff
 * aggregation_bits[committee_offset + i]).  Committee c of the list owns the bits
 * [off_c, off_c + n_c), off_c = n_0 + ... + n_{c-1}; its member p takes part iff bit off_c + p is
 * set (SSZ bit order).  The list is taken as given: a repeated id counts its selected members
 * again, as an index list with repeats does; ascending order, and the consensus rule that every
 * listed committee has an attester, are the caller's business.  Every committee takes its own
 * shorter side (its selected members, or its total minus the unselected ones).
 * n_committees == 0: the set's own pk_indices / pk_bytes count; n_committees == 1 is exactly
 * bgv_pkbits {committees[0], n_bits, bits}. */
#define BGV_MAX_SET_COMMITTEES 64 /* MAX_COMMITTEES_PER_SLOT */
#define BGV_MAX_SPAN_BITS 131072  /* 64 x 2048, the spec's bound on aggregation_bits */
typedef struct {
  const uint32_t* committees; /* n_committees ids, in bitfield order */
  uint32_t n_committees;      /* 0: the set's own pk_indices / pk_bytes count */
  uint32_t n_bits;            /* sum of the listed committees' lengths */
  const uint8_t* bits;        /* ceil(n_bits / 8) bytes, SSZ bit order */
} bgv_pkspan;

/* bgv_verify_bits / bgv_verify_bits_async with spans[i] beside sets[i] (spans may be NULL:
 * bgv_verify).  A job's code from the host's argument checks of a span set, in this order: an
 * unknown or dropped id anywhere in the list -BGV_E_BAD_INDEX; n_committees >
 * BGV_MAX_SET_COMMITTEES, n_bits > BGV_MAX_SPAN_BITS or n_bits other than the sum of the listed
 * committees' lengths -BGV_E_ARG; a set bit at or past n_bits in the last byte -BGV_E_ARG; no bit
 * set -BGV_E_EMPTY_AGGREGATE; a listed committee that holds a marked key -BGV_E_BAD_INDEX.
 * Everything else is the call with the expanded index list. */
int bgv_verify_spans(bgv_ctx* ctx, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                     const bgv_pkspan* spans, int mode, int32_t* out_job_codes, bgv_stats* stats);
int bgv_verify_spans_async(bgv_ctx* ctx, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                           const bgv_pkspan* spans, int mode, int32_t* out_job_codes, bgv_stats* stats,
                           bgv_done_fn done, void* user);

/* Parity hook: the aggregate of a span's selected members through the verify path's own kernel
 * (k_pk_agg_span, the sides the layout would take; k_pk_agg_bits for one committee), 96-byte
 * uncompressed encoding (0x40 for infinity).  Codes as the set checks above. */
int bgv_aggregate_span(bgv_ctx* ctx, const bgv_pkspan* span, uint8_t out96[96]);

/* Parity hook for bls.PublicKey.aggregate + toBytes(uncompressed)
 * (chain/bls/utils.ts:5-16, multithread/index.ts:160): sum of cached pubkeys,
 * 96-byte uncompressed ZCash encoding (0x40 flag for infinity). */
int bgv_aggregate_pubkeys(bgv_ctx* ctx, const uint32_t* indices, size_t n, uint8_t out96[96]);

/* Parity hook for hash_to_G2 with DST BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_:
 * n messages (concatenated, lengths in lens) -> n x 192-byte uncompressed points
 * (x.c1 | x.c0 | y.c1 | y.c0). */
int bgv_hash_to_g2(bgv_ctx* ctx, const uint8_t* msgs, const uint32_t* lens, size_t n, uint8_t* out192);

/* Multi-GPU: one job's batch equation split over processes -------
 * The reference spreads a call's jobs over worker threads (multithread/index.ts:153-166);
 * here ONE job (e.g. a whole block range, or config 4 mode (ii)) can span GPUs.  Each rank
 * passes its shard of the job's sets to bgv_verify_partial, which returns the shard's
 * randomized Miller-loop product
 *     prod_i e(r_i pk_i, H(m_i)) * e(-G1, sum_i r_i sig_i)       (before the final exponentiation)
 * as 576 canonical big-endian bytes (the 12 Fp coefficients in tower order), and
 *     out_codes[0] = first signature error in set order (-BLST code) or 0,
 *     out_codes[1] = first pubkey condition: -BLST code, 1 for an infinity aggregate, or 0.
 * The partials are gathered (RCCL over xGMI, or gloo) and bgv_final_verify multiplies them
 * and runs ONE final exponentiation: *out_verdict = 1 iff the product is 1 in GT.
 * The job's outcome is then: the first nonzero signature code in rank order, else the
 * first pubkey code (1 = infinity aggregate: BLST_PK_IS_INFINITY for >= 2 sets, false for
 * one), else the verdict (lodestar_amd/shard.py). */
int bgv_verify_partial(bgv_ctx* ctx, const bgv_set* sets, size_t nsets, uint8_t out576[576], int32_t out_codes[2]);
/* One process over several devices: a context created on a device list spreads every
 * bgv_verify / bgv_verify_async call of at least min_sets sets over its devices -- a job of
 * at least min_sets sets as one run of sets per device whose Fp12 partials are combined with
 * one final exponentiation, the other jobs in contiguous runs pinned to one device each
 * (chain/bls/multithread/index.ts:153-166 splits big calls over workers the same way).
 * Codes are those of the unsplit call.  Default 4096 (BGV_SPLIT_MIN env); 0 disables. */
int bgv_set_split(bgv_ctx* ctx, uint32_t min_sets);
int bgv_final_verify(bgv_ctx* ctx, const uint8_t* partials, size_t n, int32_t* out_verdict);

/* Parity hook (tests only): the per-set intermediates of a verify call's kernels with the
 * path forced, so the latency path (which serves every call of up to 16,384 pairs: gossip,
 * block import) is checked byte for byte against the bulk path and the hash_to_G2 goldens.
 *   path 1 (BGV_PATH_BULK)     k_prep (task_hash/task_sig/task_pk), k_lines + k_facc one pair per lane
 *   path 2 (BGV_PATH_LATENCY)  k_prep_a + k_prep_team, k_miller_team
 * The n sets (cached pubkeys only) form one job in groups of 64; set i gets the i-th nonzero
 * splitmix64 output from `seed` as its randomizer, so both paths see the same r_i.
 *   out_h192[i]    H(m_i), serialized like bgv_hash_to_g2
 *   out_f576[i]    its Miller-loop value f_i = e(r_i pk_i, H(m_i)) before the final
 *                  exponentiation (12 canonical big-endian Fp coefficients, tower order; 1 when
 *                  the set takes no part)
 *   out_status[2i], [2i+1]  the set's signature / pubkey status (0, 100 = infinity, or BLST code) */
#define BGV_PATH_BULK 1
#define BGV_PATH_LATENCY 2
int bgv_debug_prepare(bgv_ctx* ctx, const bgv_set* sets, size_t nsets, int path, uint64_t seed, uint8_t* out_h192,
                      uint8_t* out_f576, int32_t* out_status);

/* Parity hook for uniform groups (tests only; bgv_host_layout.h layout_call / bgv_retry_plan.h build_parts).
 * The n sets (2..64, cached pubkeys, one signing root, 96-B signatures) form ONE uniform
 * first-pass group of a bulk batch, randomizers as bgv_debug_prepare's; then ntests retry tests
 * over its slots, each a slot mask (bit k = set k), weighted (slot k with weight k + 1,
 * BGV_GROUP_WEIGHTED) when test_weighted[t] != 0.  Replaces the per-set pairs of a group whose
 * sets share a root, prod_i e(r_i pk_i, H) = e(sum_i r_i pk_i, H):
 *   out_first576       MillerLoop(sum_i r_i pk_i, H)                (k_gsum -> k_lines / k_facc)
 *   out_pk576[t]       MillerLoop(sum_{i in t} w_i r_i pk_i, H)     (k_gsum / k_gsum_w -> k_miller_team)
 *   out_sig576[t]      MillerLoop(-G1, sum_{i in t} w_i r_i sig_i)  (the test's signature pair)
 * 576-byte values as bgv_debug_prepare's f; w_i = 1, or i + 1 in a weighted test. */
int bgv_debug_uniform(bgv_ctx* ctx, const bgv_set* sets, size_t nsets, uint64_t seed, const uint64_t* test_masks,
                      const uint32_t* test_weighted, size_t ntests, uint8_t* out_first576, uint8_t* out_pk576,
                      uint8_t* out_sig576);

/* SURVEY 8(f) rows beside the verify path -------------------------------- */

/* Deposit-time pubkey validation: bls.PublicKey.fromBytes(pubkey, CoordType.affine,
 * validate=true) (state-transition/src/block/processDeposit.ts:64) for n 48-byte
 * compressed keys.  out_status[i] = 0 or -BLST code (BAD_ENCODING, POINT_NOT_ON_CURVE,
 * PK_IS_INFINITY, POINT_NOT_IN_GROUP).  out96 (may be NULL) receives the 96-byte
 * uncompressed record of every valid key (bgv_pubkeys_put / bgv_set.pk_bytes format) and the
 * infinity record (0x40, then zeros) for every other key, a decodable one outside G1 included. */
int bgv_pubkeys_validate(bgv_ctx* ctx, const uint8_t* keys48, size_t n, int32_t* out_status, uint8_t* out96);

/* Op-pool signature aggregation: bls.Signature.aggregate(sigs.map(s =>
 * Signature.fromBytes(s, undefined, true))) (chain/opPools/attestationPool.ts:184-187,
 * aggregatedAttestationPool.ts:319-321, syncCommitteeMessagePool.ts:126-129,
 * syncContributionAndProofPool.ts:181-185).  naggs aggregates over consecutive runs of
 * counts[a] signatures (96-byte records, lens[i] = the received length).  out96[a] is the
 * compressed aggregate, out_status[a] 0, -BLST code of the first signature that fails,
 * or -BGV_E_EMPTY_AGGREGATE for an empty run. */
int bgv_aggregate_signatures(bgv_ctx* ctx, const uint8_t* sigs96, const uint32_t* lens, const uint32_t* counts,
                             size_t naggs, uint8_t* out96, int32_t* out_status);

/* Verify and aggregate: bgv_verify_spans whose call also returns, per caller-chosen pool key, the
 * compressed sum of the signatures it accepted.  Replaces the gossip handlers' pair of steps
 * (network/gossip/handlers/index.ts:199,285): verifySignatureSets([set], {batchable: true}), then
 * on the main thread Signature.aggregate([aggregate.signature, Signature.fromBytes(sig, undefined,
 * true)]) in the op pool (chain/opPools/attestationPool.ts:184-187,
 * syncCommitteeMessagePool.ts:126-129), which decodes and subgroup-checks every signature a second
 * time.  Here the verdict pass has proved membership, so the second decoding is the square root
 * alone.
 *   out_job_codes    exactly those of bgv_verify_spans on the same arguments (spans may be NULL)
 *   agg_of_set[i]    the aggregate set i belongs to (< naggs), or BGV_NO_AGG
 * Set i is accepted iff the code of the job that holds it is 1.  Aggregate a is the G2 sum of the
 * signatures of the accepted sets with agg_of_set[i] == a, whatever their order or spacing; a
 * repeated signature counts again, an infinity signature adds nothing and is counted.
 *   out_agg_count[a]   how many sets were summed
 *   out_agg_status[a]  0, -BGV_E_EMPTY_AGGREGATE when the count is 0, or -code when an accepted
 *                      signature no longer decodes (the caller changed the buffer)
 *   out_agg96[a]       the compressed sum, byte for byte bgv_aggregate_signatures' over the same
 *                      signatures (the infinity encoding for a sum at infinity); zero when the
 *                      status is not 0
 * -BGV_E_ARG, nothing run and no output written: an agg_of_set[i] that is neither BGV_NO_AGG nor
 * < naggs, naggs > 2^20, a null pointer that is needed.  naggs == 0 is bgv_verify_spans.
 * When the call fails (a negative return) the aggregate outputs are not written.
 * The signatures are read from sets[i].sig once the codes are final: the caller keeps them alive
 * and unchanged until the call returns (until done() in the asynchronous form, which fires on a
 * worker thread of the context after the aggregates are written; bgv_close ends a call whose
 * aggregation is still queued with -BGV_E_CLOSED).
 * Calls with at most BGV_SIGAGG_WAVE_MAX accepted signatures decode one signature per wavefront,
 * larger ones one per lane. */
#define BGV_NO_AGG 0xFFFFFFFFu
#define BGV_SIGAGG_WAVE_MAX 2048
int bgv_verify_aggregate(bgv_ctx* ctx, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                         const bgv_pkspan* spans, int mode, const uint32_t* agg_of_set, size_t naggs,
                         int32_t* out_job_codes, uint8_t* out_agg96, int32_t* out_agg_status, uint32_t* out_agg_count,
                         bgv_stats* stats);
int bgv_verify_aggregate_async(bgv_ctx* ctx, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                               const bgv_pkspan* spans, int mode, const uint32_t* agg_of_set, size_t naggs,
                               int32_t* out_job_codes, uint8_t* out_agg96, int32_t* out_agg_status,
                               uint32_t* out_agg_count, bgv_stats* stats, bgv_done_fn done, void* user);

/* Parity hook (tests only): how many aggregation steps of bgv_verify_aggregate calls on this context
 * have launched the one-signature-per-wavefront decoding (out[0]) and the one-per-lane decoding
 * (out[1]); a call that accepted nothing launches neither. */
int bgv_debug_sigagg_launches(bgv_ctx* ctx, uint64_t out[2]);

/* Device-resident signature pools: the op pools' running aggregate per (slot, data root), kept on
 * device 0 and fed by verify calls.  Replaces, after every gossip verify call, the op pool's
 * Signature.fromBytes of the 96 bytes bgv_verify_aggregate returned (an Fp2 square root on the main
 * thread) and its Signature.aggregate([aggregate.signature, signature]) into the running aggregate
 * (chain/opPools/attestationPool.ts:184-187, syncCommitteeMessagePool.ts:126-129), and the
 * toBytes() of getAggregate: the node sends bytes, gets verdicts, and reads 96 bytes once, when an
 * aggregator asks.  A pool entry is a G2 accumulator with a count; the caller chooses its id
 * (0 .. BGV_MAX_SIGPOOL - 1).
 *
 * bgv_sigpool_open: the entry starts empty (infinity, count 0).  -BGV_E_ARG for an id that is live
 * or >= BGV_MAX_SIGPOOL.  Replaces the pool's aggregate creation on the first message of a key
 * (attestationPool.ts aggregateAttestationInto's counterpart for a new data root).
 *
 * bgv_sigpool_drop_range: drops the live entries of ids first_id .. first_id + count - 1 and returns
 * how many there were (>= 0); a dropped id may be opened again at once.  Replaces the pools' prune()
 * of old slots.
 *
 * bgv_sigpool_get: reads n entries without changing them (ids may repeat).  An id >=
 * BGV_MAX_SIGPOOL gives -BGV_E_ARG and nothing is written.  Per id:
 *   not live    out_status -BGV_E_BAD_INDEX,        out_count 0, out96 zero
 *   count 0     out_status -BGV_E_EMPTY_AGGREGATE,  out_count 0, out96 zero
 *   otherwise   out_status 0, the entry's count, the compressed sum: byte for byte
 *               bgv_aggregate_signatures' over the same signatures (the infinity encoding for a sum
 *               at infinity)
 * Replaces AttestationPool.getAggregate / SyncCommitteeMessagePool.getContribution's
 * signature.toBytes().
 *
 * bgv_verify_accumulate: bgv_verify_spans whose accepted signatures are added to pool entries.
 * Replaces verifySignatureSets followed by AttestationPool.add / SyncCommitteeMessagePool.add's
 * curve arithmetic (network/gossip/handlers/index.ts:199,285).
 *   out_job_codes    exactly those of bgv_verify_spans on the same arguments (spans may be NULL)
 *   pool_of_set[i]   the entry set i is added to, or BGV_NO_AGG; NULL: the call is bgv_verify_spans
 *   out_added[i]     (may be NULL) 1 iff set i was added
 * All tags are checked at submit: one that is neither BGV_NO_AGG nor < BGV_MAX_SIGPOOL gives
 * -BGV_E_ARG; otherwise one that names an entry that is not live gives -BGV_E_BAD_INDEX; in both
 * cases nothing runs and no output is written.  A tag on an entry that has bits
 * (bgv_sigpool_open_bits) gives -BGV_E_ARG in the same way: such an entry is fed by
 * bgv_verify_accumulate_bits alone.  Set i is added iff the code of the job that holds
 * it is 1, it is tagged, and its entry is still the one that was open at submit: an entry dropped
 * since, or dropped and opened again, receives nothing from this call.  As in bgv_verify_aggregate a
 * repeated signature counts again, an infinity signature adds nothing and is counted, and the
 * signatures are read from sets[i].sig once the codes are final: the caller keeps them alive and
 * unchanged until the call returns (until done() in the asynchronous form).  If a member no longer
 * decodes, its entry is left exactly as it was and none of that entry's sets of this call count as
 * added.  A failed call (negative return) changes no entry.  Every accepted signature is added
 * exactly once, whatever retry rounds, split calls or merged super-batches the verdicts went through.
 * Accumulation steps of one context are serialised with each other and with get / drop: after a
 * synchronous call returns, or an asynchronous call's done() has fired (on a worker thread of the
 * context), bgv_sigpool_get sees that call's additions.  bgv_close ends a call whose step is still
 * queued with -BGV_E_CLOSED: the codes stand, the entries are not written.
 * The decoding form is bgv_verify_aggregate's: at most BGV_SIGAGG_WAVE_MAX added signatures decode
 * one per wavefront, more one per lane. */
#define BGV_MAX_SIGPOOL 16384 /* ids 0..16383 */
int bgv_sigpool_open(bgv_ctx* ctx, uint32_t id);
int bgv_sigpool_drop_range(bgv_ctx* ctx, uint32_t first_id, uint32_t count);
int bgv_sigpool_get(bgv_ctx* ctx, const uint32_t* ids, size_t n, uint8_t* out96, uint32_t* out_count,
                    int32_t* out_status);
int bgv_verify_accumulate(bgv_ctx* ctx, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                          const bgv_pkspan* spans, int mode, const uint32_t* pool_of_set, int32_t* out_job_codes,
                          uint8_t* out_added, bgv_stats* stats);
int bgv_verify_accumulate_async(bgv_ctx* ctx, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                                const bgv_pkspan* spans, int mode, const uint32_t* pool_of_set,
                                int32_t* out_job_codes, uint8_t* out_added, bgv_stats* stats, bgv_done_fn done,
                                void* user);

/* Parity hook (tests only): how many accumulation steps on this context have launched the
 * one-signature-per-wavefront decoding (out[0]) and the one-per-lane decoding (out[1]); a step that
 * adds nothing launches neither. */
int bgv_debug_sigpool_launches(bgv_ctx* ctx, uint64_t out[2]);

/* Pool entries with participation bits: the aggregate's bitfield beside its signature, so an entry
 * refuses a member it already holds and bits and signature change in one step.  Replaces the bit
 * handling of aggregateAttestationInto (chain/opPools/attestationPool.ts:171-189: AlreadyKnown when
 * the bit is set) and of MatchingDataAttestationGroup.add (aggregatedAttestationPool.ts:231-275,
 * 315-322: AlreadyKnown for a subset, aggregateInto only for disjoint bitfields), which the host
 * cannot do at submit: two calls in flight may carry the same attester, and only the accumulation
 * step sees final codes one call at a time.
 *
 * bgv_sigpool_open_bits: bgv_sigpool_open for an entry that also holds a field of n_bits positions
 * (1 .. BGV_SIGPOOL_MAX_BITS), all clear; another n_bits gives -BGV_E_ARG.  The field lives in the
 * host registry (the plan needs it before anything is decoded); bgv_sigpool_drop_range and a reopen
 * clear it, and a reopen may choose another n_bits or none (bgv_sigpool_open).
 *
 * bgv_verify_accumulate_bits: bgv_verify_accumulate with bits_of_set[i], the positions set i stands
 * for in its entry: bits == NULL names the single position `bit`, otherwise bits is a field of
 * ceil(n_bits / 8) bytes in SSZ bit order (position k is bit k % 8 of byte k / 8).  The tag checks of
 * bgv_verify_accumulate run first and are unchanged.  Then, for every tagged set whose entry has
 * bits, -BGV_E_ARG when bits_of_set is NULL, n_bits is not the entry's, the single position is not
 * below n_bits, or the field has a bit at or past n_bits or no bit at all; nothing runs and nothing
 * is written.  bits_of_set[i] of an untagged set or of a plain entry's set is ignored, and such a
 * set behaves exactly as under bgv_verify_accumulate.  The fields are copied at submit: the caller
 * need not keep them.  (bgv_verify_accumulate itself gives -BGV_E_ARG at submit for a tag on an
 * entry that has bits.)
 *   out_job_codes   exactly those of bgv_verify_spans
 *   out_outcome[i]  (may be NULL) BGV_POOL_*
 * The step takes an entry's members in set order.  With B the entry's field as the step finds it
 * plus what earlier sets of this call added, and M the member's: M & B == 0 adds the signature,
 * B |= M, BGV_POOL_ADDED; otherwise M within B is BGV_POOL_KNOWN (InsertOutcome.AlreadyKnown) and
 * anything else BGV_POOL_OVERLAP (the reference's NotBetterThan / no aggregateInto); neither touches
 * the entry.  BGV_POOL_NOT_ADDED: an untagged set, a set of a job whose code is not 1, a set whose
 * entry changed generation since submit.  A set of a plain entry gets BGV_POOL_ADDED or
 * BGV_POOL_NOT_ADDED as out_added would.  Only members to be added are uploaded and decoded (the
 * decoding form follows their number), and a step with nothing to add does no device work.  Field and
 * count are committed after the device's flags are back: an entry with a member that no longer
 * decodes keeps its field, count and accumulator, and all of its sets of this call report
 * BGV_POOL_NOT_ADDED.  Everything else is as stated for bgv_verify_accumulate: every accepted
 * signature is added at most once, steps are serialised with get / drop / sum, bgv_close ends a
 * queued step with -BGV_E_CLOSED, done() fires on a worker thread of the context.
 *
 * bgv_sigpool_get_bits: bgv_sigpool_get plus, per id, the entry's field in out_bits (n x
 * BGV_SIGPOOL_BITS_BYTES, zero padded) and its n_bits in out_nbits (0 for a plain or not-live
 * entry).  An empty live entry gives -BGV_E_EMPTY_AGGREGATE, zero bits and its n_bits.  Signature,
 * count and field are read in one step: they always agree.
 *
 * bgv_sigpool_sum: the sum of entries, per group of 1 .. BGV_MAX_SUM_ENTRIES ids; reads entries and
 * changes none.  Replaces SyncContributionAndProofPool's aggregate over the best contribution of
 * each subnet (syncContributionAndProofPool.ts:169-187) and the EIP-7549 consolidation of one
 * AttestationData's committee aggregates: one bgv_sigpool_get per entry (an inversion and a
 * compression each) followed by bgv_aggregate_signatures over the bytes (a square root and a
 * subgroup check each).  The device reads 288 B per entry and writes 96 B per group.
 * -BGV_E_ARG and nothing written: ngroups > 65536, an n_ids of 0 or above BGV_MAX_SUM_ENTRIES, an
 * id >= BGV_MAX_SIGPOOL, a needed pointer that is NULL (out_bits alone may be), out_bits with a
 * bits_stride below ceil(sum of the group's n_bits / 8) for some group.  Per group:
 *   an id not live  out_status -BGV_E_BAD_INDEX, every other output of the group zero
 *   otherwise       out_count the sum of the entries' counts (a repeated id counts again);
 *                   out_nbits the sum of their n_bits; out_bits + g * bits_stride the fields
 *                   concatenated in list order at bit granularity, entry c at [off_c, off_c + n_c)
 *                   with off_c the sum of the n_bits before it (a plain entry owns no position),
 *                   the rest of the stride zero: the get_attesting_indices layout
 *   count 0         out_status -BGV_E_EMPTY_AGGREGATE, out96 zero (bits and out_nbits as above)
 *   count > 0       out_status 0, out96 the compressed G2 sum: byte for byte
 *                   bgv_aggregate_signatures' over every signature held (the infinity encoding for
 *                   a sum at infinity)
 * An opened, empty entry contributes clear positions and no point (a subnet without contribution). */
#define BGV_SIGPOOL_MAX_BITS 2048 /* MAX_VALIDATORS_PER_COMMITTEE */
#define BGV_SIGPOOL_BITS_BYTES 256
#define BGV_MAX_SUM_ENTRIES 64 /* = BGV_MAX_SET_COMMITTEES */
enum { BGV_POOL_NOT_ADDED = 0, BGV_POOL_ADDED = 1, BGV_POOL_KNOWN = 2, BGV_POOL_OVERLAP = 3 };
typedef struct {
  uint32_t n_bits; /* the entry's */
  uint32_t bit;    /* the single position, when bits == NULL */
  const uint8_t* bits;
} bgv_poolbits;
typedef struct {
  const uint32_t* ids;
  uint32_t n_ids;
} bgv_poolgroup;
int bgv_sigpool_open_bits(bgv_ctx* ctx, uint32_t id, uint32_t n_bits);
int bgv_verify_accumulate_bits(bgv_ctx* ctx, const bgv_job* jobs, size_t njobs, const bgv_set* sets, size_t nsets,
                               const bgv_pkspan* spans, int mode, const uint32_t* pool_of_set,
                               const bgv_poolbits* bits_of_set, int32_t* out_job_codes, uint8_t* out_outcome,
                               bgv_stats* stats);
int bgv_verify_accumulate_bits_async(bgv_ctx* ctx, const bgv_job* jobs, size_t njobs, const bgv_set* sets,
                                     size_t nsets, const bgv_pkspan* spans, int mode, const uint32_t* pool_of_set,
                                     const bgv_poolbits* bits_of_set, int32_t* out_job_codes, uint8_t* out_outcome,
                                     bgv_stats* stats, bgv_done_fn done, void* user);
int bgv_sigpool_get_bits(bgv_ctx* ctx, const uint32_t* ids, size_t n, uint8_t* out96, uint32_t* out_count,
                         int32_t* out_status, uint8_t* out_bits, uint32_t* out_nbits);
int bgv_sigpool_sum(bgv_ctx* ctx, const bgv_poolgroup* groups, size_t ngroups, uint8_t* out96, uint32_t* out_count,
                    int32_t* out_status, uint8_t* out_bits, size_t bits_stride, uint32_t* out_nbits);

/* Deposit signature check (processDeposit.ts:62-70): key validated as above, then
 * Signature.fromBytes(sig, affine, true).verify(pk, signingRoot); any BLS error counts
 * as invalid.  out_valid[i] = 1 or 0. */
int bgv_deposits_verify(bgv_ctx* ctx, const uint8_t* keys48, const uint8_t* msgs32, const uint8_t* sigs96, size_t n,
                        int32_t* out_valid);

/* Bench/test utilities (not part of IBlsVerifier): derive public keys and sign on
 * the device.  sks are n x 32-byte big-endian secret keys (SecretKey.fromBytes).
 * bgv_keygen writes n x 48-byte compressed pubkeys to out48 (may be NULL) and, when
 * cache_first >= 0, stores them in the pubkey cache at [cache_first, cache_first + n).
 * bgv_sign writes n x 96-byte compressed signatures sk_i * H(msg_i) (msgs: n x 32 B). */
int bgv_keygen(bgv_ctx* ctx, const uint8_t* sks, size_t n, int64_t cache_first, uint8_t* out48);
int bgv_sign(bgv_ctx* ctx, const uint8_t* sks, const uint8_t* msgs, size_t n, uint8_t* out96);

/* Super-batch geometry: verify calls queued within coalesce_us of each other are merged
 * into one device launch of at most max_batch_slots sets (the GPU form of the pool's
 * MAX_BUFFERED_SIGS / MAX_BUFFER_WAIT_MS and prepareWork packaging,
 * multithread/index.ts:39-57,386-401).  While no super-batch is running the window is
 * idle_coalesce_us instead (at most coalesce_us), so a lone call launches at once.
 * max_batch_slots = 0 and a window of UINT32_MAX leave a value unchanged.  Defaults:
 * 131072 sets, 500 us, 50 us (env BGV_MAX_BATCH_SLOTS, BGV_COALESCE_US,
 * BGV_IDLE_COALESCE_US). */
int bgv_set_batching(bgv_ctx* ctx, uint32_t max_batch_slots, uint32_t coalesce_us, uint32_t idle_coalesce_us);

/* Deterministic batch randomizers for tests (seed != 0: splitmix64 stream;
 * seed == 0: getrandom(), the default). */
int bgv_set_rng_seed(bgv_ctx* ctx, uint64_t seed);

/* Per-kernel device time (HIP events between the kernels of each verify launch).
 * Reads the accumulated milliseconds per kernel (kernel_ms[n], names[n], launches)
 * and then, if enable >= 0, resets the counters and switches event recording on (1)
 * or off (0).  Returns the number of kernels in a verify launch. */
int bgv_profile(bgv_ctx* ctx, int enable, double* kernel_ms, const char** names, int n, uint64_t* launches);

/* Human-readable name of a status code ("BLST_INVALID_SIZE", ...). */
const char* bgv_strerror(int code);

int bgv_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* BLSGPU_H */
