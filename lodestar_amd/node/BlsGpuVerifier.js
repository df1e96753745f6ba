"use strict";
/**
 * BlsGpuVerifier — IBlsVerifier (packages/beacon-node/src/chain/bls/interface.ts:20-46) on MI355X.
 *
 * Drop-in beside BlsMultiThreadWorkerPool (chain/bls/multithread/index.ts:98-424): the same
 * verifySignatureSets(sets, opts) -> Promise<boolean> and close() -> Promise<void>, the same
 * batchable buffering (index.ts:238-285, 406-412), 128-set jobs (index.ts:39,155-166) and
 * QUEUE_ABORTED after close (index.ts:176-197, 239-241).  Per-job verification, batching and
 * retry run on the GPU (libblsgpu, BGV_MODE_WORKER), so every job's verdict matches the worker's.
 *
 * Pubkeys are validator indices into the device-resident cache (SURVEY §7 "pubkey identity at
 * the boundary", option (a)): set.pubkey / set.pubkeys hold numbers (or {index}).
 *
 * Metrics: with modules.metrics (the beacon node's IMetrics) the verifier feeds the same
 * bls / blsThreadPool series as the pool (metrics/metrics/lodestar.ts:405-494, updated at
 * multithread/index.ts:129-130,136-151,317-367); the whole device is worker 0, and the
 * per-call device time stands in for the worker job time.  latencyToWorker/FromWorker
 * (structured-clone messaging) have no GPU counterpart and are not observed.
 */
const crypto = require("crypto");
const path = require("path");
const addon = require(path.join(__dirname, "blsgpu.node"));

const MAX_SIGNATURE_SETS_PER_JOB = 128; // index.ts:39
// Batchable buffering (index.ts:48,57 use 32 sets / 100 ms for CPU workers).  Gossip caps
// concurrency per topic (64 for attestations, network/gossip/validation/queue.ts:14), so the
// Node-level rate is concurrency / per-call latency: a long buffer wait only adds latency,
// and the library already merges the calls in flight into super-batches.  The flush test is
// the reference's `sigCount > maxBufferedSigs`, so 63 sends the buffer the moment a full
// queue's 64 sets are in it; at 64 every batch waited for the timer.  Measured with 64
// concurrent one-set callers on one MI355X (tests/node/gossip_bench.js,
// profiles/r03/gossip/flush_at_callers.jsonl): 63 / 1 ms 11.6k sets/s at p50 5.4 ms,
// 64 / 1 ms 9.9k at 6.4 ms, 32 / 100 ms 6.2k at 10.3 ms (14.2k at 4.4 ms for 63 / 1 ms with
// the later device chain, profiles/r03/gossip/two_wave_miller.jsonl).
const MAX_BUFFERED_SIGS = 63;
const MAX_BUFFER_WAIT_MS = 1;
// canAcceptWork() turns false while this many sets are queued or in flight: one default
// super-batch (131,072 sets) running and one forming.  A default, not a tuned number.
const MAX_INFLIGHT_SIGS = 262144;

// committee: not in the reference -- an aggregate as the beacon node holds it before
// bits.intersectValues(committeeIndices): a committee stored on the device (committeePut) and
// the participation bitfield; committees: one bitfield over several such committees in order
// (an attestation since EIP-7549: committee_bits -> ids, aggregation_bits)
const SignatureSetType = {single: "single", aggregate: "aggregate", committee: "committee", committees: "committees"};
const PUBKEY_RUN = 8192;
const NO_PROPOSER = 0xffffffff; // BGV_NO_PROPOSER
// include/blsgpu.h: BGV_BLST_* decode statuses are 1..19 (library codes start at 20)
const toUint8Array = (v) => (v instanceof Uint8Array ? v : Uint8Array.from(v));
// effectiveBalanceIncrements for the sampling rule: bytes under "phase0"; under "electra" a
// Uint16Array, with a Uint8Array or a number array widened element by element (never
// reinterpreted) and numbers that do not fit 16 bits refused, not wrapped
function samplingTable(v, rule) {
  if (rule === undefined || rule === "phase0") return toUint8Array(v);
  if (rule !== "electra") throw new TypeError(`blsgpu: unknown sampling rule ${rule}`);
  if (v instanceof Uint16Array) return v;
  if (!(v instanceof Uint8Array) && !Array.isArray(v))
    throw new TypeError("blsgpu: effectiveBalanceIncrements must be a Uint16Array, a Uint8Array or a number array");
  const out = new Uint16Array(v.length);
  for (let i = 0; i < v.length; i++) {
    if (!Number.isInteger(v[i]) || v[i] < 0 || v[i] > 0xffff)
      throw new RangeError(`blsgpu: effectiveBalanceIncrements[${i}] = ${v[i]} does not fit 16 bits`);
    out[i] = v[i];
  }
  return out;
}
const isBlstDecodeCode = (code) => typeof code === "number" && code <= -1 && code >= -19;

// One contiguous run of queued validator keys: indices [first, first + n), their 48-byte
// encodings packed in order into bytes (capacity doubles up to PUBKEY_RUN keys).
class PubkeyRun {
  constructor(first) {
    this.first = first;
    this.n = 0;
    this.bytes = new Uint8Array(48 * 64);
  }
  push(pubkey) {
    if (48 * (this.n + 1) > this.bytes.length) {
      const b = new Uint8Array(Math.min(2 * this.bytes.length, 48 * PUBKEY_RUN));
      b.set(this.bytes.subarray(0, 48 * this.n));
      this.bytes = b;
    }
    this.bytes.set(pubkey, 48 * this.n);
    this.n++;
  }
}

class QueueError extends Error {
  constructor(code) {
    super(code);
    this.type = {code};
  }
}

/** chain/bls/multithread/utils.ts:4-19 */
function chunkifyMaximizeChunkSize(arr, minPerChunk) {
  const chunkCount = Math.floor(arr.length / minPerChunk);
  if (chunkCount <= 1) return [arr];
  const perChunk = Math.ceil(arr.length / chunkCount);
  const out = [];
  for (let i = 0; i < arr.length; i += perChunk) out.push(arr.slice(i, i + perChunk));
  return out;
}

/** chain/bls/utils.ts:18-26 */
function getAggregatedPubkeysCount(sets) {
  let n = 0;
  for (const s of sets) {
    if (s.type === SignatureSetType.aggregate) n += s.pubkeys.length;
    else if (s.type === SignatureSetType.committee || s.type === SignatureSetType.committees)
      n += countBits(committeeBits(s).bits);
  }
  return n;
}

// The bitfield of a committee set: `bits` is a Uint8Array of ceil(nBits / 8) bytes in SSZ bit
// order (member k takes part iff (bits[k >> 3] >> (k & 7)) & 1) with `nBits` beside it, or a
// BitArray ({uint8Array, bitLen}: an attestation's aggregationBits, a syncCommitteeBits).
function committeeBits(s) {
  const bits = s.bits.uint8Array || s.bits;
  const nBits = s.nBits !== undefined ? s.nBits : s.bits.bitLen !== undefined ? s.bits.bitLen : 8 * bits.length;
  return {bits, nBits};
}

function countBits(bytes) {
  let n = 0;
  for (let b of bytes) for (; b; b &= b - 1) n++;
  return n;
}

function indexOf(pk) {
  return typeof pk === "number" ? pk : pk.index;
}

// A pubkey is a validator index (a number, or a PublicKey tagged with .index by the
// Index2PubkeyCache, INTEGRATION.md), else its 96-B uncompressed bytes (pk.toBytes(false)
// for @chainsafe/bls keys outside the cache, e.g. deposits).
function uncompressed(pk) {
  if (pk instanceof Uint8Array) return pk;
  return pk.toBytes(false);
}

function toNativeSet(s) {
  if (s.type === SignatureSetType.committee) {
    const {bits, nBits} = committeeBits(s);
    return {committee: s.committee, bits, nBits, msg: s.signingRoot, sig: s.signature};
  }
  if (s.type === SignatureSetType.committees) {
    const {bits, nBits} = committeeBits(s);
    return {committees: Uint32Array.from(s.committees), bits, nBits, msg: s.signingRoot, sig: s.signature};
  }
  let pks;
  if (s.type === SignatureSetType.single) pks = [s.pubkey];
  else if (s.type === SignatureSetType.aggregate) pks = s.pubkeys;
  else throw Error("Unknown signature set type");
  if (pks.every((pk) => indexOf(pk) !== undefined)) {
    return {pkIndices: Uint32Array.from(pks, indexOf), msg: s.signingRoot, sig: s.signature};
  }
  const bytes = new Uint8Array(96 * pks.length);
  pks.forEach((pk, i) => bytes.set(uncompressed(pk), 96 * i));
  return {pkBytes: bytes, msg: s.signingRoot, sig: s.signature};
}

class BlsGpuVerifier {
  constructor(opts = {}, modules = {}) {
    this.metrics = modules.metrics || null;
    this.ctx = opts.ctx || addon.init(opts.devices || []);
    this.pendingRuns = []; // PubkeyRun in hook order
    this.pendingKeys = 0;
    this.flushing = null;
    this.onPubkeyError = opts.onPubkeyError || null;
    this.blsVerifyAllMultiThread = opts.blsVerifyAllMultiThread || false;
    this.maxBufferedSigs = opts.maxBufferedSigs || MAX_BUFFERED_SIGS;
    this.maxBufferWaitMs = opts.maxBufferWaitMs || MAX_BUFFER_WAIT_MS;
    this.maxInflightSigs = opts.maxInflightSigs || MAX_INFLIGHT_SIGS;
    this.inflightSigs = 0; // sets queued, buffered or in a device call
    this.jobs = [];
    this.bufferedJobs = null;
    this.closed = false;
    this.counters = {aggregatedPubkeys: 0, batchRetries: 0, successJobsSignatureSetsCount: 0, errorJobsSignatureSetsCount: 0};
    const metrics = this.metrics;
    if (metrics) {
      metrics.blsThreadPool.queueLength.addCollect(() => metrics.blsThreadPool.queueLength.set(this.jobs.length));
    }
  }

  /**
   * Index2PubkeyCache growth -> device cache (INTEGRATION.md §2): a function for
   * state-transition's pubkey-added hook, called with (index, 48-byte pubkey, PublicKey).  It
   * tags the PublicKey with .index (so sets built by the reference's producers travel as
   * indices) and queues the key; queued keys go to the device in contiguous runs before the
   * next verification or every 65,536 keys, off the event loop (flushPubkeys).
   */
  pubkeyAddedHook() {
    return (index, pubkey, pk) => {
      if (pk && typeof pk === "object") pk.index = index;
      // packed into its run here, in the caller's time (the state transition adds keys one at a
      // time), so a flush hands whole runs to the addon without touching each key again
      let r = this.pendingRuns[this.pendingRuns.length - 1];
      if (!r || r.first + r.n !== index || r.n >= PUBKEY_RUN) {
        r = new PubkeyRun(index);
        this.pendingRuns.push(r);
      }
      r.push(pubkey);
      this.pendingKeys++;
      // a gap error here reappears at the next verifySignatureSets, which awaits the flush
      if (this.pendingKeys >= 65536) this.flushPubkeys().catch(() => {});
    };
  }

  /**
   * Uploads the queued keys in contiguous runs with the addon's asynchronous put (a libuv pool
   * thread decodes them; the library publishes a run once every device holds it, without
   * waiting for running verifies), so a validator-set growth never stalls the event loop
   * (EpochContext.addPubkey, state-transition/src/cache/epochContext.ts:702-705;
   * pubkeyCache.ts:56-77).  One flush chain at a time; keys queued meanwhile join it.
   * Only a run whose records fail to decode (a BLST status) is committed -- with those indices
   * marked, so sets naming them reject BGV_E_BAD_INDEX -- then reported once (onPubkeyError,
   * else a console warning) and dropped, so one bad key cannot stop later uploads or
   * verification.  Any other failure (a gap in the indices, a device or memory error) wrote
   * nothing: that run stays queued with every run after it, and the error reaches the caller.
   * The runs are packed as the hook receives the keys, so the event loop only sorts a few run
   * records here and hands the addon views of their bytes (the addon holds a reference to each
   * until its put completes).
   */
  flushPubkeys() {
    if (this.closed) return Promise.resolve();
    if (!this.flushing && this.pendingRuns.length) {
      this.flushing = this._flushRuns().finally(() => {
        this.flushing = null;
      });
    }
    return this.flushing || Promise.resolve();
  }

  async _flushRuns() {
    while (this.pendingRuns.length && !this.closed) {
      const runs = this.pendingRuns;
      this.pendingRuns = [];
      this.pendingKeys = 0;
      let sorted = true;
      for (let k = 1; k < runs.length && sorted; k++) sorted = runs[k].first > runs[k - 1].first;
      if (!sorted) runs.sort((a, b) => a.first - b.first);
      let i = 0;
      try {
        for (; i < runs.length; i++) {
          const r = runs[i];
          try {
            await addon.pubkeysPutAsync(this.ctx, r.first, r.bytes.subarray(0, 48 * r.n), 48);
          } catch (e) {
            if (!isBlstDecodeCode(e.bgvCode) || this.closed) throw e;
            this.reportPubkeyError(e, r.first, r.n);
          }
        }
      } finally {
        if (i < runs.length) {
          this.pendingRuns = runs.slice(i).concat(this.pendingRuns);
          this.pendingKeys = this.pendingRuns.reduce((a, r) => a + r.n, 0);
        }
      }
    }
  }

  reportPubkeyError(e, first, n) {
    const msg = `BlsGpuVerifier: pubkeys [${first}, ${first + n}) uploaded with undecodable keys marked: ${e.message}`;
    if (this.onPubkeyError) this.onPubkeyError(e, first, n);
    else console.warn(msg);
  }

  async verifySignatureSets(sets, opts = {}) {
    if (this.pendingRuns.length || this.flushing) await this.flushPubkeys();
    const nAgg = getAggregatedPubkeysCount(sets);
    this.counters.aggregatedPubkeys += nAgg;
    if (this.metrics) this.metrics.bls.aggregatedPubkeys.inc(nAgg);
    if (opts.verifyOnMainThread && !this.blsVerifyAllMultiThread) {
      // index.ts:138-151: one job verified at once (no buffering)
      const timer = this.metrics ? this.metrics.blsThreadPool.mainThreadDurationInThreadPool.startTimer() : null;
      this.inflightSigs += sets.length;
      try {
        const codes = await addon.verify(this.ctx, [{sets: sets.map(toNativeSet), batchable: false}], 1);
        return unwrap(codes[0]);
      } finally {
        this.inflightSigs -= sets.length;
        if (timer) timer();
      }
    }
    const results = await Promise.all(
      chunkifyMaximizeChunkSize(sets, MAX_SIGNATURE_SETS_PER_JOB).map((chunk) =>
        this.queueBlsWork({opts, sets: chunk.map(toNativeSet)})
      )
    );
    if (results.length === 0) throw Error("Empty results array");
    return results.every((v) => v === true);
  }

  /**
   * IBlsVerifier.verifySignatureSetsSameMessage (chain/bls/interface.ts, from Electra-era
   * versions on): sets of {publicKey, signature} over one signing root, e.g. the unaggregated
   * attestations of one AttestationData.  Every set is its own batchable one-set job over the
   * shared root, so one bad signature costs the others nothing; resolves to one boolean per set.
   * A set whose job ends in an error code (an undecodable signature, an unknown index) is false,
   * as the interface's per-set retry reports it; only a failed call (a closed verifier, a device
   * error) rejects.
   */
  async verifySignatureSetsSameMessage(sets, message, opts = {}) {
    return (await this._sameMessage(sets, message, opts, false)).results;
  }

  /**
   * verifySignatureSetsSameMessage whose device call also sums the signatures it accepted
   * (bgv_verify_aggregate): resolves to {results, signature}, signature the compressed aggregate
   * of the sets whose result is true -- what the op pool's Signature.aggregate would compute after
   * decoding and subgroup-checking each one again (opPools/attestationPool.ts:184-187,
   * syncCommitteeMessagePool.ts:126-129) -- or null when no set was accepted.
   */
  async verifyAndAggregateSameMessage(sets, message, opts = {}) {
    return this._sameMessage(sets, message, opts, true);
  }

  /**
   * verifySignatureSetsSameMessage whose device call also adds the signatures it accepted to the
   * device-resident pool entry poolId (bgv_verify_accumulate; poolOpen, poolGet): resolves to one
   * boolean per set, true iff the set was accepted and added.  The op pool's running aggregate
   * (opPools/attestationPool.ts:184-187, syncCommitteeMessagePool.ts:126-129) then needs no curve
   * arithmetic on the host: the node reads 96 bytes once, when an aggregator asks (poolGet).
   */
  async verifyAndPoolSameMessage(sets, message, poolId, opts = {}) {
    return (await this._sameMessage(sets, message, opts, false, poolId)).results;
  }

  /**
   * verifyAndPoolSameMessage into an entry that holds participation bits (poolOpen(id, {nBits});
   * bgv_verify_accumulate_bits).  Each set is {publicKey, signature} with `bit` (its position in the
   * entry) or `bits` (its field, a Uint8Array of ceil(nBits / 8) bytes in SSZ bit order);
   * opts.nBits is the entry's size.  Resolves to one {valid, outcome} per set: `valid` is the
   * verdict (a known attestation is still a valid gossip message) and `outcome` what the entry did
   * with it: "added" (InsertOutcome.NewData / Aggregated), "known" (AlreadyKnown), "overlap"
   * (NotBetterThan: it shares some position with the entry and brings others), or null when the
   * set was not valid or the entry was dropped meanwhile.  Bits and signature change in one step
   * on the device side, so the pool keeps neither (INTEGRATION.md §2e).
   */
  async verifyAndPoolBitsSameMessage(sets, message, poolId, opts = {}) {
    const members = sets.map((s) =>
      s.bits !== undefined ? {poolNBits: opts.nBits, poolBits: s.bits} : {poolNBits: opts.nBits, poolBit: s.bit}
    );
    return (await this._sameMessage(sets, message, opts, false, poolId, members)).results;
  }

  async _sameMessage(sets, message, opts, aggregate, pool, members) {
    if (this.pendingRuns.length || this.flushing) await this.flushPubkeys();
    if (sets.length === 0) return {results: [], signature: null};
    const native = sets.map((s) =>
      toNativeSet({type: SignatureSetType.single, pubkey: s.publicKey, signingRoot: message, signature: s.signature})
    );
    // one unit in the buffer and one device call, whatever its size; each set its own job there
    return this.queueBlsWork({opts: {...opts, batchable: true}, sets: native, perSet: true, aggregate, pool, members});
  }

  /**
   * Opens the device-resident signature pool entry `id` (0..16383), empty (INTEGRATION.md §2e);
   * with opts.nBits (1..2048) it also holds a participation field of that many positions, all clear.
   */
  poolOpen(id, opts = {}) {
    if (opts.nBits) addon.sigpoolOpenBits(this.ctx, id, opts.nBits);
    else addon.sigpoolOpen(this.ctx, id);
  }

  /** Drops the live entries of ids first .. first + count - 1 (a pruned slot's); returns how many. */
  poolDropRange(first, count) {
    return addon.sigpoolDropRange(this.ctx, first, count);
  }

  /**
   * Reads entries without changing them, off the event loop: per id {status, count, signature},
   * status 0 with the compressed aggregate of the `count` signatures added so far, else a negative
   * library code (not open, or nothing added yet) with signature null.
   */
  async poolGet(ids) {
    const arr = ids instanceof Uint32Array ? ids : Uint32Array.from(ids);
    const {status, count, sigs} = await addon.sigpoolGet(this.ctx, arr);
    return Array.from(arr, (_, k) => ({
      status: status[k],
      count: count[k],
      signature: status[k] === 0 ? sigs.slice(96 * k, 96 * k + 96) : null,
    }));
  }

  /**
   * poolGet plus the entry's participation field: per id {status, count, signature, nBits, bits},
   * bits a Uint8Array of ceil(nBits / 8) bytes (nBits 0 for an entry without bits or not open).
   * Signature, count and bits are read in one step.
   */
  async poolGetBits(ids) {
    const arr = ids instanceof Uint32Array ? ids : Uint32Array.from(ids);
    const r = await addon.sigpoolGetBits(this.ctx, arr);
    return Array.from(arr, (_, k) => poolRecord(r, k));
  }

  /**
   * Sums entries on the device, off the event loop (bgv_sigpool_sum): `groups` is a list of id
   * lists (1..64 ids each); per group {status, count, signature|null, bits, nBits} with the
   * entries' fields concatenated in list order -- SyncContributionAndProofPool's getSyncAggregate
   * over the subnets' best contributions, or the EIP-7549 on-chain attestation of one
   * AttestationData over its committees.  No entry changes.
   */
  async poolSum(groups) {
    const lengths = Uint32Array.from(groups, (g) => g.length);
    const ids = Uint32Array.from([].concat(...groups.map((g) => Array.from(g))));
    const r = await addon.sigpoolSum(this.ctx, ids, lengths);
    return groups.map((_, k) => poolRecord(r, k));
  }

  /** IBlsVerifier.canAcceptWork: false while the sets queued or in flight reach opts.maxInflightSigs. */
  canAcceptWork() {
    return !this.closed && this.inflightSigs < this.maxInflightSigs;
  }

  /**
   * A committee onto the device(s) under `id` (0..16383): its validator indices and their pubkey
   * sum (INTEGRATION.md §2c).  Sets of type "committee" then name it with a bitfield.  The
   * queued pubkeys go first, so a committee of just-added validators finds its keys.
   */
  async committeePut(id, indices) {
    await this.flushPubkeys();
    addon.committeePut(this.ctx, id, indices instanceof Uint32Array ? indices : Uint32Array.from(indices));
  }

  /** Frees the id at once; calls already queued finish on the committee they named. */
  committeeDrop(id) {
    addon.committeeDrop(this.ctx, id);
  }

  /**
   * All committees of one epoch in one call (INTEGRATION.md §2c): the device shuffles
   * `activeIndices` with `seed` (computeEpochShuffling with unshuffleList, over `rounds`
   * swap-or-not rounds), stores the slots * committeesPerSlot committees under firstId,
   * firstId + 1, ... and sums their pubkeys.  Runs off the event loop; resolves to the epoch's
   * shuffling (IEpochShuffling.shuffling).  The queued pubkeys go first.
   */
  async shufflingPut(firstId, seed, activeIndices, slots, committeesPerSlot, rounds) {
    await this.flushPubkeys();
    const active = activeIndices instanceof Uint32Array ? activeIndices : Uint32Array.from(activeIndices);
    return addon.shufflingPut(this.ctx, firstId, seed, active, slots, committeesPerSlot, rounds);
  }

  /**
   * The proposers of `slots` slots from startSlot on (computeProposers, util/seed.ts:22-39) in one
   * device call: the per-slot seeds sha256(epochSeed | LE64(slot)) are hashed here, the balance-
   * weighted sampling (computeProposerIndex) runs on the device off the event loop.  Resolves to a
   * number[] with -1 where every candidate was rejected, as the reference.  The pubkey cache is
   * not involved.  opts.rule: "phase0" (the default: one random byte per candidate, byte
   * increments) or "electra" (EIP-7251: 16 random bits, effectiveBalanceIncrements a Uint16Array
   * or a number array; a Uint8Array is widened).
   */
  async computeProposers(epochSeed, startSlot, activeIndices, effectiveBalanceIncrements, opts) {
    const {slots, maxEffectiveBalanceIncrement, rounds, rule} = opts;
    const seeds = new Uint8Array(32 * slots);
    const msg = Buffer.alloc(40);
    Buffer.from(epochSeed.buffer, epochSeed.byteOffset, epochSeed.byteLength).copy(msg, 0, 0, 32);
    for (let k = 0; k < slots; k++) {
      msg.writeBigUInt64LE(BigInt(startSlot + k), 32);
      seeds.set(crypto.createHash("sha256").update(msg).digest(), 32 * k);
    }
    const active = activeIndices instanceof Uint32Array ? activeIndices : Uint32Array.from(activeIndices);
    const eff = samplingTable(effectiveBalanceIncrements, rule);
    const call = rule === "electra" ? addon.proposersElectra : addon.proposers;
    const out = await call(this.ctx, seeds, active, eff, maxEffectiveBalanceIncrement, rounds);
    return Array.from(out, (v) => (v === NO_PROPOSER ? -1 : v));
  }

  /**
   * The next sync committee in one device call (getNextSyncCommittee, util/syncCommittee.ts:21-38;
   * INTEGRATION.md §2c): the first `size` candidates accepted by balance become committee `id`,
   * repeats kept, on every device, exactly as after committeePut of the same list.  Resolves to
   * {indices: Uint32Array, aggregatePubkey: Uint8Array(48)}.  The queued pubkeys go first.
   * opts.rule as for computeProposers.
   */
  async syncCommitteePut(id, seed, activeIndices, effectiveBalanceIncrements, opts) {
    const {size, maxEffectiveBalanceIncrement, rounds, rule} = opts;
    const eff = samplingTable(effectiveBalanceIncrements, rule);
    await this.flushPubkeys();
    const active = activeIndices instanceof Uint32Array ? activeIndices : Uint32Array.from(activeIndices);
    const call = rule === "electra" ? addon.syncCommitteePutElectra : addon.syncCommitteePut;
    return call(this.ctx, id, seed, active, eff, maxEffectiveBalanceIncrement, size, rounds);
  }

  /** Drops the live ids of firstId .. firstId + count - 1 (an epoch's committees); returns how many. */
  committeeDropRange(firstId, count) {
    return addon.committeeDropRange(this.ctx, firstId, count);
  }

  // index.ts:176-197.  Idempotent; device calls already in flight complete (the library
  // drains them before releasing the context), queued and later jobs reject QUEUE_ABORTED.
  async close() {
    if (this.closed) return;
    if (this.bufferedJobs) clearTimeout(this.bufferedJobs.timeout);
    const pending = this.jobs.concat(this.bufferedJobs ? this.bufferedJobs.jobs : []);
    for (const job of pending) {
      this.inflightSigs -= job.workReq.sets.length;
      job.reject(new QueueError("QUEUE_ABORTED"));
    }
    this.jobs = [];
    this.bufferedJobs = null;
    this.closed = true;
    addon.close(this.ctx);
  }

  queueBlsWork(workReq) {
    if (this.closed) return Promise.reject(new QueueError("QUEUE_ABORTED"));
    return new Promise((resolve, reject) => {
      const job = {resolve, reject, workReq, addedTimeMs: Date.now()};
      this.inflightSigs += workReq.sets.length;
      if (workReq.opts.batchable) {
        // a buffered run holds one kind of caller: a pool caller does not join aggregate callers, nor the reverse
        const kind = callerKind(workReq);
        if (this.bufferedJobs && kind && this.bufferedJobs.kind && this.bufferedJobs.kind !== kind) {
          clearTimeout(this.bufferedJobs.timeout);
          this.runBufferedJobs();
        }
        if (!this.bufferedJobs) {
          this.bufferedJobs = {jobs: [], sigCount: 0, timeout: setTimeout(this.runBufferedJobs, this.maxBufferWaitMs)};
        }
        this.bufferedJobs.jobs.push(job);
        this.bufferedJobs.kind = this.bufferedJobs.kind || kind;
        this.bufferedJobs.sigCount += workReq.sets.length;
        if (this.bufferedJobs.sigCount > this.maxBufferedSigs) {
          clearTimeout(this.bufferedJobs.timeout);
          this.runBufferedJobs();
        }
      } else {
        this.jobs.push(job);
        setImmediate(this.runJob);
      }
    });
  }

  runBufferedJobs = () => {
    if (this.bufferedJobs) {
      this.jobs.push(...this.bufferedJobs.jobs);
      this.bufferedJobs = null;
      setImmediate(this.runJob);
    }
  };

  // Scheduled with setImmediate where index.ts uses setTimeout(runJob, 0): jobs queued in the
  // same macrotask still leave in one call, without Node's 1 ms floor on a zero timeout (a
  // whole millisecond on every gossip batch's critical path).
  // All queued jobs go to the device in one call -- one per kind of caller where runs of both
  // kinds were flushed together; the library merges concurrent calls into super-batches, so there
  // is no idle-worker bookkeeping here (index.ts:290-381).
  runJob = async () => {
    if (this.closed || this.jobs.length === 0) return;
    const all = this.jobs.splice(0, this.jobs.length);
    const calls = [[]];
    let kind = null;
    for (const job of all) {
      const k = callerKind(job.workReq);
      if (k && kind && k !== kind) {
        calls.push([]);
        kind = null;
      }
      kind = kind || k;
      calls[calls.length - 1].push(job);
    }
    await Promise.all(calls.map((jobs) => this.runCall(jobs)));
  };

  runCall = async (jobs) => {
    const m = this.metrics ? this.metrics.blsThreadPool : null;
    let startedSigSets = 0;
    for (const job of jobs) {
      startedSigSets += job.workReq.sets.length;
      if (m) m.jobWaitTime.observe((Date.now() - job.addedTimeMs) / 1000);
    }
    if (m) {
      m.totalJobsGroupsStarted.inc(1);
      m.totalJobsStarted.inc(jobs.length);
      m.totalSigSetsStarted.inc(startedSigSets);
    }
    // A same-message caller's sets travel as one-set jobs from `first` on; with an aggregate
    // wanted they carry an id of their own within this call, with a pool entry named that entry.
    // Without a tagged set the call is addon.verify, exactly as before.
    const nativeJobs = [];
    let naggs = 0;
    let pooled = false;
    let withBits = false; // a run holds one kind of caller: every pool caller of this call has members
    let nsets = 0;
    for (const job of jobs) {
      const w = job.workReq;
      job.first = nativeJobs.length;
      job.firstSet = nsets;
      nsets += w.sets.length;
      if (!w.perSet) {
        nativeJobs.push({sets: w.sets, batchable: Boolean(w.opts.batchable)});
        continue;
      }
      job.agg = w.aggregate ? naggs++ : -1;
      const tag = w.pool !== undefined ? {pool: w.pool} : job.agg >= 0 ? {agg: job.agg} : null;
      pooled = pooled || w.pool !== undefined;
      withBits = withBits || w.members !== undefined;
      w.sets.forEach((s, k) =>
        nativeJobs.push({sets: [tag ? {...s, ...tag, ...(w.members ? w.members[k] : null)} : s], batchable: true})
      );
    }
    try {
      let codes, aggs, added, outcome;
      if (withBits) {
        const res = await addon.verifyAccumulateBits(this.ctx, nativeJobs, 0);
        codes = res.codes;
        codes.stats = res.stats;
        outcome = res.outcome;
      } else if (pooled) {
        const res = await addon.verifyAccumulate(this.ctx, nativeJobs, 0);
        codes = res.codes;
        codes.stats = res.stats;
        added = res.added;
      } else if (naggs) {
        const res = await addon.verifyAggregate(this.ctx, nativeJobs, 0);
        codes = res.codes;
        codes.stats = res.stats;
        aggs = res.aggs;
      } else {
        codes = await addon.verify(this.ctx, nativeJobs, 0);
      }
      let successCount = 0;
      let errorCount = 0;
      jobs.forEach((job) => {
        const w = job.workReq;
        if (w.perSet) {
          // per set: an error code is false for that set (the interface's per-set retry), never a rejection
          const inPool = w.pool !== undefined;
          if (w.members !== undefined) {
            const results = w.sets.map((_, k) => ({
              valid: codes[job.first + k] === 1,
              outcome: POOL_OUTCOME[outcome[job.firstSet + k]],
            }));
            w.sets.forEach((_, k) => (codes[job.first + k] < 0 ? errorCount++ : successCount++));
            job.resolve({results, signature: null});
            return;
          }
          const results = w.sets.map((_, k) => codes[job.first + k] === 1 && (!inPool || added[job.firstSet + k] === 1));
          w.sets.forEach((_, k) => (codes[job.first + k] < 0 ? errorCount++ : successCount++));
          const ok = job.agg >= 0 && aggs.status[job.agg] === 0;
          job.resolve({results, signature: ok ? aggs.sigs.slice(96 * job.agg, 96 * job.agg + 96) : null});
          return;
        }
        const c = codes[job.first];
        if (c < 0) {
          errorCount += job.workReq.sets.length;
          job.reject(Error(addon.strerror(-c)));
        } else {
          successCount += job.workReq.sets.length;
          job.resolve(c === 1);
        }
      });
      const st = codes.stats || {batchRetries: 0, batchSigsSuccess: 0, deviceMs: 0};
      this.counters.successJobsSignatureSetsCount += successCount;
      this.counters.errorJobsSignatureSetsCount += errorCount;
      this.counters.batchRetries += st.batchRetries;
      if (m) {
        const jobTimeSec = st.deviceMs / 1000;
        m.timePerSigSet.observe(jobTimeSec / Math.max(1, startedSigSets));
        m.jobsWorkerTime.inc({workerId: 0}, jobTimeSec);
        m.successJobsSignatureSetsCount.inc(successCount);
        m.errorJobsSignatureSetsCount.inc(errorCount);
        m.batchRetries.inc(st.batchRetries);
        m.batchSigsSuccess.inc(st.batchSigsSuccess);
      }
    } catch (e) {
      for (const job of jobs) job.reject(e);
    } finally {
      this.inflightSigs -= startedSigSets;
    }
  };

  // ---- SURVEY 8(f) entry points (synchronous; low volume beside verifySignatureSets) ----

  /** Light-client sync-aggregate check, isValidBlsAggregate (light-client/src/validation.ts:152-176):
   * PublicKey.aggregate(publicKeys) (throws on an empty list), then
   * Signature.fromBytes(signature, undefined, true).verify(aggPubkey, message) as one
   * non-batchable aggregate set: an undecodable or non-G2 signature throws with its BLST code,
   * an infinity aggregate verifies false. */
  async isValidBlsAggregate(publicKeys, message, signature) {
    if (publicKeys.length === 0) throw Error("EMPTY_AGGREGATE_ARRAY");
    return this.verifySignatureSets(
      [{type: SignatureSetType.aggregate, pubkeys: publicKeys, signingRoot: message, signature}],
      {batchable: false}
    );
  }

  /** bls.Signature.aggregate(sigs.map((s) => Signature.fromBytes(s, undefined, true))).toBytes()
   * (chain/opPools/attestationPool.ts:184-187): throws Error(BLST code) like the dependency. */
  aggregateSignatures(sigs) {
    return this.aggregateSignaturesMany([sigs])[0];
  }

  /** One aggregate per op-pool entry in a single device call; each element is the compressed
   * aggregate or an Error carrying the BLST code of its first failing signature. */
  aggregateSignaturesMany(aggregates) {
    const {status, sigs} = addon.aggregateSignatures(this.ctx, aggregates);
    return aggregates.map((_, a) => {
      if (status[a] < 0) throw Error(addon.strerror(-status[a]));
      return sigs.slice(96 * a, 96 * a + 96);
    });
  }

  /** Deposit-time key check, PublicKey.fromBytes(pk, affine, true) (processDeposit.ts:64):
   * per key null (valid) or the BLST code name. */
  validatePubkeys(keys48) {
    const flat = new Uint8Array(48 * keys48.length);
    keys48.forEach((k, i) => {
      if (k.length !== 48) throw Error("BLST_BAD_ENCODING");
      flat.set(k, 48 * i);
    });
    const {status} = addon.pubkeysValidate(this.ctx, flat);
    return Array.from(status, (c) => (c === 0 ? null : addon.strerror(-c)));
  }

  /** processDeposit.ts:62-70 signature check over {pubkey, signingRoot, signature} records. */
  verifyDeposits(deposits) {
    const n = deposits.length;
    const keys = new Uint8Array(48 * n);
    const roots = new Uint8Array(32 * n);
    const sigs = new Uint8Array(96 * n);
    deposits.forEach((d, i) => {
      keys.set(d.pubkey, 48 * i);
      roots.set(d.signingRoot, 32 * i);
      sigs.set(d.signature, 96 * i);
    });
    return Array.from(addon.depositsVerify(this.ctx, keys, roots, sigs), (v) => v === 1);
  }
}

// which kind of same-message caller a unit of work is: "poolbits", "pool", "aggregate" or null
function callerKind(w) {
  return w.members !== undefined ? "poolbits" : w.pool !== undefined ? "pool" : w.aggregate ? "aggregate" : null;
}

// BGV_POOL_NOT_ADDED, _ADDED, _KNOWN, _OVERLAP
const POOL_OUTCOME = [null, "added", "known", "overlap"];

// entry or group k of a sigpoolGetBits / sigpoolSum result
function poolRecord(r, k) {
  const nBits = r.nBits[k];
  return {
    status: r.status[k],
    count: r.count[k],
    signature: r.status[k] === 0 ? r.sigs.slice(96 * k, 96 * k + 96) : null,
    nBits,
    bits: r.bits.slice(r.stride * k, r.stride * k + ((nBits + 7) >> 3)),
  };
}

function unwrap(code) {
  if (code < 0) throw Error(addon.strerror(-code));
  return code === 1;
}

module.exports = {BlsGpuVerifier, SignatureSetType, QueueError, chunkifyMaximizeChunkSize, getAggregatedPubkeysCount, toNativeSet, addon};
