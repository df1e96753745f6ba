/**
 * Type declarations of @lodestar/blsgpu.  BlsGpuVerifier implements the shape of the beacon
 * node's IBlsVerifier (packages/beacon-node/src/chain/bls/interface.ts:20-46) over the
 * ISignatureSet union (packages/state-transition/src/util/signatureSets.ts:5-22), with one
 * widening: a pubkey may be a validator index into the device cache (or a PublicKey tagged
 * with .index by the pubkey-added hook) as well as a key object or 96-byte record.
 */

/** interface.ts:3-18 */
export interface VerifySignatureOpts {
  batchable?: boolean;
  verifyOnMainThread?: boolean;
}

/** interface.ts:20-46 */
export interface IBlsVerifier {
  verifySignatureSets(sets: ISignatureSet[], opts?: VerifySignatureOpts): Promise<boolean>;
  /** one boolean per set; every set is verified on its own over the shared signing root */
  verifySignatureSetsSameMessage(
    sets: SameMessageSet[],
    message: Uint8Array,
    opts?: Omit<VerifySignatureOpts, "verifyOnMainThread">
  ): Promise<boolean[]>;
  close(): Promise<void>;
  canAcceptWork(): boolean;
}

export declare const SignatureSetType: {
  readonly single: "single";
  readonly aggregate: "aggregate";
  readonly committee: "committee";
  readonly committees: "committees";
};
export type SignatureSetType = typeof SignatureSetType[keyof typeof SignatureSetType];

/** a cached validator index, a PublicKey tagged with its index, or uncompressed key bytes */
export type PubkeyRef = number | {index: number} | {toBytes(compressed?: boolean): Uint8Array} | Uint8Array;

export interface ISingleSignatureSet {
  type: "single";
  pubkey: PubkeyRef;
  signingRoot: Uint8Array; // 32 bytes
  signature: Uint8Array; // 96 bytes compressed G2 (untrusted)
}
export interface IAggregatedSignatureSet {
  type: "aggregate";
  pubkeys: PubkeyRef[];
  signingRoot: Uint8Array;
  signature: Uint8Array;
}
/**
 * Not in the reference: the aggregate as the node holds it before bits.intersectValues -- a
 * committee stored with BlsGpuVerifier.committeePut and the participation bitfield (member k
 * takes part iff (bits[k >> 3] >> (k & 7)) & 1).  bits: ceil(nBits / 8) bytes with nBits beside
 * it, or a BitArray.
 */
export interface ICommitteeSignatureSet {
  type: "committee";
  committee: number;
  bits: Uint8Array | {uint8Array: Uint8Array; bitLen: number};
  nBits?: number;
  signingRoot: Uint8Array;
  signature: Uint8Array;
}
/**
 * One bitfield over several stored committees, concatenated in list order: committee c owns the
 * bits from the sum of the lengths before it on (an attestation since EIP-7549: committee_bits
 * mapped to ids, aggregation_bits).  A repeated id counts its selected members again.
 */
export interface ICommitteesSignatureSet {
  type: "committees";
  committees: number[];
  bits: Uint8Array | {uint8Array: Uint8Array; bitLen: number};
  nBits?: number;
  signingRoot: Uint8Array;
  signature: Uint8Array;
}
export type ISignatureSet =
  | ISingleSignatureSet
  | IAggregatedSignatureSet
  | ICommitteeSignatureSet
  | ICommitteesSignatureSet;

/** one signer of a shared signing root (an unaggregated attestation, a sync committee message) */
export interface SameMessageSet {
  publicKey: PubkeyRef;
  signature: Uint8Array; // 96 bytes compressed G2 (untrusted)
}

/** a pool entry (poolGetBits) or a sum of entries (poolSum) */
export interface PoolRecord {
  /** 0, or a negative library code (not open, nothing added yet) with signature null */
  status: number;
  count: number;
  signature: Uint8Array | null;
  /** positions of the field; the sum of the entries' for poolSum */
  nBits: number;
  /** ceil(nBits / 8) bytes, SSZ bit order */
  bits: Uint8Array;
}

export interface BlsGpuVerifierOpts {
  devices?: number[];
  maxBufferedSigs?: number;
  maxBufferWaitMs?: number;
  /** canAcceptWork() is false while this many sets are queued or in flight (default 262,144) */
  maxInflightSigs?: number;
  blsVerifyAllMultiThread?: boolean;
  /** called once per uploaded run that held undecodable keys (those indices stay unusable) */
  onPubkeyError?: (e: Error, first: number, n: number) => void;
}

export interface BlsGpuVerifierModules {
  metrics?: unknown | null;
}

/** the acceptance rule of balance-weighted sampling: one random byte ("phase0", the default) or 16 bits (EIP-7251) */
export type SamplingRule = "phase0" | "electra";
export declare class QueueError extends Error {
  type: {code: string};
}

export declare class BlsGpuVerifier implements IBlsVerifier {
  constructor(opts?: BlsGpuVerifierOpts, modules?: BlsGpuVerifierModules);
  verifySignatureSets(sets: ISignatureSet[], opts?: VerifySignatureOpts): Promise<boolean>;
  verifySignatureSetsSameMessage(
    sets: SameMessageSet[],
    message: Uint8Array,
    opts?: Omit<VerifySignatureOpts, "verifyOnMainThread">
  ): Promise<boolean[]>;
  /**
   * verifySignatureSetsSameMessage whose device call also returns the compressed sum of the
   * accepted sets' signatures (null when none was accepted): the op pool's Signature.aggregate
   * without a second decoding and subgroup check of each signature.
   */
  verifyAndAggregateSameMessage(
    sets: SameMessageSet[],
    message: Uint8Array,
    opts?: Omit<VerifySignatureOpts, "verifyOnMainThread">
  ): Promise<{results: boolean[]; signature: Uint8Array | null}>;
  /**
   * verifySignatureSetsSameMessage whose device call also adds the accepted sets' signatures to the
   * device-resident pool entry poolId (poolOpen): true iff the set was accepted and added.  The op
   * pool's running aggregate then needs no curve arithmetic on the host
   */
  verifyAndPoolSameMessage(
    sets: SameMessageSet[],
    message: Uint8Array,
    poolId: number,
    opts?: Omit<VerifySignatureOpts, "verifyOnMainThread">
  ): Promise<boolean[]>;
  /**
   * verifyAndPoolSameMessage into an entry that holds participation bits (poolOpen(id, {nBits})):
   * each set names its position (`bit`) or its field (`bits`, ceil(nBits / 8) bytes, SSZ bit
   * order).  `valid` is the verdict; `outcome` is what the entry did with a valid set: "added",
   * "known" (every position already held: InsertOutcome.AlreadyKnown), "overlap" (some held, some
   * new: not aggregated), or null (not valid, or the entry was dropped meanwhile).
   */
  verifyAndPoolBitsSameMessage(
    sets: (SameMessageSet & ({bit: number} | {bits: Uint8Array}))[],
    message: Uint8Array,
    poolId: number,
    opts: Omit<VerifySignatureOpts, "verifyOnMainThread"> & {nBits: number}
  ): Promise<{valid: boolean; outcome: "added" | "known" | "overlap" | null}[]>;
  /**
   * opens the device-resident signature pool entry id (0..16383), empty; with nBits (1..2048) it
   * also holds a participation field of that many positions
   */
  poolOpen(id: number, opts?: {nBits?: number}): void;
  /** poolGet plus the entry's field: nBits is 0 for an entry without bits or not open */
  poolGetBits(ids: Uint32Array | number[]): Promise<PoolRecord[]>;
  /**
   * sums entries on the device without changing them: per group of 1..64 ids the aggregate of every
   * signature held and the entries' fields concatenated in list order
   */
  poolSum(groups: (Uint32Array | number[])[]): Promise<PoolRecord[]>;
  /** drops the live entries of ids first .. first + count - 1; returns how many there were */
  poolDropRange(first: number, count: number): number;
  /**
   * reads entries without changing them: status 0 with the compressed aggregate of the `count`
   * signatures added so far, else a negative library code (not open, nothing added yet) and null
   */
  poolGet(ids: Uint32Array | number[]): Promise<{status: number; count: number; signature: Uint8Array | null}[]>;
  canAcceptWork(): boolean;
  close(): Promise<void>;
  /** state-transition pubkey-added hook: (index, 48-byte pubkey, PublicKey?) */
  pubkeyAddedHook(): (index: number, pubkey: Uint8Array, pk?: object) => void;
  /** uploads the queued keys off the event loop; verifySignatureSets awaits it */
  flushPubkeys(): Promise<void>;
  /** stores a committee (validator indices, their pubkey sum) on the device(s) under id 0..16383 */
  committeePut(id: number, indices: Uint32Array | number[]): Promise<void>;
  /** frees the id at once; queued calls finish on the committee they named */
  committeeDrop(id: number): void;
  /**
   * an epoch's committees in one device call: shuffles activeIndices with seed over `rounds`
   * swap-or-not rounds, stores the slots * committeesPerSlot committees under firstId, firstId + 1, ...
   * and resolves to the shuffling (IEpochShuffling.shuffling)
   */
  shufflingPut(
    firstId: number,
    seed: Uint8Array,
    activeIndices: Uint32Array,
    slots: number,
    committeesPerSlot: number,
    rounds: number
  ): Promise<Uint32Array>;
  /**
   * computeProposers on the device: the proposers of opts.slots slots from startSlot on, -1 where
   * every candidate was rejected; the per-slot seeds are hashed here.  opts.rule "electra" selects
   * EIP-7251's 16-bit draws: effectiveBalanceIncrements is then a Uint16Array or a number array (a
   * Uint8Array is widened) and maxEffectiveBalanceIncrement may reach 65535 (mainnet: 2048)
   */
  computeProposers(
    epochSeed: Uint8Array,
    startSlot: number,
    activeIndices: Uint32Array | number[],
    effectiveBalanceIncrements: Uint8Array | Uint16Array | number[],
    opts: {slots: number; maxEffectiveBalanceIncrement: number; rounds: number; rule?: SamplingRule}
  ): Promise<number[]>;
  /**
   * getNextSyncCommittee on the device: the first opts.size candidates accepted by balance (repeats
   * kept) become committee id; resolves to the list and its 48-byte aggregate pubkey.  opts.rule as
   * for computeProposers
   */
  syncCommitteePut(
    id: number,
    seed: Uint8Array,
    activeIndices: Uint32Array | number[],
    effectiveBalanceIncrements: Uint8Array | Uint16Array | number[],
    opts: {size: number; maxEffectiveBalanceIncrement: number; rounds: number; rule?: SamplingRule}
  ): Promise<{indices: Uint32Array; aggregatePubkey: Uint8Array}>;
  /** drops the live ids of firstId .. firstId + count - 1; returns how many there were */
  committeeDropRange(firstId: number, count: number): number;
  onPubkeyError: ((e: Error, first: number, n: number) => void) | null;
  isValidBlsAggregate(publicKeys: PubkeyRef[], message: Uint8Array, signature: Uint8Array): Promise<boolean>;
  aggregateSignatures(sigs: Uint8Array[]): Uint8Array;
  aggregateSignaturesMany(aggregates: Uint8Array[][]): Uint8Array[];
  validatePubkeys(keys48: Uint8Array[]): (string | null)[];
  verifyDeposits(deposits: {pubkey: Uint8Array; signingRoot: Uint8Array; signature: Uint8Array}[]): boolean[];
}

/** IChainOptions fields added beside blsVerifyAllMainThread / blsVerifyAllMultiThread (options.ts:12-13) */
export interface BlsGpuChainOptions {
  blsGpu?: boolean;
  blsGpuDevices?: number[];
  blsGpuMaxBufferedSigs?: number;
  blsGpuMaxBufferWaitMs?: number;
}
export interface BlsChainOptions extends BlsGpuChainOptions {
  blsVerifyAllMainThread?: boolean;
  blsVerifyAllMultiThread?: boolean;
}

export declare const blsGpuChainOptionDefaults: Readonly<BlsGpuChainOptions>;
export declare const blsGpuCliOptions: Readonly<Record<string, object>>;
export declare function parseBlsGpuArgs(args: Record<string, unknown>): BlsGpuChainOptions;

export interface BlsVerifierImpls {
  BlsSingleThreadVerifier?: new (modules: {metrics?: unknown | null}) => IBlsVerifier;
  BlsMultiThreadWorkerPool?: new (opts: BlsChainOptions, modules: {metrics?: unknown; logger?: unknown}) => IBlsVerifier;
  setPubkeyAddedHook?: (hook: (index: number, pubkey: Uint8Array, pk?: object) => void) => void;
}

/** chain.ts:189-192 with the GPU branch */
export declare function createBlsVerifier(
  opts: BlsChainOptions,
  modules: {metrics?: unknown | null; logger?: unknown},
  impls?: BlsVerifierImpls
): IBlsVerifier;
export declare function createBlsGpuVerifier(
  opts: BlsChainOptions,
  modules?: {metrics?: unknown | null},
  setPubkeyAddedHook?: BlsVerifierImpls["setPubkeyAddedHook"]
): BlsGpuVerifier;

export declare function chunkifyMaximizeChunkSize<T>(arr: T[], minPerChunk: number): T[][];
