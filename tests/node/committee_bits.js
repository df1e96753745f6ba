"use strict";
// Committee-bitfield sets through the Node layer (tests/test_node_committee_bits.py).
//   node tests/node/committee_bits.js cpu   the addon's exports, toNativeSet's committee form and
//                                           the bits producers of signatureSets.js (no device)
//   node tests/node/committee_bits.js       one valid and one invalid committee set through
//                                           BlsGpuVerifier.verifySignatureSets on the device
const assert = require("assert");
const path = require("path");
const node = path.join(__dirname, "..", "..", "lodestar_amd", "node");
const {BlsGpuVerifier, SignatureSetType, getAggregatedPubkeysCount, addon, toNativeSet} = require(
  path.join(node, "BlsGpuVerifier.js")
);
const ss = require(path.join(node, "signatureSets.js"));

const N = 11; // committee members = validator indices 0..N-1 in another order
const MEMBERS = [3, 0, 7, 1, 9, 4, 10, 2, 8, 5, 6];
const BITS = Uint8Array.from([0b11011011, 0b00000101]); // positions 0,1,3,4,6,7,8,10 of 11

function makeState() {
  const forks = [
    {name: "phase0", epoch: 0, version: Uint8Array.from([0, 0, 0, 0])},
    {name: "altair", epoch: 1, version: Uint8Array.from([1, 0, 0, 0])},
  ];
  const config = ss.createForkConfig(forks, new Uint8Array(32).fill(0x42));
  return {
    slot: 70,
    config,
    epochCtx: {
      getBeaconCommittee: () => MEMBERS,
      currentSyncCommitteeIndexed: {validatorIndices: MEMBERS},
    },
  };
}

function makeAttestation() {
  return {
    aggregationBits: {uint8Array: BITS, bitLen: N},
    data: {
      slot: 69,
      index: 0,
      beaconBlockRoot: new Uint8Array(32).fill(1),
      source: {epoch: 1, root: new Uint8Array(32).fill(2)},
      target: {epoch: 2, root: new Uint8Array(32).fill(3)},
    },
    signature: new Uint8Array(96),
  };
}

function makeBlock(bits) {
  return {
    slot: 70,
    parentRoot: new Uint8Array(32).fill(9),
    body: {syncAggregate: {syncCommitteeBits: {uint8Array: bits, bitLen: N}, syncCommitteeSignature: new Uint8Array(96).fill(5)}},
  };
}

function expand(bits) {
  return MEMBERS.filter((_, k) => (bits[k >> 3] >> (k & 7)) & 1);
}

function cpuChecks() {
  for (const f of ["committeePut", "committeeDrop", "aggregateCommitteeBits"]) assert.strictEqual(typeof addon[f], "function", f);
  assert.strictEqual(SignatureSetType.committee, "committee");
  const state = makeState();
  const att = makeAttestation();
  // the bits producer: the index producer's signing root, the bitfield instead of the indices
  const byIdx = ss.getAttestationWithIndicesSignatureSet(state, att, expand(BITS));
  const byBits = ss.getAttestationBitsSignatureSet(state, att, 77);
  assert.strictEqual(byBits.type, "committee");
  assert.strictEqual(byBits.committee, 77);
  assert.strictEqual(byBits.nBits, N);
  assert.deepStrictEqual(Array.from(byBits.bits), Array.from(BITS));
  assert.deepStrictEqual(Array.from(byBits.signingRoot), Array.from(byIdx.signingRoot));
  assert.deepStrictEqual(expand(byBits.bits), byIdx.pubkeys);
  assert.strictEqual(getAggregatedPubkeysCount([byBits, byIdx]), 8 + 8);
  const nat = toNativeSet(byBits);
  assert.deepStrictEqual(Object.keys(nat).sort(), ["bits", "committee", "msg", "nBits", "sig"]);
  assert.strictEqual(nat.committee, 77);
  assert.strictEqual(nat.nBits, N);
  // the existing producers keep their output
  assert.strictEqual(byIdx.type, "aggregate");
  assert.deepStrictEqual(Object.keys(toNativeSet(byIdx)).sort(), ["msg", "pkIndices", "sig"]);
  // sync aggregate: same root as the index form, null for an empty infinity aggregate
  const block = makeBlock(BITS);
  const syncIdx = ss.getSyncCommitteeSignatureSet(state, block);
  const syncBits = ss.getSyncCommitteeBitsSignatureSet(state, block, 78);
  assert.deepStrictEqual(Array.from(syncBits.signingRoot), Array.from(syncIdx.signingRoot));
  assert.deepStrictEqual(expand(syncBits.bits), syncIdx.pubkeys);
  assert.strictEqual(syncBits.committee, 78);
  const empty = makeBlock(new Uint8Array(2));
  assert.throws(() => ss.getSyncCommitteeBitsSignatureSet(state, empty, 78), /not infinity/);
  empty.body.syncAggregate.syncCommitteeSignature = ss.G2_POINT_AT_INFINITY;
  assert.strictEqual(ss.getSyncCommitteeBitsSignatureSet(state, empty, 78), null);
  return {cpu: "ok"};
}

async function gpuChecks() {
  const sks = new Uint8Array(32 * N);
  for (let i = 0; i < N; i++) sks.fill(i + 1, 32 * i, 32 * (i + 1));
  const pool = new BlsGpuVerifier({maxBufferWaitMs: 20});
  addon.keygen(pool.ctx, sks, 0);
  await pool.committeePut(77, MEMBERS);
  const state = makeState();
  const att = makeAttestation();
  const set = ss.getAttestationBitsSignatureSet(state, att, 77);
  // signed by the participants: the signature of sum(sk) mod r over the set's signing root
  const R = BigInt("0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001");
  let sum = 0n;
  for (const v of expand(BITS)) sum += BigInt("0x" + Buffer.from(sks.slice(32 * v, 32 * v + 32)).toString("hex"));
  const skAgg = Uint8Array.from(Buffer.from((sum % R).toString(16).padStart(64, "0"), "hex"));
  set.signature = addon.sign(pool.ctx, skAgg, set.signingRoot);
  const report = {};
  assert.strictEqual(await pool.verifySignatureSets([set]), true);
  assert.strictEqual(await pool.verifySignatureSets([set], {batchable: true}), true);
  report.valid = "ok";
  // one participant's bit flipped: false, not an error
  const flipped = Uint8Array.from(BITS);
  flipped[0] ^= 0b00001000;
  assert.strictEqual(await pool.verifySignatureSets([Object.assign({}, set, {bits: flipped})]), false);
  assert.strictEqual(await pool.verifySignatureSets([Object.assign({}, set, {bits: flipped})], {batchable: true}), false);
  report.invalid = "ok";
  // the same participants as an index list decide the same
  const byIdx = ss.getAttestationWithIndicesSignatureSet(state, att, expand(BITS));
  byIdx.signature = set.signature;
  assert.strictEqual(await pool.verifySignatureSets([byIdx, set]), true);
  // parity hook against the index form's aggregate
  assert.deepStrictEqual(
    Array.from(addon.aggregateCommitteeBits(pool.ctx, 77, BITS, N)),
    Array.from(addon.aggregatePubkeys(pool.ctx, Uint32Array.from(expand(BITS))))
  );
  report.parity = "ok";
  await assert.rejects(pool.verifySignatureSets([Object.assign({}, set, {bits: new Uint8Array(2)})]), /EMPTY_AGGREGATE/);
  pool.committeeDrop(77);
  await assert.rejects(pool.verifySignatureSets([set]), /BGV_E_BAD_INDEX/);
  report.dropped = "ok";
  await pool.close();
  return report;
}

(async () => {
  const out = process.argv[2] === "cpu" ? cpuChecks() : await gpuChecks();
  console.log(JSON.stringify(out));
})().catch((e) => {
  console.error(e && e.stack ? e.stack : e);
  process.exit(1);
});
