"use strict";
// Span sets ({type: "committees"}: one bitfield over several stored committees) through the Node
// layer (tests/test_node_multi_committee.py).
//   node tests/node/multi_committee.js cpu   toNativeSet's committees form and the producer of
//                                            signatureSets.js against the expanded-index producer
//   node tests/node/multi_committee.js       a valid and an invalid "committees" set through
//                                            BlsGpuVerifier.verifySignatureSets on the device
const assert = require("assert");
const path = require("path");
const node = path.join(__dirname, "..", "..", "lodestar_amd", "node");
const {BlsGpuVerifier, SignatureSetType, getAggregatedPubkeysCount, addon, toNativeSet} = require(
  path.join(node, "BlsGpuVerifier.js")
);
const ss = require(path.join(node, "signatureSets.js"));

// three committees over validator indices 0..11; the bitfield is laid over 5 + 4 + 3 = 12 bits
const COMMITTEES = {70: [3, 0, 7, 1, 9], 71: [4, 10, 2, 8], 72: [5, 6, 11]};
const IDS = [70, 71, 72];
const NBITS = 12;
const BITS = Uint8Array.from([0b01101111, 0b00001110]); // 0,1,2,3 | 5,6 | 9,10,11 (bit 4, 7, 8 clear)
const ROOT = new Uint8Array(32).fill(0x5a);

function expand(bits) {
  const out = [];
  let off = 0;
  for (const id of IDS) {
    COMMITTEES[id].forEach((v, k) => {
      if ((bits[(off + k) >> 3] >> ((off + k) & 7)) & 1) out.push(v);
    });
    off += COMMITTEES[id].length;
  }
  return out;
}

function cpuChecks() {
  assert.strictEqual(SignatureSetType.committees, "committees");
  const sig = new Uint8Array(96).fill(7);
  const set = ss.getAttestationCommitteesBitsSignatureSet(IDS, {uint8Array: BITS, bitLen: NBITS}, ROOT, sig);
  assert.strictEqual(set.type, "committees");
  assert.deepStrictEqual(set.committees, IDS);
  assert.strictEqual(set.nBits, NBITS);
  assert.deepStrictEqual(Array.from(set.bits), Array.from(BITS));
  assert.strictEqual(set.signingRoot, ROOT);
  // against the expanded-index form: the same participants, counted the same
  const byIdx = {type: SignatureSetType.aggregate, pubkeys: expand(BITS), signingRoot: ROOT, signature: sig};
  assert.deepStrictEqual(byIdx.pubkeys, [3, 0, 7, 1, 4, 10, 5, 6, 11]);
  assert.deepStrictEqual(expand(set.bits), byIdx.pubkeys);
  assert.strictEqual(getAggregatedPubkeysCount([set]), byIdx.pubkeys.length);
  assert.strictEqual(getAggregatedPubkeysCount([set, byIdx]), 2 * byIdx.pubkeys.length);
  // plain bytes instead of a BitArray: the length in bits is 8 per byte
  const plain = ss.getAttestationCommitteesBitsSignatureSet(IDS, BITS, ROOT, sig);
  assert.strictEqual(plain.nBits, 16);
  const nat = toNativeSet(set);
  assert.deepStrictEqual(Object.keys(nat).sort(), ["bits", "committees", "msg", "nBits", "sig"]);
  assert.ok(nat.committees instanceof Uint32Array);
  assert.deepStrictEqual(Array.from(nat.committees), IDS);
  assert.strictEqual(nat.nBits, NBITS);
  return {cpu: "ok"};
}

async function gpuChecks() {
  const N = 12;
  const sks = new Uint8Array(32 * N);
  for (let i = 0; i < N; i++) sks.fill(i + 1, 32 * i, 32 * (i + 1));
  const pool = new BlsGpuVerifier({maxBufferWaitMs: 20});
  addon.keygen(pool.ctx, sks, 0);
  for (const id of IDS) await pool.committeePut(id, COMMITTEES[id]);
  const R = BigInt("0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001");
  let sum = 0n;
  for (const v of expand(BITS)) sum += BigInt("0x" + Buffer.from(sks.slice(32 * v, 32 * v + 32)).toString("hex"));
  const skAgg = Uint8Array.from(Buffer.from((sum % R).toString(16).padStart(64, "0"), "hex"));
  const signature = addon.sign(pool.ctx, skAgg, ROOT);
  const set = ss.getAttestationCommitteesBitsSignatureSet(IDS, {uint8Array: BITS, bitLen: NBITS}, ROOT, signature);
  const report = {};
  assert.strictEqual(await pool.verifySignatureSets([set]), true);
  assert.strictEqual(await pool.verifySignatureSets([set], {batchable: true}), true);
  report.valid = "ok";
  const flipped = Uint8Array.from(BITS);
  flipped[0] ^= 0b00100000; // a member of the second committee dropped
  assert.strictEqual(await pool.verifySignatureSets([Object.assign({}, set, {bits: flipped})]), false);
  assert.strictEqual(await pool.verifySignatureSets([Object.assign({}, set, {bits: flipped})], {batchable: true}), false);
  report.invalid = "ok";
  // beside the index form and a one-committee set in one call
  const byIdx = {type: SignatureSetType.aggregate, pubkeys: expand(BITS), signingRoot: ROOT, signature};
  const one = {type: SignatureSetType.committee, committee: 72, bits: Uint8Array.from([0b111]), nBits: 3, signingRoot: ROOT};
  let s1 = 0n;
  for (const v of COMMITTEES[72]) s1 += BigInt("0x" + Buffer.from(sks.slice(32 * v, 32 * v + 32)).toString("hex"));
  one.signature = addon.sign(pool.ctx, Uint8Array.from(Buffer.from((s1 % R).toString(16).padStart(64, "0"), "hex")), ROOT);
  assert.strictEqual(await pool.verifySignatureSets([byIdx, set, one]), true);
  report.mixed = "ok";
  await assert.rejects(pool.verifySignatureSets([Object.assign({}, set, {bits: new Uint8Array(2)})]), /EMPTY_AGGREGATE/);
  pool.committeeDrop(71);
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
