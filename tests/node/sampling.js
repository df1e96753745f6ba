"use strict";
// Device-side balance-weighted sampling through the Node layer (tests/test_node_sampling.py).
//   node tests/node/sampling.js cpu   the addon and BlsGpuVerifier export the new entry points
//   node tests/node/sampling.js       computeProposers on (`low`, 257) equals a restatement of
//                                     computeProposers / computeProposerIndex written here with
//                                     crypto; syncCommitteePut, then a valid and an invalid
//                                     {type: "committee"} set through verifySignatureSets
const assert = require("assert");
const crypto = require("crypto");
const path = require("path");
const node = path.join(__dirname, "..", "..", "lodestar_amd", "node");
const {BlsGpuVerifier, SignatureSetType, addon} = require(path.join(node, "BlsGpuVerifier.js"));

const ROUNDS = 90;
const MAX_INCR = 32;
const SEED = crypto.createHash("sha256").update("lodestar-amd gpu sampling").digest();
const sha256 = (...parts) => crypto.createHash("sha256").update(Buffer.concat(parts)).digest();
const le = (v, n) => {
  const b = Buffer.alloc(n);
  b.writeBigUInt64LE(BigInt(v), 0);
  return b.subarray(0, n);
};

function cpuChecks() {
  for (const f of ["proposers", "syncCommitteePut"]) assert.strictEqual(typeof addon[f], "function", f);
  for (const f of ["computeProposers", "syncCommitteePut"])
    assert.strictEqual(typeof BlsGpuVerifier.prototype[f], "function", f);
  return {cpu: "ok"};
}

// the spec's compute_shuffled_index and util/seed.ts's computeProposerIndex, restated
function computeShuffledIndex(index, n, seed) {
  for (let r = 0; r < ROUNDS; r++) {
    const rb = Buffer.from([r]);
    const pivot = Number(sha256(seed, rb).readBigUInt64LE(0) % BigInt(n));
    const flip = (pivot + n - index) % n;
    const position = Math.max(index, flip);
    const source = sha256(seed, rb, le(Math.floor(position / 256), 8).subarray(0, 4));
    const bit = (source[Math.floor((position % 256) / 8)] >> position % 8) & 1;
    index = bit ? flip : index;
  }
  return index;
}
function computeProposerIndex(eff, indices, seed) {
  let i = 0;
  for (;;) {
    const candidate = indices[computeShuffledIndex(i % indices.length, indices.length, seed)];
    const randByte = sha256(seed, le(Math.floor(i / 32), 8))[i % 32];
    if (eff[candidate] * 255 >= MAX_INCR * randByte) return candidate;
    i += 1;
    if (i === indices.length) return -1;
  }
}

async function gpuChecks() {
  const N = 64;
  const sks = new Uint8Array(32 * N);
  for (let i = 0; i < N; i++) sks.fill(i + 1, 32 * i, 32 * (i + 1));
  const pool = new BlsGpuVerifier({maxBufferWaitMs: 20});
  addon.keygen(pool.ctx, sks, 0);
  const report = {};

  // proposers: the `low` table over 257 gapped indices, 32 slots from slot 0
  const active = Array.from({length: 257}, (_, i) => i + Math.floor(i / 6));
  const low = Uint8Array.from({length: active[256] + 1}, (_, v) => 1 + (v % 4));
  const opts = {slots: 32, maxEffectiveBalanceIncrement: MAX_INCR, rounds: ROUNDS};
  const pending = pool.computeProposers(SEED, 0, active, low, opts);
  assert.ok(pending instanceof Promise);
  const got = await pending;
  const want = [];
  for (let slot = 0; slot < 32; slot++) want.push(computeProposerIndex(low, active, sha256(SEED, le(slot, 8))));
  assert.deepStrictEqual(got, want);
  report.proposers = "ok";
  // two indices with low balances: most slots have no proposer (-1)
  const two = await pool.computeProposers(SEED, 0, [0, 1], low, opts);
  const wantTwo = [];
  for (let slot = 0; slot < 32; slot++) wantTwo.push(computeProposerIndex(low, [0, 1], sha256(SEED, le(slot, 8))));
  assert.deepStrictEqual(two, wantTwo);
  assert.ok(two.includes(-1));
  report.none = "ok";

  // a sync committee of 16 over the 64 cached keys; every member signs
  const act = Uint32Array.from({length: N}, (_, i) => i);
  const mixed = Uint8Array.from({length: N}, (_, v) => (v % 3 ? 32 : 1 + (v % 7)));
  const sopts = {size: 16, maxEffectiveBalanceIncrement: MAX_INCR, rounds: ROUNDS};
  const res = await pool.syncCommitteePut(300, SEED, act, mixed, sopts);
  assert.ok(res.indices instanceof Uint32Array && res.indices.length === 16);
  assert.ok(res.aggregatePubkey instanceof Uint8Array && res.aggregatePubkey.length === 48);
  assert.ok(res.aggregatePubkey[0] & 0x80);
  const R = BigInt("0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001");
  let sum = 0n;
  for (const v of res.indices) sum += BigInt("0x" + Buffer.from(sks.slice(32 * v, 32 * v + 32)).toString("hex"));
  const skAgg = Uint8Array.from(Buffer.from((sum % R).toString(16).padStart(64, "0"), "hex"));
  // the aggregate is the public key of the summed secret keys
  assert.deepStrictEqual(Buffer.from(res.aggregatePubkey), Buffer.from(addon.keygen(pool.ctx, skAgg, -1)));
  report.aggregate = "ok";
  const signingRoot = new Uint8Array(32).fill(9);
  const set = {
    type: SignatureSetType.committee,
    committee: 300,
    bits: Uint8Array.from([0xff, 0xff]),
    nBits: 16,
    signingRoot,
    signature: addon.sign(pool.ctx, skAgg, signingRoot),
  };
  assert.strictEqual(await pool.verifySignatureSets([set]), true);
  report.valid = "ok";
  assert.strictEqual(
    await pool.verifySignatureSets([Object.assign({}, set, {bits: Uint8Array.from([0xff, 0xfe])})]),
    false
  );
  report.invalid = "ok";
  await assert.rejects(
    pool.syncCommitteePut(300, SEED, act, mixed, sopts),
    (e) => e.bgvCode === -23 // BGV_E_ARG: the id is live
  );
  pool.committeeDrop(300);
  report.rejects = "ok";
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
