"use strict";
// Device-side balance-weighted sampling under Electra's rule through the Node layer
// (tests/test_node_sampling_electra.py).
//   node tests/node/sampling_electra.js cpu   the addon exports proposersElectra / syncCommitteePutElectra
//   node tests/node/sampling_electra.js       computeProposers(..., {rule: "electra"}) on (`min`, 257)
//                                             equals a restatement of the spec's compute_proposer_index
//                                             (EIP-7251) written here with crypto; a Uint8Array table
//                                             gives what its widened Uint16Array gives; syncCommitteePut,
//                                             then a valid and an invalid {type: "committee"} set
const assert = require("assert");
const crypto = require("crypto");
const path = require("path");
const node = path.join(__dirname, "..", "..", "lodestar_amd", "node");
const {BlsGpuVerifier, SignatureSetType, addon} = require(path.join(node, "BlsGpuVerifier.js"));

const ROUNDS = 90;
const MAX_INCR = 2048;
const MAX_RANDOM_VALUE = 65535;
const SEED = crypto.createHash("sha256").update("lodestar-amd gpu sampling").digest();
const sha256 = (...parts) => crypto.createHash("sha256").update(Buffer.concat(parts)).digest();
const le = (v, n) => {
  const b = Buffer.alloc(8);
  b.writeBigUInt64LE(BigInt(v), 0);
  return b.subarray(0, n);
};

function cpuChecks() {
  for (const f of ["proposersElectra", "syncCommitteePutElectra"]) assert.strictEqual(typeof addon[f], "function", f);
  return {cpu: "ok"};
}

// the spec's compute_shuffled_index and compute_proposer_index as of Electra, restated
function computeShuffledIndex(index, n, seed) {
  for (let r = 0; r < ROUNDS; r++) {
    const rb = Buffer.from([r]);
    const pivot = Number(sha256(seed, rb).readBigUInt64LE(0) % BigInt(n));
    const flip = (pivot + n - index) % n;
    const position = Math.max(index, flip);
    const source = sha256(seed, rb, le(Math.floor(position / 256), 4));
    const bit = (source[Math.floor((position % 256) / 8)] >> position % 8) & 1;
    index = bit ? flip : index;
  }
  return index;
}
function computeProposerIndex(eff, indices, seed, maxIncr) {
  let i = 0;
  for (;;) {
    const candidate = indices[computeShuffledIndex(i % indices.length, indices.length, seed)];
    const randomValue = sha256(seed, le(Math.floor(i / 16), 8)).readUInt16LE((i % 16) * 2);
    if (eff[candidate] * MAX_RANDOM_VALUE >= maxIncr * randomValue) return candidate;
    i += 1;
    if (i === indices.length) return -1; // bounded at the list's end, as the byte rule's loop is
  }
}

async function gpuChecks() {
  const N = 64;
  const sks = new Uint8Array(32 * N);
  for (let i = 0; i < N; i++) sks.fill(i + 1, 32 * i, 32 * (i + 1));
  const pool = new BlsGpuVerifier({maxBufferWaitMs: 20});
  addon.keygen(pool.ctx, sks, 0);
  const report = {};

  // proposers: the `min` table (32 of 2048 everywhere) over 257 gapped indices, 32 slots from slot 0
  const active = Array.from({length: 257}, (_, i) => i + Math.floor(i / 6));
  const min = new Uint16Array(active[256] + 1).fill(32);
  const opts = {slots: 32, maxEffectiveBalanceIncrement: MAX_INCR, rounds: ROUNDS, rule: "electra"};
  const pending = pool.computeProposers(SEED, 0, active, min, opts);
  assert.ok(pending instanceof Promise);
  const got = await pending;
  const want = [];
  for (let slot = 0; slot < 32; slot++)
    want.push(computeProposerIndex(min, active, sha256(SEED, le(slot, 8)), MAX_INCR));
  assert.deepStrictEqual(got, want);
  assert.ok(want.includes(-1) && want.some((v) => v >= 0));
  report.proposers = "ok";

  // a Uint8Array under "electra" is widened, not reinterpreted: 1 + v % 4 of 32 as bytes, as
  // 16-bit values and as numbers give one result, which is not the byte rule's
  const small = Uint8Array.from({length: active[256] + 1}, (_, v) => 1 + (v % 4));
  const sopt = Object.assign({}, opts, {maxEffectiveBalanceIncrement: 32});
  const fromBytes = await pool.computeProposers(SEED, 0, active, small, sopt);
  assert.deepStrictEqual(fromBytes, await pool.computeProposers(SEED, 0, active, Uint16Array.from(small), sopt));
  assert.deepStrictEqual(fromBytes, await pool.computeProposers(SEED, 0, active, Array.from(small), sopt));
  const wantSmall = [];
  for (let slot = 0; slot < 32; slot++)
    wantSmall.push(computeProposerIndex(small, active, sha256(SEED, le(slot, 8)), 32));
  assert.deepStrictEqual(fromBytes, wantSmall);
  const byteRule = await pool.computeProposers(SEED, 0, active, small, Object.assign({}, sopt, {rule: "phase0"}));
  assert.notDeepStrictEqual(fromBytes, byteRule);
  await assert.rejects(pool.computeProposers(SEED, 0, active, [65536], sopt), RangeError);
  const unknown = Object.assign({}, sopt, {rule: "deneb"});
  await assert.rejects(pool.computeProposers(SEED, 0, active, small, unknown), TypeError);
  report.widened = "ok";

  // a sync committee of 16 over the 64 cached keys; every member signs
  const act = Uint32Array.from({length: N}, (_, i) => i);
  const mixed = Uint16Array.from({length: N}, (_, v) => (v % 3 ? 2048 : 32 + 300 * (v % 7)));
  const copts = {size: 16, maxEffectiveBalanceIncrement: MAX_INCR, rounds: ROUNDS, rule: "electra"};
  const res = await pool.syncCommitteePut(310, SEED, act, mixed, copts);
  assert.ok(res.indices instanceof Uint32Array && res.indices.length === 16);
  assert.ok(res.aggregatePubkey instanceof Uint8Array && res.aggregatePubkey.length === 48);
  // the spec's get_next_sync_committee_indices, restated
  const wantIdx = [];
  for (let i = 0; wantIdx.length < 16; i++) {
    const candidate = act[computeShuffledIndex(i % N, N, SEED)];
    const randomValue = sha256(SEED, le(Math.floor(i / 16), 8)).readUInt16LE((i % 16) * 2);
    if (mixed[candidate] * MAX_RANDOM_VALUE >= MAX_INCR * randomValue) wantIdx.push(candidate);
  }
  assert.deepStrictEqual(Array.from(res.indices), wantIdx);
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
    committee: 310,
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
    pool.syncCommitteePut(310, SEED, act, mixed, copts),
    (e) => e.bgvCode === -23 // BGV_E_ARG: the id is live
  );
  pool.committeeDrop(310);
  // the addon takes a Uint16Array only
  assert.throws(() => addon.proposersElectra(pool.ctx, new Uint8Array(32), act, new Uint8Array(N), MAX_INCR, ROUNDS));
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
