"use strict";
// Device-side epoch shuffling through the Node layer (tests/test_node_shuffling.py).
//   node tests/node/shuffling.js cpu   the addon and BlsGpuVerifier export shufflingPut / committeeDropRange
//   node tests/node/shuffling.js       shufflingPut resolves to the reference's 16-element unshuffleList
//                                      vector; a committee set on the shuffled committee verifies,
//                                      one with a flipped bit does not
const assert = require("assert");
const fs = require("fs");
const path = require("path");
const node = path.join(__dirname, "..", "..", "lodestar_amd", "node");
const {BlsGpuVerifier, SignatureSetType, addon} = require(path.join(node, "BlsGpuVerifier.js"));

const KAT = JSON.parse(fs.readFileSync(path.join(__dirname, "..", "golden", "shuffling.json"), "utf8")).unshuffle[1];
const N = 16;
const BITS = Uint8Array.from([0b10110111, 0b01001101]); // positions 0,1,2,4,5,7,8,10,11,14 of 16

function cpuChecks() {
  for (const f of ["shufflingPut", "committeeDropRange"]) {
    assert.strictEqual(typeof addon[f], "function", f);
    assert.strictEqual(typeof BlsGpuVerifier.prototype[f], "function", f);
  }
  assert.strictEqual(KAT.input.length, N);
  return {cpu: "ok"};
}

async function gpuChecks() {
  const sks = new Uint8Array(32 * N);
  for (let i = 0; i < N; i++) sks.fill(i + 1, 32 * i, 32 * (i + 1));
  const pool = new BlsGpuVerifier({maxBufferWaitMs: 20});
  addon.keygen(pool.ctx, sks, 0);
  const report = {};
  const seed = Uint8Array.from(Buffer.from(KAT.seed, "hex"));
  const pending = pool.shufflingPut(200, seed, Uint32Array.from(KAT.input), 1, 1, KAT.rounds);
  assert.ok(pending instanceof Promise);
  const shuffling = await pending;
  assert.ok(shuffling instanceof Uint32Array);
  assert.deepStrictEqual(Array.from(shuffling), KAT.res);
  report.kat = "ok";
  // committee 200 is the whole shuffling; signed by the participants' sum(sk) mod r
  const members = KAT.res.filter((_, k) => (BITS[k >> 3] >> (k & 7)) & 1);
  const R = BigInt("0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001");
  let sum = 0n;
  for (const v of members) sum += BigInt("0x" + Buffer.from(sks.slice(32 * v, 32 * v + 32)).toString("hex"));
  const skAgg = Uint8Array.from(Buffer.from((sum % R).toString(16).padStart(64, "0"), "hex"));
  const signingRoot = new Uint8Array(32).fill(7);
  const set = {
    type: SignatureSetType.committee,
    committee: 200,
    bits: BITS,
    nBits: N,
    signingRoot,
    signature: addon.sign(pool.ctx, skAgg, signingRoot),
  };
  assert.strictEqual(await pool.verifySignatureSets([set]), true);
  report.valid = "ok";
  const flipped = Uint8Array.from(BITS);
  flipped[0] ^= 0b00010000;
  assert.strictEqual(await pool.verifySignatureSets([Object.assign({}, set, {bits: flipped})]), false);
  report.invalid = "ok";
  await assert.rejects(
    pool.shufflingPut(200, seed, Uint32Array.from(KAT.input), 1, 1, KAT.rounds),
    (e) => e.bgvCode === -23 // BGV_E_ARG: the id is live
  );
  assert.strictEqual(pool.committeeDropRange(200, 1), 1);
  assert.strictEqual(pool.committeeDropRange(200, 1), 0);
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
