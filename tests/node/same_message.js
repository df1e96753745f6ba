"use strict";
// verifySignatureSetsSameMessage / verifyAndAggregateSameMessage / canAcceptWork of BlsGpuVerifier
// (tests/test_node_same_message.py).
//   node tests/node/same_message.js cpu   against a mock addon (no GPU): which addon entry a run
//                                         takes, how callers' sets travel and how the results
//                                         come back to each caller; canAcceptWork at its bound
//   node tests/node/same_message.js       on the device: five signers of one root, one wrong
const assert = require("assert");
const path = require("path");
const node = path.join(__dirname, "..", "..", "lodestar_amd", "node");
const addonPath = path.join(node, "blsgpu.node");

// ---- CPU: a mock addon that accepts a set iff its signature's first byte is 1 (2: an error code)
const calls = [];
const codeOf = (job) => {
  if (job.sets.some((s) => s.sig[0] === 2)) return -8;
  return job.sets.every((s) => s.sig[0] === 1) ? 1 : 0;
};
let hold = false; // device calls wait in `waiting` while set
const waiting = [];
const gate = () => new Promise((r) => (hold ? waiting.push(r) : setTimeout(r, 2)));
const mock = {
  init: () => ({}),
  close: () => {},
  strerror: (c) => "code " + c,
  verify: async (ctx, jobs) => {
    calls.push({entry: "verify", jobs});
    await gate();
    return Int32Array.from(jobs.map(codeOf));
  },
  verifyAggregate: async (ctx, jobs) => {
    calls.push({entry: "verifyAggregate", jobs});
    await gate();
    const codes = Int32Array.from(jobs.map(codeOf));
    let naggs = 0;
    for (const j of jobs) for (const s of j.sets) if (s.agg !== undefined) naggs = Math.max(naggs, s.agg + 1);
    const status = new Int32Array(naggs).fill(-20);
    const count = new Uint32Array(naggs);
    const sigs = new Uint8Array(96 * naggs);
    // the "sum": byte 1 of every accepted signature added up, the aggregate's id in byte 0
    jobs.forEach((j, i) => {
      for (const s of j.sets) {
        if (s.agg === undefined || codes[i] !== 1) continue;
        status[s.agg] = 0;
        count[s.agg]++;
        sigs[96 * s.agg] = s.agg;
        sigs[96 * s.agg + 1] += s.sig[1];
      }
    });
    return {codes, stats: {batchRetries: 0, batchSigsSuccess: 0, deviceMs: 0}, aggs: {status, count, sigs}};
  },
};

const ROOT = new Uint8Array(32).fill(0x5a);
const sig = (first, second) => {
  const b = new Uint8Array(96);
  b[0] = first;
  b[1] = second;
  return b;
};

async function cpuChecks() {
  require.cache[addonPath] = {id: addonPath, filename: addonPath, loaded: true, exports: mock};
  const {BlsGpuVerifier} = require(path.join(node, "BlsGpuVerifier.js"));
  const v = new BlsGpuVerifier({maxBufferWaitMs: 5, maxBufferedSigs: 1000});
  const single = (s) => ({type: "single", pubkey: 7, signingRoot: ROOT, signature: s});

  // two aggregating callers and a plain one in the same run: one device call, per-caller results
  const a = v.verifyAndAggregateSameMessage(
    [{publicKey: 0, signature: sig(1, 10)}, {publicKey: 1, signature: sig(0, 20)}, {publicKey: 2, signature: sig(1, 30)}],
    ROOT, {batchable: true});
  const plain = v.verifySignatureSets([single(sig(1, 0)), single(sig(1, 0))], {batchable: true});
  const b = v.verifyAndAggregateSameMessage(
    [{publicKey: 3, signature: sig(2, 1)}, {publicKey: 4, signature: sig(1, 2)}], ROOT, {batchable: true});
  const bare = v.verifySignatureSetsSameMessage(
    [{publicKey: 5, signature: sig(1, 0)}, {publicKey: 6, signature: sig(0, 0)}], ROOT);
  const none = v.verifyAndAggregateSameMessage([{publicKey: 8, signature: sig(0, 9)}], ROOT);
  const [ra, rp, rb, rbare, rnone] = await Promise.all([a, plain, b, bare, none]);
  assert.strictEqual(calls.length, 1);
  assert.strictEqual(calls[0].entry, "verifyAggregate");
  // every same-message set is its own batchable one-set job; the plain caller's job is untouched
  assert.deepStrictEqual(calls[0].jobs.map((j) => [j.sets.length, j.batchable]),
    [[1, true], [1, true], [1, true], [2, true], [1, true], [1, true], [1, true], [1, true], [1, true]]);
  assert.deepStrictEqual(calls[0].jobs.map((j) => j.sets[0].agg), [0, 0, 0, undefined, 1, 1, undefined, undefined, 2]);
  assert.ok(calls[0].jobs.every((j) => j.sets.every((s) => s.msg === ROOT)));
  assert.deepStrictEqual(Array.from(calls[0].jobs[0].sets[0].pkIndices), [0]);
  assert.deepStrictEqual(ra.results, [true, false, true]);
  assert.deepStrictEqual([ra.signature[0], ra.signature[1], ra.signature.length], [0, 40, 96]);
  assert.strictEqual(rp, true);
  assert.deepStrictEqual(rb.results, [false, true]); // an error code is false for its set, not a rejection
  assert.deepStrictEqual([rb.signature[0], rb.signature[1]], [1, 2]);
  assert.deepStrictEqual(rbare, [true, false]);
  assert.deepStrictEqual(rnone, {results: [false], signature: null});
  assert.deepStrictEqual(await v.verifyAndAggregateSameMessage([], ROOT), {results: [], signature: null});

  // a run with no tagged set still calls addon.verify
  calls.length = 0;
  const r2 = await Promise.all([
    v.verifySignatureSets([single(sig(1, 0))], {batchable: true}),
    v.verifySignatureSetsSameMessage([{publicKey: 1, signature: sig(1, 0)}, {publicKey: 2, signature: sig(2, 0)}], ROOT),
    v.verifySignatureSets([single(sig(0, 0))]),
  ]);
  assert.ok(calls.length >= 1 && calls.every((c) => c.entry === "verify"), JSON.stringify(calls.map((c) => c.entry)));
  assert.ok(calls.every((c) => c.jobs.every((j) => j.sets.every((s) => s.agg === undefined))));
  assert.deepStrictEqual(r2, [true, [true, false], false]);
  await v.close();

  // canAcceptWork flips at the bound, counts queued and in-flight sets, and recovers
  const w = new BlsGpuVerifier({maxInflightSigs: 4, maxBufferWaitMs: 1});
  assert.strictEqual(new BlsGpuVerifier({ctx: {}}).maxInflightSigs, 262144);
  assert.strictEqual(w.canAcceptWork(), true);
  hold = true;
  const p1 = w.verifySignatureSetsSameMessage(
    [1, 2, 3].map((k) => ({publicKey: k, signature: sig(1, 0)})), ROOT);
  assert.strictEqual(w.inflightSigs, 3);
  assert.strictEqual(w.canAcceptWork(), true); // 3 < 4
  const p2 = w.verifySignatureSets([single(sig(1, 0))]);
  await new Promise((r) => setTimeout(r, 20)); // both are in device calls now (or queued behind one)
  assert.strictEqual(w.inflightSigs, 4);
  assert.strictEqual(w.canAcceptWork(), false); // 4 >= 4
  hold = false;
  for (const go of waiting.splice(0)) go();
  assert.deepStrictEqual(await p1, [true, true, true]);
  assert.strictEqual(await p2, true);
  assert.strictEqual(w.canAcceptWork(), true);
  // queued work rejected by close() is given back
  const p3 = w.verifySignatureSets([single(sig(1, 0))], {batchable: true});
  assert.strictEqual(w.inflightSigs, 1);
  await w.close();
  await assert.rejects(p3, /QUEUE_ABORTED/);
  assert.strictEqual(w.inflightSigs, 0);
  assert.strictEqual(w.canAcceptWork(), false); // closed
  return {cpu: "ok"};
}

// ---- GPU
async function gpuChecks() {
  const {BlsGpuVerifier, addon} = require(path.join(node, "BlsGpuVerifier.js"));
  const N = 5;
  const sks = new Uint8Array(32 * N);
  for (let i = 0; i < N; i++) sks.fill(i + 1, 32 * i, 32 * (i + 1));
  const pool = new BlsGpuVerifier({maxBufferWaitMs: 20});
  addon.keygen(pool.ctx, sks, 0);
  const msgs = new Uint8Array(32 * N);
  for (let i = 0; i < N; i++) msgs.set(ROOT, 32 * i);
  const all = addon.sign(pool.ctx, sks, msgs);
  const sigs = [];
  for (let i = 0; i < N; i++) sigs.push(all.slice(96 * i, 96 * i + 96));
  // set 2 carries signer 3's signature
  const sets = [0, 1, 2, 3, 4].map((k) => ({publicKey: k, signature: k === 2 ? sigs[3] : sigs[k]}));
  const report = {};
  assert.deepStrictEqual(await pool.verifySignatureSetsSameMessage(sets, ROOT), [true, true, false, true, true]);
  report.results = "ok";
  const want = pool.aggregateSignatures([sigs[0], sigs[1], sigs[3], sigs[4]]);
  const [agg, other] = await Promise.all([
    pool.verifyAndAggregateSameMessage(sets, ROOT),
    pool.verifyAndAggregateSameMessage([{publicKey: 1, signature: sigs[1]}], ROOT),
  ]);
  assert.deepStrictEqual(agg.results, [true, true, false, true, true]);
  assert.deepStrictEqual(Buffer.from(agg.signature), Buffer.from(want));
  assert.deepStrictEqual(other.results, [true]);
  assert.deepStrictEqual(Buffer.from(other.signature), Buffer.from(sigs[1]));
  report.aggregate = "ok";
  // an undecodable signature is false for its set and absent from the sum; none accepted: null
  const bad = await pool.verifyAndAggregateSameMessage(
    [{publicKey: 0, signature: sigs[0]}, {publicKey: 1, signature: sigs[1].slice(0, 95)}], ROOT);
  assert.deepStrictEqual(bad.results, [true, false]);
  assert.deepStrictEqual(Buffer.from(bad.signature), Buffer.from(sigs[0]));
  const none = await pool.verifyAndAggregateSameMessage([{publicKey: 0, signature: sigs[1]}], ROOT);
  assert.deepStrictEqual(none, {results: [false], signature: null});
  report.errors = "ok";
  assert.strictEqual(pool.canAcceptWork(), true);
  await pool.close();
  await assert.rejects(pool.verifySignatureSetsSameMessage(sets, ROOT), /QUEUE_ABORTED/);
  report.closed = "ok";
  return report;
}

(async () => {
  const out = process.argv[2] === "cpu" ? await cpuChecks() : await gpuChecks();
  console.log(JSON.stringify(out));
})().catch((e) => {
  console.error(e && e.stack ? e.stack : e);
  process.exit(1);
});
