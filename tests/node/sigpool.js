"use strict";
// poolOpen / poolDropRange / poolGet / verifyAndPoolSameMessage of BlsGpuVerifier
// (tests/test_node_sigpool.py).
//   node tests/node/sigpool.js cpu   against a mock addon (no GPU): a buffered run holds one kind
//                                    of caller, how a pool caller's sets travel and how `added`
//                                    comes back to it
//   node tests/node/sigpool.js       on the device: two calls into one entry with a wrong signer and
//                                    an undecodable signature in the second, poolGet against
//                                    aggregateSignatures of the accepted sets; a pool caller and an
//                                    aggregating caller issued together
const assert = require("assert");
const path = require("path");
const node = path.join(__dirname, "..", "..", "lodestar_amd", "node");
const addonPath = path.join(node, "blsgpu.node");

// ---- CPU: a mock addon that accepts a set iff its signature's first byte is 1 (2: an error code);
// a pool entry whose id is odd "no longer decodes": nothing of it is added
const calls = [];
const codeOf = (job) => {
  if (job.sets.some((s) => s.sig[0] === 2)) return -8;
  return job.sets.every((s) => s.sig[0] === 1) ? 1 : 0;
};
const stats = {batchRetries: 0, batchSigsSuccess: 0, deviceMs: 0};
const tick = () => new Promise((r) => setTimeout(r, 2));
const mock = {
  init: () => ({}),
  close: () => {},
  strerror: (c) => "code " + c,
  verify: async (ctx, jobs) => {
    calls.push({entry: "verify", jobs});
    await tick();
    return Int32Array.from(jobs.map(codeOf));
  },
  verifyAggregate: async (ctx, jobs) => {
    calls.push({entry: "verifyAggregate", jobs});
    await tick();
    const codes = Int32Array.from(jobs.map(codeOf));
    let naggs = 0;
    for (const j of jobs) for (const s of j.sets) if (s.agg !== undefined) naggs = Math.max(naggs, s.agg + 1);
    const status = new Int32Array(naggs).fill(-20);
    const sigs = new Uint8Array(96 * naggs);
    jobs.forEach((j, i) => {
      for (const s of j.sets) {
        if (s.agg === undefined || codes[i] !== 1) continue;
        status[s.agg] = 0;
        sigs[96 * s.agg + 1] += s.sig[1];
      }
    });
    return {codes, stats, aggs: {status, count: new Uint32Array(naggs), sigs}};
  },
  verifyAccumulate: async (ctx, jobs) => {
    calls.push({entry: "verifyAccumulate", jobs});
    await tick();
    const codes = Int32Array.from(jobs.map(codeOf));
    const added = [];
    jobs.forEach((j, i) => {
      for (const s of j.sets) added.push(s.pool !== undefined && codes[i] === 1 && s.pool % 2 === 0 ? 1 : 0);
    });
    return {codes, stats, added: Uint8Array.from(added)};
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

  // two pool callers around a plain two-set job, then an aggregating caller: it starts a new run
  const p1 = v.verifyAndPoolSameMessage(
    [{publicKey: 0, signature: sig(1, 0)}, {publicKey: 1, signature: sig(0, 0)}, {publicKey: 2, signature: sig(2, 0)}],
    ROOT, 4, {batchable: true});
  const plain = v.verifySignatureSets([single(sig(1, 0)), single(sig(1, 0))], {batchable: true});
  const p2 = v.verifyAndPoolSameMessage([{publicKey: 3, signature: sig(1, 0)}, {publicKey: 4, signature: sig(1, 0)}], ROOT, 7);
  const a1 = v.verifyAndAggregateSameMessage([{publicKey: 5, signature: sig(1, 9)}], ROOT);
  const bare = v.verifySignatureSetsSameMessage([{publicKey: 6, signature: sig(1, 0)}], ROOT);
  // ... and a pool caller after it, the reverse
  const p3 = v.verifyAndPoolSameMessage([{publicKey: 8, signature: sig(1, 0)}], ROOT, 6);
  const [r1, rp, r2, ra, rb, r3] = await Promise.all([p1, plain, p2, a1, bare, p3]);
  assert.deepStrictEqual(calls.map((c) => c.entry), ["verifyAccumulate", "verifyAggregate", "verifyAccumulate"]);
  assert.deepStrictEqual(calls[0].jobs.map((j) => [j.sets.length, j.batchable]),
    [[1, true], [1, true], [1, true], [2, true], [1, true], [1, true]]);
  assert.deepStrictEqual(calls[0].jobs.map((j) => j.sets[0].pool), [4, 4, 4, undefined, 7, 7]);
  assert.deepStrictEqual(calls[1].jobs.map((j) => [j.sets[0].agg, j.sets[0].pool]), [[0, undefined], [undefined, undefined]]);
  assert.deepStrictEqual(calls[2].jobs.map((j) => [j.sets[0].agg, j.sets[0].pool]), [[undefined, 6]]);
  assert.ok(calls.every((c) => c.jobs.every((j) => j.sets.every((s) => s.msg === ROOT))));
  assert.deepStrictEqual(r1, [true, false, false]); // an error code is false for its set, not a rejection
  assert.strictEqual(rp, true);
  assert.deepStrictEqual(r2, [false, false]); // accepted, and not added: `added` is read at the SET's index
  assert.deepStrictEqual([ra.results, ra.signature[1]], [[true], 9]);
  assert.deepStrictEqual(rb, [true]);
  assert.deepStrictEqual(r3, [true]);
  assert.deepStrictEqual(await v.verifyAndPoolSameMessage([], ROOT, 4), []);

  // a run with neither kind still goes through addon.verify
  calls.length = 0;
  const r4 = await Promise.all([
    v.verifySignatureSets([single(sig(1, 0))], {batchable: true}),
    v.verifySignatureSetsSameMessage([{publicKey: 1, signature: sig(1, 0)}, {publicKey: 2, signature: sig(2, 0)}], ROOT),
  ]);
  assert.deepStrictEqual(calls.map((c) => c.entry), ["verify"]);
  assert.deepStrictEqual(r4, [true, [true, false]]);
  await v.close();
  await assert.rejects(v.verifyAndPoolSameMessage([{publicKey: 0, signature: sig(1, 0)}], ROOT, 4), /QUEUE_ABORTED/);
  return {cpu: "ok"};
}

// ---- GPU
async function gpuChecks() {
  const {BlsGpuVerifier, addon} = require(path.join(node, "BlsGpuVerifier.js"));
  const N = 8;
  const sks = new Uint8Array(32 * N);
  for (let i = 0; i < N; i++) sks.fill(i + 1, 32 * i, 32 * (i + 1));
  const v = new BlsGpuVerifier({maxBufferWaitMs: 20});
  addon.keygen(v.ctx, sks, 0);
  const msgs = new Uint8Array(32 * N);
  for (let i = 0; i < N; i++) msgs.set(ROOT, 32 * i);
  const all = addon.sign(v.ctx, sks, msgs);
  const sigs = [];
  for (let i = 0; i < N; i++) sigs.push(all.slice(96 * i, 96 * i + 96));
  const set = (k, s) => ({publicKey: k, signature: s === undefined ? sigs[k] : s});
  const report = {};
  const same = (a, b) => assert.deepStrictEqual(Buffer.from(a), Buffer.from(b));

  v.poolOpen(5);
  assert.throws(() => v.poolOpen(5));
  assert.deepStrictEqual(await v.poolGet([5, 6]), [
    {status: -20, count: 0, signature: null}, // BGV_E_EMPTY_AGGREGATE
    {status: -22, count: 0, signature: null}, // BGV_E_BAD_INDEX
  ]);
  // two calls; a wrong signer and an undecodable signature in the second
  assert.deepStrictEqual(await v.verifyAndPoolSameMessage([set(0), set(1), set(2)], ROOT, 5), [true, true, true]);
  let got = await v.poolGet([5]);
  assert.deepStrictEqual([got[0].status, got[0].count], [0, 3]);
  same(got[0].signature, v.aggregateSignatures([sigs[0], sigs[1], sigs[2]]));
  assert.deepStrictEqual(
    await v.verifyAndPoolSameMessage([set(3), set(4, sigs[5]), set(5, sigs[5].slice(0, 95)), set(6)], ROOT, 5),
    [true, false, false, true]);
  got = await v.poolGet(Uint32Array.from([5, 5]));
  assert.deepStrictEqual([got[0].status, got[0].count], [0, 5]);
  same(got[0].signature, v.aggregateSignatures([sigs[0], sigs[1], sigs[2], sigs[3], sigs[6]]));
  same(got[1].signature, got[0].signature);
  report.pool = "ok";

  // a pool caller and an aggregating caller issued together: a run each, both right
  v.poolOpen(6);
  const [pooled, agg] = await Promise.all([
    v.verifyAndPoolSameMessage([set(1), set(7)], ROOT, 6),
    v.verifyAndAggregateSameMessage([set(2), set(3), set(4, sigs[0])], ROOT),
  ]);
  assert.deepStrictEqual(pooled, [true, true]);
  assert.deepStrictEqual(agg.results, [true, true, false]);
  same(agg.signature, v.aggregateSignatures([sigs[2], sigs[3]]));
  got = await v.poolGet([6]);
  assert.strictEqual(got[0].count, 2);
  same(got[0].signature, v.aggregateSignatures([sigs[1], sigs[7]]));
  report.together = "ok";

  // an entry that is not open rejects the call; dropped entries are gone
  await assert.rejects(v.verifyAndPoolSameMessage([set(0)], ROOT, 9));
  assert.strictEqual(v.poolDropRange(0, 16384), 2);
  assert.deepStrictEqual((await v.poolGet([5]))[0], {status: -22, count: 0, signature: null});
  report.drop = "ok";
  await v.close();
  await assert.rejects(v.verifyAndPoolSameMessage([set(0)], ROOT, 5), /QUEUE_ABORTED/);
  assert.throws(() => v.poolOpen(1), /QUEUE_ABORTED/);
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
