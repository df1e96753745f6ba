"use strict";
// poolOpen(id, {nBits}) / verifyAndPoolBitsSameMessage / poolGetBits / poolSum of BlsGpuVerifier
// (tests/test_node_sigpool_bits.py).
//   node tests/node/sigpool_bits.js cpu   against a mock addon (no GPU): how a bits caller's sets
//                                         travel, how outcomes come back, and that a buffered run
//                                         holds one kind of caller
//   node tests/node/sigpool_bits.js       on the device: a duplicate within one call and one across
//                                         calls, poolGetBits, and poolSum of four 128-position
//                                         entries (one empty) against aggregateSignatures
const assert = require("assert");
const path = require("path");
const node = path.join(__dirname, "..", "..", "lodestar_amd", "node");
const addonPath = path.join(node, "blsgpu.node");

const ROOT = new Uint8Array(32).fill(0x5a);

// ---- CPU: a mock addon that accepts a set iff its signature's first byte is 1 and reports the
// outcome its second byte names
const calls = [];
const stats = {batchRetries: 0, batchSigsSuccess: 0, deviceMs: 0};
const tick = () => new Promise((r) => setTimeout(r, 2));
const mock = {
  init: () => ({}),
  close: () => {},
  strerror: (c) => "code " + c,
  verify: async (ctx, jobs) => {
    calls.push({entry: "verify", jobs});
    await tick();
    return Int32Array.from(jobs.map((j) => (j.sets[0].sig[0] === 1 ? 1 : 0)));
  },
  verifyAccumulate: async (ctx, jobs) => {
    calls.push({entry: "verifyAccumulate", jobs});
    await tick();
    const codes = Int32Array.from(jobs.map((j) => (j.sets[0].sig[0] === 1 ? 1 : 0)));
    return {codes, stats, added: Uint8Array.from(codes)};
  },
  verifyAccumulateBits: async (ctx, jobs) => {
    calls.push({entry: "verifyAccumulateBits", jobs});
    await tick();
    const codes = Int32Array.from(jobs.map((j) => (j.sets[0].sig[0] === 2 ? -8 : j.sets[0].sig[0] === 1 ? 1 : 0)));
    const outcome = [];
    jobs.forEach((j, i) => {
      for (const s of j.sets) outcome.push(codes[i] === 1 && s.pool !== undefined ? s.sig[1] : 0);
    });
    return {codes, stats, outcome: Uint8Array.from(outcome)};
  },
  sigpoolOpen: (ctx, id) => calls.push({entry: "sigpoolOpen", id}),
  sigpoolOpenBits: (ctx, id, nBits) => calls.push({entry: "sigpoolOpenBits", id, nBits}),
  sigpoolSum: async (ctx, ids, lengths) => {
    calls.push({entry: "sigpoolSum", ids: Array.from(ids), lengths: Array.from(lengths)});
    const n = lengths.length;
    const bits = new Uint8Array(512 * n);
    bits[0] = 0x81;
    bits[512] = 0xff;
    bits[513] = 0x01;
    return {status: Int32Array.from([0, -20]), count: Uint32Array.from([3, 0]), sigs: new Uint8Array(96 * n).fill(7),
      bits, nBits: Uint32Array.from([8, 9]), stride: 512};
  },
};

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
  v.poolOpen(3, {nBits: 130});
  v.poolOpen(4);
  assert.deepStrictEqual(calls.splice(0), [{entry: "sigpoolOpenBits", id: 3, nBits: 130}, {entry: "sigpoolOpen", id: 4}]);

  const field = Uint8Array.from([3]);
  // a bits caller, a plain job, a second bits caller; then a pool caller: it starts a new run
  const b1 = v.verifyAndPoolBitsSameMessage(
    [{publicKey: 0, signature: sig(1, 1), bit: 5}, {publicKey: 1, signature: sig(1, 2), bit: 5},
      {publicKey: 2, signature: sig(0, 1), bit: 6}, {publicKey: 3, signature: sig(2, 1), bit: 7}],
    ROOT, 3, {nBits: 130});
  const plain = v.verifySignatureSets([{type: "single", pubkey: 7, signingRoot: ROOT, signature: sig(1, 0)}], {batchable: true});
  const b2 = v.verifyAndPoolBitsSameMessage([{publicKey: 4, signature: sig(1, 3), bits: field}], ROOT, 9, {nBits: 8});
  const p1 = v.verifyAndPoolSameMessage([{publicKey: 5, signature: sig(1, 0)}], ROOT, 4);
  const b3 = v.verifyAndPoolBitsSameMessage([{publicKey: 6, signature: sig(1, 1), bit: 0}], ROOT, 3, {nBits: 130});
  const [r1, rp, r2, q1, r3] = await Promise.all([b1, plain, b2, p1, b3]);
  assert.deepStrictEqual(calls.map((c) => c.entry), ["verifyAccumulateBits", "verifyAccumulate", "verifyAccumulateBits"]);
  const tagsOf = (c) => c.jobs.map((j) => [j.sets[0].pool, j.sets[0].poolNBits, j.sets[0].poolBit, j.sets[0].poolBits]);
  assert.deepStrictEqual(tagsOf(calls[0]), [
    [3, 130, 5, undefined], [3, 130, 5, undefined], [3, 130, 6, undefined], [3, 130, 7, undefined],
    [undefined, undefined, undefined, undefined], [9, 8, undefined, field]]);
  assert.deepStrictEqual(tagsOf(calls[1]), [[4, undefined, undefined, undefined]]);
  assert.deepStrictEqual(tagsOf(calls[2]), [[3, 130, 0, undefined]]);
  assert.ok(calls.every((c) => c.jobs.every((j) => j.batchable === true && j.sets[0].msg === ROOT)));
  // valid is the verdict, whatever the entry did; an error code is not a rejection
  assert.deepStrictEqual(r1, [{valid: true, outcome: "added"}, {valid: true, outcome: "known"},
    {valid: false, outcome: null}, {valid: false, outcome: null}]);
  assert.strictEqual(rp, true);
  assert.deepStrictEqual(r2, [{valid: true, outcome: "overlap"}]); // read at the SET's index, past the plain job
  assert.deepStrictEqual(q1, [true]);
  assert.deepStrictEqual(r3, [{valid: true, outcome: "added"}]);
  assert.deepStrictEqual(await v.verifyAndPoolBitsSameMessage([], ROOT, 3, {nBits: 130}), []);

  calls.length = 0;
  const sums = await v.poolSum([[1, 2, 3], Uint32Array.from([9])]);
  assert.deepStrictEqual(calls, [{entry: "sigpoolSum", ids: [1, 2, 3, 9], lengths: [3, 1]}]);
  assert.deepStrictEqual(sums.map((s) => [s.status, s.count, s.signature && s.signature.length, s.nBits, Array.from(s.bits)]),
    [[0, 3, 96, 8, [0x81]], [-20, 0, null, 9, [0xff, 0x01]]]);
  await v.close();
  await assert.rejects(v.verifyAndPoolBitsSameMessage([{publicKey: 0, signature: sig(1, 1), bit: 0}], ROOT, 3, {nBits: 130}),
    /QUEUE_ABORTED/);
  return {cpu: "ok"};
}

// ---- GPU
async function gpuChecks() {
  const {BlsGpuVerifier, addon} = require(path.join(node, "BlsGpuVerifier.js"));
  const N = 12;
  const sks = new Uint8Array(32 * N);
  for (let i = 0; i < N; i++) sks.fill(i + 1, 32 * i, 32 * (i + 1));
  const v = new BlsGpuVerifier({maxBufferWaitMs: 20});
  addon.keygen(v.ctx, sks, 0);
  const msgs = new Uint8Array(32 * N);
  for (let i = 0; i < N; i++) msgs.set(ROOT, 32 * i);
  const all = addon.sign(v.ctx, sks, msgs);
  const sigs = [];
  for (let i = 0; i < N; i++) sigs.push(all.slice(96 * i, 96 * i + 96));
  const set = (k, bit, s) => ({publicKey: k, signature: s === undefined ? sigs[k] : s, bit});
  const report = {};
  const same = (a, b) => assert.deepStrictEqual(Buffer.from(a), Buffer.from(b));
  const field = (positions, n) => {
    const b = new Uint8Array((n + 7) >> 3);
    for (const k of positions) b[k >> 3] |= 1 << (k & 7);
    return b;
  };
  const added = {valid: true, outcome: "added"};
  const known = {valid: true, outcome: "known"};

  // a duplicate within one call, one across calls, a wrong signer and an undecodable signature
  v.poolOpen(5, {nBits: 130});
  assert.throws(() => v.poolOpen(5, {nBits: 130}));
  let got = await v.poolGetBits([5, 6]);
  assert.deepStrictEqual([got[0].status, got[0].count, got[0].signature, got[0].nBits], [-20, 0, null, 130]);
  same(got[0].bits, new Uint8Array(17));
  assert.deepStrictEqual([got[1].status, got[1].nBits, got[1].bits.length], [-22, 0, 0]);
  assert.deepStrictEqual(
    await v.verifyAndPoolBitsSameMessage([set(0, 0), set(1, 129), set(0, 0), set(2, 64)], ROOT, 5, {nBits: 130}),
    [added, added, known, added]);
  assert.deepStrictEqual(
    await v.verifyAndPoolBitsSameMessage(
      [set(1, 129), set(3, 7), set(4, 8, sigs[5]), set(5, 9, sigs[5].slice(0, 95)),
        {publicKey: 6, signature: sigs[6], bits: field([0, 100], 130)}],
      ROOT, 5, {nBits: 130}),
    [known, added, {valid: false, outcome: null}, {valid: false, outcome: null}, {valid: true, outcome: "overlap"}]);
  got = await v.poolGetBits(Uint32Array.from([5]));
  assert.deepStrictEqual([got[0].status, got[0].count, got[0].nBits], [0, 4, 130]);
  same(got[0].bits, field([0, 129, 64, 7], 130));
  same(got[0].signature, v.aggregateSignatures([sigs[0], sigs[1], sigs[2], sigs[3]]));
  same((await v.poolGet([5]))[0].signature, got[0].signature);
  // n_bits that is not the entry's rejects the call
  await assert.rejects(v.verifyAndPoolBitsSameMessage([set(7, 1)], ROOT, 5, {nBits: 128}));
  report.bits = "ok";

  // four subnets of 128 positions, the third without a contribution
  for (const id of [10, 11, 12, 13]) v.poolOpen(id, {nBits: 128});
  const fill = [[10, [[7, 0], [8, 127]]], [11, [[9, 5]]], [13, [[10, 1], [11, 2]]]];
  for (const [id, members] of fill) {
    const res = await v.verifyAndPoolBitsSameMessage(members.map(([k, bit]) => set(k, bit)), ROOT, id, {nBits: 128});
    assert.deepStrictEqual(res, members.map(() => added));
  }
  const sums = await v.poolSum([[10, 11, 12, 13], [12], [11, 5]]);
  assert.deepStrictEqual(sums.map((s) => [s.status, s.count, s.nBits]), [[0, 5, 512], [-20, 0, 128], [0, 5, 258]]);
  same(sums[0].signature, v.aggregateSignatures([7, 8, 9, 10, 11].map((k) => sigs[k])));
  same(sums[0].bits, field([0, 127, 128 + 5, 384 + 1, 384 + 2], 512));
  assert.strictEqual(sums[1].signature, null);
  same(sums[1].bits, new Uint8Array(16));
  same(sums[2].signature, v.aggregateSignatures([9, 0, 1, 2, 3].map((k) => sigs[k])));
  same(sums[2].bits, field([5, 128 + 0, 128 + 129, 128 + 64, 128 + 7], 258));
  same((await v.poolGetBits([10]))[0].bits, field([0, 127], 128)); // a sum changes nothing
  assert.deepStrictEqual((await v.poolSum([[10, 99], [13]])).map((s) => [s.status, s.count]), [[-22, 0], [0, 2]]);
  await assert.rejects(v.poolSum([[10, 16384]])); // an id past the end rejects the call
  report.sum = "ok";

  assert.strictEqual(v.poolDropRange(0, 16384), 5);
  assert.deepStrictEqual((await v.poolGetBits([5]))[0].status, -22);
  await v.close();
  await assert.rejects(v.verifyAndPoolBitsSameMessage([set(0, 0)], ROOT, 5, {nBits: 130}), /QUEUE_ABORTED/);
  assert.throws(() => v.poolOpen(1, {nBits: 8}), /QUEUE_ABORTED/);
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
