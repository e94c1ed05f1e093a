// Synchronous deflate() / inflate() from three N-API environments at once: the main thread and two worker_threads
// Workers.  At these sizes (deflate_bound >= 4 MiB) a synchronous call goes through its environment's page-locked scratch
// block, and every environment must have its own: each result is compared byte for byte with what the main thread
// computed alone, while the second Worker also calls trim() — which releases its own scratch block, nobody else's.
// Run by tests/test_gpu_worker_node.py on the GPU box:  node tests/host_node_worker_test.js
'use strict';
const assert = require('assert');
const { Worker, isMainThread, parentPort, workerData } = require('worker_threads');
const z = require('../zlib.es_amd/host/zlib.js');

const ROUNDS = 6;
const same = (a, b) => Buffer.from(a.buffer, a.byteOffset, a.length).equals(Buffer.from(b.buffer, b.byteOffset, b.length));
function loop(who, input, expect, trimEvery) {
  for (let r = 0; r < ROUNDS; r++) {
    const c = z.deflate(input);
    assert.ok(same(c, expect), who + ': deflate bytes differ in round ' + r);
    assert.ok(same(z.inflate(c), input), who + ': inflate bytes differ in round ' + r);
    if (trimEvery && r % trimEvery === trimEvery - 1) z.trim();
  }
}

if (!isMainThread) {
  parentPort.once('message', () => {
    loop(workerData.who, workerData.input, workerData.expect, workerData.trimEvery);
    parentPort.postMessage('done');
  });
  parentPort.postMessage('ready');
} else {
  const text = new Uint8Array(3 << 20);  // text-like: words of a small vocabulary
  {
    const words = ['the ', 'quick ', 'brown ', 'fox ', 'jumps ', 'over ', 'a ', 'lazy ', 'dog.\n', 'compression ', 'of ', 'blocks, '];
    let s = 0x2545f491 >>> 0;
    for (let i = 0; i < text.length;) {
      s ^= s << 13; s >>>= 0; s ^= s >>> 17; s ^= s << 5; s >>>= 0;
      const w = words[s % words.length];
      for (let k = 0; k < w.length && i < text.length; k++) text[i++] = w.charCodeAt(k);
    }
  }
  const noise = new Uint8Array((3 << 20) + 4096);  // xorshift32 bytes
  {
    let s = 12345;
    for (let i = 0; i < noise.length; i++) {
      s ^= s << 13; s >>>= 0; s ^= s >>> 17; s ^= s << 5; s >>>= 0;
      noise[i] = s & 255;
    }
  }
  const inputs = [text, noise];
  const expects = inputs.map((x) => z.deflate(x));  // alone: nothing else runs yet
  inputs.forEach((x, k) => assert.ok(same(z.inflate(expects[k]), x), 'round trip of input ' + k + ' alone'));

  let ready = 0, done = 0, exited = 0;
  // (workerData is copied, not transferred: a result array's memory belongs to the environment that made it)
  const workers = inputs.map((x, k) => new Worker(__filename, {workerData: {who: 'Worker ' + k, input: x, expect: expects[k], trimEvery: k === 1 ? 2 : 0}}));
  for (const w of workers) {
    w.on('error', (e) => { console.error(e); process.exit(1); });
    w.on('exit', (code) => {
      if (code !== 0) { console.error('a Worker exited with ' + code); process.exit(1); }
      if (++exited < workers.length) return;
      assert.strictEqual(done, workers.length);
      console.log('worker checks passed: ' + ROUNDS + ' rounds on three threads');
    });
    w.on('message', (m) => {
      if (m === 'done') { done++; return; }
      if (++ready < workers.length) return;
      for (const v of workers) v.postMessage('go');
      loop('main thread', inputs[0], expects[0], 0);  // meanwhile
    });
  }
}
