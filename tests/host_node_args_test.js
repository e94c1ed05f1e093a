// What the façade zlib.es_amd/host/zlib.js throws for arguments it cannot take, before any device is touched: the
// constructor and the exact message of every case, once on the main thread and once inside a worker_threads Worker (an
// N-API environment of its own).  Run by tests/test_host_cpu.py:  node tests/host_node_args_test.js
'use strict';
const assert = require('assert');
const { Worker, isMainThread } = require('worker_threads');
const z = require('../zlib.es_amd/host/zlib.js');

function run() {
  let n = 0;
  // f throws synchronously (the Async forms too: a bad argument is thrown, not a rejection) an error of exactly this kind
  function throwsExactly(f, ctor, msg, what) {
    let got = null, ret;
    try { ret = f(); } catch (e) { got = e; }
    if (ret && typeof ret.then === 'function') ret.catch(() => {});
    assert.ok(got !== null, what + ': nothing was thrown');
    assert.strictEqual(Object.getPrototypeOf(got), ctor.prototype, what + ': thrown ' + (got && got.constructor && got.constructor.name));
    assert.strictEqual(got.message, msg, what);
    n++;
  }
  const u = new Uint8Array(8);
  const idx = {compressed: new BigUint64Array(2), uncompressed: new BigUint64Array(2)};

  // group 1: "<sig>: input must be a Uint8Array"
  const inputMsg = (sig) => sig + ': input must be a Uint8Array';
  throwsExactly(() => z.deflate(), TypeError, inputMsg('deflate(input)'), 'deflate()');
  for (const bad of ['x', new Uint16Array(4), new ArrayBuffer(8)])
    throwsExactly(() => z.deflate(bad), TypeError, inputMsg('deflate(input)'), 'deflate(' + Object.prototype.toString.call(bad) + ')');
  for (const [name, sig] of [['inflate', 'inflate(input)'], ['deflateRaw', 'deflateRaw(input)'], ['inflateRaw', 'inflateRaw(input, offset)'],
                             ['gzip', 'gzip(input)'], ['gunzip', 'gunzip(input)'], ['bgzip', 'bgzip(input)'], ['bgzipIndex', 'bgzipIndex(input)'],
                             ['adler32', 'adler32(input)'], ['deflateAsync', 'deflateAsync(input)'], ['inflateAsync', 'inflateAsync(input)']])
    throwsExactly(() => z[name]('x'), TypeError, inputMsg(sig), name + "('x')");

  // group 2: the other TypeErrors
  const READ = 'bgzfRead(file, index, pos, len): ';
  throwsExactly(() => z.bgzfIndex('x'), TypeError, 'bgzfIndex(file): file must be a Uint8Array', "bgzfIndex('x')");
  throwsExactly(() => z.bgzfRead('x', idx, 0, 1), TypeError, READ + 'file must be a Uint8Array', "bgzfRead('x', ...)");
  throwsExactly(() => z.bgzfRead(u, {compressed: [0], uncompressed: [0]}, 0, 1), TypeError, READ + 'index must be what bgzfIndex(file) returned', 'bgzfRead: plain arrays as index');
  throwsExactly(() => z.bgzfRead(u, {compressed: new BigUint64Array(1), uncompressed: new BigUint64Array(1)}, 0, 1), TypeError,
                READ + 'index must be what bgzfIndex(file) returned', 'bgzfRead: one-entry index');
  throwsExactly(() => z.bgzfRead(u, idx, -1, 1), TypeError, READ + 'pos and len must be non-negative safe integers or bigints', 'bgzfRead: pos -1');
  throwsExactly(() => z.bgzfRead(u, idx, 0), TypeError, READ + 'pos and len must be non-negative safe integers or bigints', 'bgzfRead: no len');
  for (const bad of [-1, 1.5, NaN, '1', 1n, null])
    throwsExactly(() => z.inflateRaw(u, bad), TypeError, 'inflateRaw(input, offset): offset must be a non-negative safe integer', 'inflateRaw(u, ' + typeof bad + ' ' + String(bad) + ')');
  throwsExactly(() => z.deflateBatch(u), TypeError, 'batch(inputs): inputs must be an array of Uint8Array', 'deflateBatch(u)');
  throwsExactly(() => z.deflateBatch([u, 5]), TypeError, 'batch(inputs): every element must be a Uint8Array', 'deflateBatch([u, 5])');
  throwsExactly(() => z.inflateBatchAsync([5]), TypeError, 'batch(inputs): every element must be a Uint8Array', 'inflateBatchAsync([5])');
  for (const bad of [-1, 1.5, '4'])
    throwsExactly(() => z.allocPinned(bad), TypeError, 'allocPinned(n): n must be a non-negative integer', 'allocPinned(' + typeof bad + ' ' + bad + ')');

  // group 3: plain Errors from the library's host-side argument rules
  throwsExactly(() => z.deflate(new Uint8Array(0)), Error, 'Data is corrupted', 'deflate of 0 bytes');
  throwsExactly(() => z.deflate(new Uint8Array(1)), Error, 'Data is corrupted', 'deflate of 1 byte');
  throwsExactly(() => z.deflateRaw(new Uint8Array(1)), Error, 'Data is corrupted', 'deflateRaw of 1 byte');
  throwsExactly(() => z.gzip(new Uint8Array(1)), Error, 'Data is corrupted', 'gzip of 1 byte');
  for (const empty of [new Uint8Array(0), Buffer.alloc(0), new Int8Array(0), new Uint8ClampedArray(0)])
    throwsExactly(() => z.inflate(empty), Error, 'Not compressed by deflate', 'inflate of an empty ' + empty.constructor.name);
  return n;
}

const where = isMainThread ? 'main thread' : 'Worker';
console.log(run() + ' argument checks passed on the ' + where);
if (isMainThread) {
  const w = new Worker(__filename);
  w.on('error', (e) => { console.error(e); process.exit(1); });
  w.on('exit', (code) => {
    if (code !== 0) { console.error('Worker exited with ' + code); process.exit(1); }
    console.log('argument checks passed on both threads');
  });
}
