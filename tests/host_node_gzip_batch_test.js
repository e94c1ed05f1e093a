// gzipBatch() / gunzipBatch() of the N-API façade (zlib.es_amd/host/zlib.js): round trips, the files byte for byte those of
// gzip() where it writes and read by Node's own zlib where it does not, per-file Errors on a mixed batch (the call does not
// throw), and the argument errors.  ZES_GZB_DIR (tests/test_gpu_gzip_batch_node.py): the files the Python call gave.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const nodeZlib = require('zlib');
const z = require(path.join(__dirname, '..', 'zlib.es_amd', 'host', 'zlib.js'));

function text(n, seed) {
  const a = new Uint8Array(n);
  let s = seed >>> 0;
  const words = ['alpha ', 'beta ', 'gamma ', 'delta\n', 'epsilon ', 'zeta, '];
  let i = 0;
  while (i < n) {
    s = (s * 1103515245 + 12345) >>> 0;
    const w = words[(s >>> 16) % words.length];
    for (let k = 0; k < w.length && i < n; k++) a[i++] = w.charCodeAt(k);
  }
  return a;
}
const same = (a, b) => Buffer.from(a).equals(Buffer.from(b));

// round trip, and exact bytes against gzip(); the lengths gzip() refuses are stored files
const lens = [0, 1, 2, 17, 1000, 65536, 131072, 131073, 300000];
const inputs = lens.map((n, k) => text(n, 100 + k));
const files = z.gzipBatch(inputs);
assert.strictEqual(files.length, inputs.length);
files.forEach((f, k) => {
  const n = lens[k];
  assert.ok(f instanceof Uint8Array, 'gzipBatch ' + n);
  assert.ok(same(nodeZlib.gunzipSync(f), inputs[k]), 'node reads gzipBatch() ' + n);
  if (n === 0 || n === 1 || n % 131072 === 1) {
    assert.throws(() => z.gzip(inputs[k]), { message: 'Data is corrupted' });
    assert.strictEqual(f.length, 18 + n + 5 * Math.max(1, Math.ceil(n / 65535)), 'stored ' + n);
  } else {
    const g = z.gzip(inputs[k]);
    if (g.length < 18 + n + 5 * Math.max(1, Math.ceil(n / 65535))) assert.ok(same(f, g), 'gzip() bytes ' + n);
    else assert.strictEqual(f.length, 18 + n + 5 * Math.max(1, Math.ceil(n / 65535)), 'stored ' + n);
  }
});
const back = z.gunzipBatch(files);
back.forEach((b, k) => assert.ok(b instanceof Uint8Array && same(b, inputs[k]), 'round trip ' + lens[k]));
assert.deepStrictEqual(z.gzipBatch([]), []);
assert.deepStrictEqual(z.gunzipBatch([]), []);

// a mixed batch: per-file statuses, good neighbours unharmed
const good = new Uint8Array(nodeZlib.gzipSync(inputs[4], { level: 6 }));
const crc = new Uint8Array(good);
crc[crc.length - 8] ^= 1;
const two = new Uint8Array(Buffer.concat([nodeZlib.gzipSync(inputs[3]), nodeZlib.gzipSync(inputs[4])]));
const batch = [good, crc, new Uint8Array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]), two, new Uint8Array(0), files[5]];
const mixed = z.gunzipBatch(batch);
assert.ok(same(mixed[0], inputs[4]) && same(mixed[5], inputs[5]));
assert.ok(mixed[1] instanceof Error && /checksum/.test(mixed[1].message));
assert.ok(mixed[2] instanceof Error && /gzip/.test(mixed[2].message));
assert.ok(same(mixed[3], Buffer.concat([Buffer.from(inputs[3]), Buffer.from(inputs[4])])), 'two members');
assert.ok(mixed[4] instanceof Error && /gzip/.test(mixed[4].message));
for (const k of [1, 2, 4]) assert.throws(() => z.gunzip(batch[k]), { message: mixed[k].message });  // what gunzip() says of the file alone

// argument errors
for (const fn of [z.gzipBatch, z.gunzipBatch]) {
  assert.throws(() => fn(), TypeError);
  assert.throws(() => fn(new Uint8Array(4)), TypeError);
  assert.throws(() => fn([new Uint8Array(4), 'text']), TypeError);
  assert.throws(() => fn([null]), TypeError);
}

// the files of the Python call, byte for byte
const dir = process.env.ZES_GZB_DIR;
if (dir) {
  const exp = JSON.parse(fs.readFileSync(path.join(dir, 'expected.json'), 'utf8'));
  const ins = exp.items.map((it) => new Uint8Array(fs.readFileSync(path.join(dir, it.input))));
  const got = z.gzipBatch(ins);
  exp.items.forEach((it, k) => assert.ok(same(got[k], fs.readFileSync(path.join(dir, it.file))), 'python bytes ' + it.name));
  const outs = z.gunzipBatch(exp.files.map((it) => new Uint8Array(fs.readFileSync(path.join(dir, it.file)))));
  exp.files.forEach((it, k) => {
    if (it.message) assert.ok(outs[k] instanceof Error && outs[k].message === it.message, it.name + ': ' + (outs[k] && outs[k].message));
    else assert.ok(same(outs[k], fs.readFileSync(path.join(dir, it.plain))), it.name);
  });
}
console.log('gzip batch node checks passed');
