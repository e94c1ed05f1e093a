// The `{ interlaced }` option of pngDecodeBatch(), pngDecode(), pngPixelsBatch() and pngPixels() of the N-API façade on the
// GPU.  The fixture comes from the Python side: ZES_ADAM7_DIR holds interlaced and plain files as <k>.png, expected.json (per
// file: whether it is interlaced, and the files that hold its scanlines and its pixels; and the message of the status an
// interlaced file gets without the option).
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const z = require(path.join(__dirname, '..', 'zlib.es_amd', 'host', 'zlib.js'));

const dir = process.env.ZES_ADAM7_DIR;
assert.ok(dir, 'ZES_ADAM7_DIR is not set');
const expected = JSON.parse(fs.readFileSync(path.join(dir, 'expected.json'), 'utf8'));
const files = expected.files.map((f) => new Uint8Array(fs.readFileSync(path.join(dir, f.file))));
const same = (what, got, file) => {
  assert.ok(!(got instanceof Error) && got.data instanceof Uint8Array, what + ' is ' + got);
  assert.ok(Buffer.from(got.data.buffer, got.data.byteOffset, got.data.length).equals(fs.readFileSync(path.join(dir, file))), what + ': bytes');
};
const refused = (what, got) => assert.ok(got instanceof Error && !(got instanceof TypeError) && got.message === expected.unsupported, what + ': ' + got);
const caught = (fn) => {
  try {
    return fn();
  } catch (e) {
    return e;
  }
};
assert.ok(expected.files.some((f) => f.interlaced) && expected.files.some((f) => !f.interlaced));
// with the option: every file, interlaced or not, in one batch
const rows = z.pngDecodeBatch(files, { interlaced: true });
const pixels = z.pngPixelsBatch(files, { interlaced: true });
assert.ok(rows.length === files.length && pixels.length === files.length);
expected.files.forEach((f, k) => {
  same(f.name + ': scanlines', rows[k], f.rows);
  same(f.name + ': pixels', pixels[k], f.pixels);
  assert.strictEqual(rows[k].info.interlace, f.interlaced ? 1 : 0);
  assert.strictEqual(pixels[k].data.length, rows[k].info.width * rows[k].info.height * 4);
});
// one file a call
expected.files.forEach((f, k) => {
  if (k % 4) return;
  same(f.name + ' alone: scanlines', z.pngDecode(files[k], { interlaced: true }), f.rows);
  same(f.name + ' alone: pixels', z.pngPixels(files[k], { interlaced: true }), f.pixels);
});
// without the option, or with it off: the interlaced ones are refused, the others decode
for (const opt of [[], [undefined], [{}], [{ interlaced: false }], [{ interlaced: 1 }]]) {
  const r = z.pngDecodeBatch(files, ...opt), p = z.pngPixelsBatch(files, ...opt);
  expected.files.forEach((f, k) => {
    if (f.interlaced) {
      refused(f.name + ' without the option', r[k]);
      refused(f.name + ' without the option (pixels)', p[k]);
    } else {
      same(f.name, r[k], f.rows);
      same(f.name, p[k], f.pixels);
    }
  });
}
const first = expected.files.findIndex((f) => f.interlaced);
refused('pngDecode', caught(() => z.pngDecode(files[first])));
refused('pngPixels', caught(() => z.pngPixels(files[first])));
// a second argument that is not an object: a TypeError
const typeError = (fn, message) => assert.throws(fn, (e) => e instanceof TypeError && e.message === message, message);
for (const bad of [null, true, 1, 'interlaced', [], [{ interlaced: true }]]) {
  typeError(() => z.pngDecodeBatch(files, bad), 'pngDecodeBatch(files): options must be an object { interlaced?: boolean }');
  typeError(() => z.pngDecode(files[0], bad), 'pngDecodeBatch(files): options must be an object { interlaced?: boolean }');
  typeError(() => z.pngPixelsBatch(files, bad), 'pngPixelsBatch(files): options must be an object { interlaced?: boolean }');
  typeError(() => z.pngPixels(files[0], bad), 'pngPixelsBatch(files): options must be an object { interlaced?: boolean }');
}
// the first argument is judged as before
typeError(() => z.pngDecodeBatch('png', { interlaced: true }), 'pngDecodeBatch(files): files must be an array of Uint8Array');
typeError(() => z.pngPixelsBatch([null], { interlaced: true }), 'pngPixelsBatch(files): every element must be a Uint8Array');
assert.deepStrictEqual(z.pngDecodeBatch([], { interlaced: true }), []);
assert.strictEqual(z.pngDecodeBatch.length, 1);
console.log('adam7 node checks passed');
