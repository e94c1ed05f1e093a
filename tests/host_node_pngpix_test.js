// pngPixels() and pngPixelsBatch() of the N-API façade on the GPU.  The fixture comes from the Python side: ZES_PNGPIX_DIR
// holds files of tests/_pngpix.py's tables as <k>.png, expected.json (per file: the pixels' file — computed by the numpy rule
// — and the header's facts, or the messages the file's Error may carry), and the pixel files.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const z = require(path.join(__dirname, '..', 'zlib.es_amd', 'host', 'zlib.js'));

const dir = process.env.ZES_PNGPIX_DIR;
assert.ok(dir, 'ZES_PNGPIX_DIR is not set');
const expected = JSON.parse(fs.readFileSync(path.join(dir, 'expected.json'), 'utf8'));
const files = expected.files.map((f) => new Uint8Array(fs.readFileSync(path.join(dir, f.file))));
const judge = (what, got, want) => {
  if (want.pixels !== undefined) {
    assert.ok(!(got instanceof Error) && got.data instanceof Uint8Array, what + ' is ' + got);
    assert.strictEqual(got.data.length, got.info.width * got.info.height * 4, what + ': width * height * 4 bytes');
    assert.ok(Buffer.from(got.data.buffer, got.data.byteOffset, got.data.length).equals(fs.readFileSync(path.join(dir, want.pixels))), what + ': pixels');
    assert.deepStrictEqual(got.info, want.info, what + ': info');
    assert.deepStrictEqual(got.info, z.pngInfo(files[want.k]), what + ': info is pngInfo\'s');
  } else {
    assert.ok(got instanceof Error && !(got instanceof TypeError), what + ' should be an Error');
    assert.ok(want.messages.includes(got.message), what + ': ' + got.message);
  }
};
// the batch: every file in one call, damaged ones between good ones
const all = z.pngPixelsBatch(files);
assert.ok(Array.isArray(all) && all.length === files.length);
all.forEach((got, k) => judge(expected.files[k].name, got, expected.files[k]));
assert.ok(all.filter((r) => r instanceof Error).length >= 10, 'the damage table should have given Errors');
assert.ok(all.filter((r) => !(r instanceof Error)).length >= 40);
// one file a call: the same, thrown
expected.files.forEach((f, k) => {
  if (k % 4 && f.pixels !== undefined) return;
  let got;
  try {
    got = z.pngPixels(files[k]);
  } catch (e) {
    got = e;
  }
  judge(f.name + ' alone', got, f);
});
// the scanline form beside it: the same records, other bytes
const first = expected.files.findIndex((f) => f.pixels !== undefined);
assert.deepStrictEqual(z.pngDecode(files[first]).info, z.pngPixels(files[first]).info);
// argument errors: TypeErrors, before anything is looked at
const typeError = (fn, message) => assert.throws(fn, (e) => e instanceof TypeError && e.message === message, message);
for (const bad of [undefined, null, 'png', 7, {}, files[0]]) typeError(() => z.pngPixelsBatch(bad), 'pngPixelsBatch(files): files must be an array of Uint8Array');
for (const bad of [[files[0], 'png'], [null], [[files[0]]], [new Float32Array(2)]]) typeError(() => z.pngPixelsBatch(bad), 'pngPixelsBatch(files): every element must be a Uint8Array');
typeError(() => z.pngPixels('png'), 'pngPixelsBatch(files): every element must be a Uint8Array');
assert.deepStrictEqual(z.pngPixelsBatch([]), []);
console.log('pngpix node checks passed');
