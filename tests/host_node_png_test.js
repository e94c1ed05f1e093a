// pngInfo(), pngDecode() and pngDecodeBatch() of the N-API façade on the GPU.  The fixture comes from the Python side:
// ZES_PNG_DIR holds the files of tests/_png.py's tables as <k>.png, expected.json (per file: the scanlines' file and the
// header's facts, or the messages the file's Error may carry; and what pngInfo answers), and the scanline files.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const z = require(path.join(__dirname, '..', 'zlib.es_amd', 'host', 'zlib.js'));

const dir = process.env.ZES_PNG_DIR;
assert.ok(dir, 'ZES_PNG_DIR is not set');
const expected = JSON.parse(fs.readFileSync(path.join(dir, 'expected.json'), 'utf8'));
const files = expected.files.map((f) => new Uint8Array(fs.readFileSync(path.join(dir, f.file))));
const judge = (what, got, want) => {
  if (want.plain !== undefined) {
    assert.ok(!(got instanceof Error) && got.data instanceof Uint8Array, what + ' is ' + got);
    assert.ok(Buffer.from(got.data.buffer, got.data.byteOffset, got.data.length).equals(fs.readFileSync(path.join(dir, want.plain))), what + ': bytes');
    assert.deepStrictEqual(got.info, want.info, what + ': info');
  } else {
    assert.ok(got instanceof Error && !(got instanceof TypeError), what + ' should be an Error');
    assert.ok(want.messages.includes(got.message), what + ': ' + got.message);
  }
};
// the batch: every file of both tables in one call, damaged ones between good ones
const all = z.pngDecodeBatch(files);
assert.ok(Array.isArray(all) && all.length === files.length);
all.forEach((got, k) => judge(expected.files[k].name, got, expected.files[k]));
assert.ok(all.filter((r) => r instanceof Error).length >= 15, 'the damage table should have given Errors');
assert.ok(all.filter((r) => !(r instanceof Error)).length >= 40);
// one file a call: the same, thrown
expected.files.forEach((f, k) => {
  if (k % 5 && f.plain !== undefined) return;
  let got;
  try {
    got = z.pngDecode(files[k]);
  } catch (e) {
    got = e;
  }
  judge(f.name + ' alone', got, f);
});
// pngInfo: the host rule, no CRC
expected.files.forEach((f, k) => {
  if (f.infoMessage !== undefined) assert.throws(() => z.pngInfo(files[k]), (e) => e instanceof Error && !(e instanceof TypeError) && e.message === f.infoMessage, f.name);
  else assert.deepStrictEqual(z.pngInfo(files[k]), f.info, f.name + ': pngInfo');
});
// argument errors: TypeErrors, before anything is looked at
const typeError = (fn, message) => assert.throws(fn, (e) => e instanceof TypeError && e.message === message, message);
for (const bad of [undefined, null, 'png', 7, [1, 2], {}, new Uint16Array(4)]) typeError(() => z.pngInfo(bad), 'pngInfo(file): file must be a Uint8Array');
for (const bad of [undefined, null, 'png', 7, {}, files[0]]) typeError(() => z.pngDecodeBatch(bad), 'pngDecodeBatch(files): files must be an array of Uint8Array');
for (const bad of [[files[0], 'png'], [null], [[files[0]]], [new Float32Array(2)]]) typeError(() => z.pngDecodeBatch(bad), 'pngDecodeBatch(files): every element must be a Uint8Array');
typeError(() => z.pngDecode('png'), 'pngDecodeBatch(files): every element must be a Uint8Array');
assert.deepStrictEqual(z.pngDecodeBatch([]), []);
console.log('png node checks passed');
