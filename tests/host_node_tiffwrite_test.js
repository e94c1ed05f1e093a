// tiffWrite() of the N-API façade (zlib.es_amd/host/zlib.js) on the images tests/test_gpu_tiffwrite_node.py writes into
// ZES_TIFFW_DIR: expected.json lists, per item, the pixel bytes, the info object and the file that the Python form wrote.  The
// bytes must equal the Python form's, and tiffInfo / tiffRead of them must give the info and the pixels back.  Then the
// argument errors.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const z = require(path.join(__dirname, '..', 'zlib.es_amd', 'host', 'zlib.js'));

const dir = process.env.ZES_TIFFW_DIR;
assert.ok(dir, 'ZES_TIFFW_DIR is not set');
const read = (name) => new Uint8Array(fs.readFileSync(path.join(dir, name)));
const expected = JSON.parse(fs.readFileSync(path.join(dir, 'expected.json'), 'utf8'));
assert.ok(expected.items.length >= 5);

let n = 0;
for (const it of expected.items) {
  const pixels = read(it.pixels), want = read(it.file);
  const got = z.tiffWrite(pixels, it.info);
  assert.ok(got instanceof Uint8Array && got.length === want.length, it.name + ': length ' + got.length + ', expected ' + want.length);
  assert.ok(Buffer.from(got).equals(Buffer.from(want)), it.name + ': bytes');
  assert.deepStrictEqual(z.tiffInfo(got), it.info, it.name + ': tiffInfo of the written file');
  const back = z.tiffRead(got);
  assert.deepStrictEqual([back.width, back.height, back.samples, back.bits], [it.info.width, it.info.height, it.info.samples, it.info.bits], it.name);
  assert.ok(Buffer.from(back.data).equals(Buffer.from(pixels)), it.name + ': pixels read back');
  // across, down, size and dirs are optional
  const lean = Object.assign({}, it.info);
  delete lean.across; delete lean.down; delete lean.size; delete lean.dirs;
  assert.ok(Buffer.from(z.tiffWrite(pixels, lean)).equals(Buffer.from(want)), it.name + ': without the computed fields');
  n++;
}

// argument errors: TypeErrors from the façade and the addon, the library's statuses as plain Errors
const first = expected.items[0], px = read(first.pixels);
assert.throws(() => z.tiffWrite(px), TypeError);
assert.throws(() => z.tiffWrite(px, null), TypeError);
assert.throws(() => z.tiffWrite(px, [first.info]), TypeError);
assert.throws(() => z.tiffWrite('no bytes', first.info), TypeError);
assert.throws(() => z.tiffWrite(px, Object.assign({}, first.info, { width: -1 })), TypeError);
assert.throws(() => z.tiffWrite(px, Object.assign({}, first.info, { bits: 8.5 })), TypeError);
assert.throws(() => z.tiffWrite(px.subarray(1), first.info), { name: 'Error', message: expected.arg });
assert.throws(() => z.tiffWrite(px, Object.assign({}, first.info, { photometric: 3 })), { name: 'Error', message: expected.arg });
assert.throws(() => z.tiffWrite(px, Object.assign({}, first.info, { compression: 1, predictor: 2 })), { name: 'Error', message: expected.unsupported });

console.log('tiffwrite node checks passed: ' + n + ' images');
