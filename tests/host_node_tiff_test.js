// tiffInfo() / tiffRead() of the N-API façade (zlib.es_amd/host/zlib.js) on the files tests/test_gpu_tiff_node.py writes into
// ZES_TIFF_DIR with tests/_tiff.py: expected.json lists, per item, the file, the call's options, and either the record and the
// pixel bytes the helper's independent reader gives, or the message the call must throw.  Then the argument errors.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const z = require(path.join(__dirname, '..', 'zlib.es_amd', 'host', 'zlib.js'));

const dir = process.env.ZES_TIFF_DIR;
assert.ok(dir, 'ZES_TIFF_DIR is not set');
const read = (name) => new Uint8Array(fs.readFileSync(path.join(dir, name)));
const expected = JSON.parse(fs.readFileSync(path.join(dir, 'expected.json'), 'utf8'));
assert.ok(expected.items.length >= 8);

let good = 0, bad = 0;
for (const it of expected.items) {
  const file = read(it.file);
  if (it.info) {
    const info = it.dir === undefined ? z.tiffInfo(file) : z.tiffInfo(file, it.dir);
    assert.deepStrictEqual(info, it.info, it.name + ': tiffInfo');
  }
  const options = it.options === null ? undefined : it.options;
  if (it.message !== undefined) {
    assert.throws(() => (options === undefined ? z.tiffRead(file) : z.tiffRead(file, options)), { name: 'Error', message: it.message }, it.name);
    if (it.info === undefined) assert.throws(() => z.tiffInfo(file, it.dir), { name: 'Error', message: it.message }, it.name + ': tiffInfo');
    bad++;
    continue;
  }
  const got = options === undefined ? z.tiffRead(file) : z.tiffRead(file, options);
  const want = read(it.pixels);
  assert.deepStrictEqual([got.width, got.height, got.samples, got.bits], it.shape, it.name + ': shape');
  assert.ok(got.data instanceof Uint8Array && got.data.length === want.length, it.name + ': length');
  assert.ok(Buffer.from(got.data).equals(Buffer.from(want)), it.name + ': pixels');
  good++;
}
assert.ok(good >= 5 && bad >= 3);

// argument errors: TypeErrors from the façade and the addon, the library's ZES_E_ARG as a plain Error
const first = read(expected.items[0].file);
assert.throws(() => z.tiffInfo('no bytes'), TypeError);
assert.throws(() => z.tiffInfo(first, -1), TypeError);
assert.throws(() => z.tiffInfo(first, 1.5), TypeError);
assert.throws(() => z.tiffRead(first, 3), TypeError);
assert.throws(() => z.tiffRead(first, [0]), TypeError);
assert.throws(() => z.tiffRead(first, { rect: { x: 0, y: 0, w: 4 } }), TypeError);
assert.throws(() => z.tiffRead(first, { rect: { x: 0, y: 0, w: -4, h: 1 } }), TypeError);
assert.throws(() => z.tiffRead(first, { dir: 'one' }), TypeError);
assert.throws(() => z.tiffRead(first, { rect: { x: 0, y: 0, w: 0, h: 1 } }), { name: 'Error', message: expected.arg });
assert.throws(() => z.tiffRead(first, { rect: { x: 0, y: 0, w: 100000, h: 1 } }), { name: 'Error', message: expected.arg });
assert.throws(() => z.tiffRead(first, { dir: 7 }), { name: 'Error', message: expected.arg });
assert.strictEqual(z.tiffInfo(first).dirs, 1);

console.log('tiff node checks passed: ' + good + ' images, ' + bad + ' refusals');
