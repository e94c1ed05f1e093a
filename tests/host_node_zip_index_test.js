// zipIndex() of the N-API façade, without a device: the entries of the archives the Python side wrote (ZES_ZIP_DIR holds
// <k>.zip and expected.json: per archive what CPython's zipfile lists), the rejected archives with their messages, and the
// façade's TypeErrors for arguments that are not what it asks for.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const z = require(path.join(__dirname, '..', 'zlib.es_amd', 'host', 'zlib.js'));

const dir = process.env.ZES_ZIP_DIR;
assert.ok(dir, 'ZES_ZIP_DIR is not set');
const expected = JSON.parse(fs.readFileSync(path.join(dir, 'expected.json'), 'utf8'));
assert.ok(expected.archives.length >= 8);
expected.archives.forEach((a) => {
  const file = new Uint8Array(fs.readFileSync(path.join(dir, a.file)));
  const index = z.zipIndex(file);
  assert.ok(index.raw instanceof Uint8Array && index.raw.length === 40 * a.entries.length, a.what);
  assert.strictEqual(index.entries.length, a.entries.length, a.what);
  index.entries.forEach((e, k) => {
    const w = a.entries[k];
    assert.deepStrictEqual(Object.keys(e).sort(), ['compressedSize', 'crc32', 'flags', 'method', 'name', 'nameBytes', 'size'], a.what);
    assert.ok(e.nameBytes instanceof Uint8Array && Buffer.from(e.nameBytes).toString('hex') === w.nameHex, a.what + ': nameBytes of entry ' + k);
    assert.deepStrictEqual([e.name, e.method, e.flags, e.compressedSize, e.size, e.crc32], [w.name, w.method, w.flags, w.csize, w.usize, w.crc], a.what + ': entry ' + k);
    const view = new DataView(index.raw.buffer, index.raw.byteOffset + 40 * k, 40);
    assert.strictEqual(Number(view.getBigUint64(0, true)), w.hdr_off, a.what + ': header offset of entry ' + k);
  });
});
expected.rejects.forEach((r) => {
  const file = new Uint8Array(fs.readFileSync(path.join(dir, r.file)));
  assert.throws(() => z.zipIndex(file), (e) => e instanceof Error && !(e instanceof TypeError) && e.message === r.message, r.what);
});
// a name without flag bit 11 is its bytes as code points, whatever they are
assert.strictEqual(z.zipIndex(new Uint8Array(fs.readFileSync(path.join(dir, expected.latin1.file)))).entries[0].name, expected.latin1.name);

for (const bad of [undefined, null, 'text', 5, [80, 75], {}, new Uint16Array(22)]) assert.throws(() => z.zipIndex(bad), TypeError);
const file = new Uint8Array(fs.readFileSync(path.join(dir, expected.archives[0].file)));
const index = z.zipIndex(file);
for (const bad of [undefined, null, 'text', 7, {}, { raw: [1, 2] }, { raw: new Uint8Array(39) }, { entries: index.entries }])
  assert.throws(() => z.zipRead(file, bad), TypeError);
assert.throws(() => z.zipRead('text', index), TypeError);
for (const bad of ['0', 1, {}, [0.5], [-1], ['0'], [2 ** 32], new Uint8Array(1), new Int32Array(1), new Float64Array(1)])
  assert.throws(() => z.zipRead(file, index, bad), TypeError);
assert.throws(() => z.zipRead(file, index, [index.entries.length]), (e) => !(e instanceof TypeError) && /bad argument/.test(e.message));
// nothing selected: nothing to do, and no device is asked for
assert.deepStrictEqual(z.zipRead(file, index, []), []);
assert.deepStrictEqual(z.zipRead(file, index, new Uint32Array(0)), []);
console.log('zip index node checks passed');
