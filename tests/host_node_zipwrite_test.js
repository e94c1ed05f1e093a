// zip() of the N-API façade on the GPU.  The fixture comes from the Python side: ZES_ZIP_DIR holds expected.json (the files:
// per file its name as a string or, as hex, as bytes, and the file that holds its data) and want.zip, the archive that the
// builder of tests/_zip.py and the CPU oracle give for them.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const z = require(path.join(__dirname, '..', 'zlib.es_amd', 'host', 'zlib.js'));

const dir = process.env.ZES_ZIP_DIR;
assert.ok(dir, 'ZES_ZIP_DIR is not set');
const expected = JSON.parse(fs.readFileSync(path.join(dir, 'expected.json'), 'utf8'));
const files = expected.files.map((f) => ({
  name: f.name !== undefined ? f.name : Uint8Array.from(Buffer.from(f.nameHex, 'hex')),
  data: new Uint8Array(fs.readFileSync(path.join(dir, f.data))),
}));
assert.ok(files.some((f) => typeof f.name === 'string') && files.some((f) => f.name instanceof Uint8Array));
const want = fs.readFileSync(path.join(dir, 'want.zip'));
const got = z.zip(files);
assert.ok(got instanceof Uint8Array && got.length === want.length, 'zip(files) has ' + got.length + ' bytes, expected ' + want.length);
assert.ok(Buffer.from(got.buffer, got.byteOffset, got.length).equals(want), 'zip(files) differs from the expected archive');
// the same bytes a second time, and from the names as bytes
const asBytes = files.map((f) => ({ name: typeof f.name === 'string' ? new TextEncoder().encode(f.name) : f.name, data: f.data }));
for (const again of [z.zip(files), z.zip(asBytes)]) assert.ok(Buffer.from(again).equals(want), 'a second zip() differs');
// and back through the reader
const index = z.zipIndex(got);
assert.strictEqual(index.entries.length, files.length);
index.entries.forEach((e, k) => {
  const name = files[k].name;
  if (typeof name === 'string') assert.strictEqual(e.name, name, 'name of entry ' + k);
  else assert.ok(Buffer.from(e.nameBytes).equals(Buffer.from(name)), 'name bytes of entry ' + k);
  assert.strictEqual(e.size, files[k].data.length);
  assert.strictEqual(e.method, expected.files[k].method, 'method of entry ' + k);
});
z.zipRead(got, index).forEach((r, k) => {
  assert.ok(r instanceof Uint8Array, 'entry ' + k + ' is ' + r);
  assert.ok(Buffer.from(r.buffer, r.byteOffset, r.length).equals(Buffer.from(files[k].data)), 'bytes of entry ' + k);
});
assert.ok(Buffer.from(z.zip([])).equals(Buffer.concat([Buffer.from('PK\x05\x06', 'latin1'), Buffer.alloc(18)])));
console.log('zip write node checks passed');
