// zipRead() of the N-API façade on the GPU.  The fixture comes from the Python side: ZES_ZIP_DIR holds standard.zip and
// failure.zip, expected.json (per archive and entry: the plain bytes' file, or the messages the entry's Error may carry), and
// the plain files.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const z = require(path.join(__dirname, '..', 'zlib.es_amd', 'host', 'zlib.js'));

const dir = process.env.ZES_ZIP_DIR;
assert.ok(dir, 'ZES_ZIP_DIR is not set');
const expected = JSON.parse(fs.readFileSync(path.join(dir, 'expected.json'), 'utf8'));
const judge = (what, got, want, k) => {
  if (want.plain !== undefined) {
    assert.ok(got instanceof Uint8Array, what + ': entry ' + k + ' is ' + got);
    assert.ok(Buffer.from(got.buffer, got.byteOffset, got.length).equals(fs.readFileSync(path.join(dir, want.plain))), what + ': bytes of entry ' + k);
  } else {
    assert.ok(got instanceof Error && !(got instanceof TypeError), what + ': entry ' + k + ' should be an Error');
    assert.ok(want.messages.includes(got.message), what + ': entry ' + k + ': ' + got.message);
  }
};
let errors = 0;
for (const a of expected.archives) {
  const file = new Uint8Array(fs.readFileSync(path.join(dir, a.file)));
  const index = z.zipIndex(file);
  assert.strictEqual(index.entries.length, a.entries.length);
  const all = z.zipRead(file, index);
  assert.ok(Array.isArray(all) && all.length === a.entries.length);
  all.forEach((got, k) => judge(a.file, got, a.entries[k], k));
  errors += all.filter((r) => r instanceof Error).length;
  // a selection: backwards, every second entry, the first one twice — as numbers and as a Uint32Array
  const sel = a.entries.map((_, k) => k).reverse().filter((k) => k % 2 === 0).concat([0, 0]);
  for (const s of [sel, Uint32Array.from(sel)]) {
    const some = z.zipRead(file, index, s);
    assert.strictEqual(some.length, sel.length);
    some.forEach((got, i) => judge(a.file + ' selected', got, a.entries[sel[i]], sel[i]));
  }
  // the index's records are all zipRead looks at
  z.zipRead(file, { raw: index.raw.slice() }, [0]).forEach((got) => judge(a.file + ' raw', got, a.entries[0], 0));
}
assert.ok(errors >= 10, 'the failure archive should have given Errors');
console.log('zip read node checks passed');
