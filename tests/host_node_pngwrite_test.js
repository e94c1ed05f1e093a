// pngEncode() and pngEncodeBatch() of the N-API façade on the GPU.  The fixture comes from the Python side: ZES_PNGW_DIR holds
// expected.json (per image: its record, the scanlines' file, the file the Python call made of it or the message its Error
// carries) and the files it names.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const z = require(path.join(__dirname, '..', 'zlib.es_amd', 'host', 'zlib.js'));

const dir = process.env.ZES_PNGW_DIR;
assert.ok(dir, 'ZES_PNGW_DIR is not set');
const expected = JSON.parse(fs.readFileSync(path.join(dir, 'expected.json'), 'utf8'));
const read = (f) => new Uint8Array(fs.readFileSync(path.join(dir, f)));
const images = expected.images.map((m) => Object.assign({}, m.image, { data: read(m.rows) },
  m.palette ? { palette: read(m.palette) } : {}, m.transparency ? { transparency: read(m.transparency) } : {}));
const same = (a, b) => Buffer.from(a.buffer, a.byteOffset, a.length).equals(Buffer.from(b.buffer, b.byteOffset, b.length));
// the batch: byte equality with the Python result, an Error in the place of a record that is refused
const all = z.pngEncodeBatch(images);
assert.ok(Array.isArray(all) && all.length === images.length);
let good = 0;
all.forEach((got, k) => {
  const m = expected.images[k];
  if (m.png !== undefined) {
    assert.ok(got instanceof Uint8Array, m.name + ' is ' + got);
    assert.ok(same(got, read(m.png)), m.name + ': bytes');
    good++;
    // the round trip through pngDecode
    const back = z.pngDecode(got);
    assert.ok(same(back.data, images[k].data), m.name + ': round trip');
    assert.strictEqual(back.info.width, m.image.width);
    assert.strictEqual(back.info.height, m.image.height);
    assert.strictEqual(back.info.colourType, m.image.colourType);
  } else {
    assert.ok(got instanceof Error && !(got instanceof TypeError) && got.message === m.message, m.name + ': ' + got);
  }
});
assert.ok(good >= 3 && good < all.length);
// one image a call: the same bytes; a refused one throws
expected.images.forEach((m, k) => {
  if (m.png !== undefined) assert.ok(same(z.pngEncode(images[k]), read(m.png)), m.name + ' alone');
  else assert.throws(() => z.pngEncode(images[k]), (e) => e instanceof Error && !(e instanceof TypeError) && e.message === m.message, m.name);
});
// the defaults: depth 8, filter 5
const first = expected.images.findIndex((m) => m.png !== undefined && m.image.depth === 8 && m.image.filter === 5);
assert.ok(first >= 0);
const { depth, filter, ...bare } = images[first];
assert.ok(same(z.pngEncode(bare), read(expected.images[first].png)), 'defaults');
// argument errors: TypeErrors, before anything is looked at
const typeError = (fn, message) => assert.throws(fn, (e) => e instanceof TypeError && e.message === message, message);
for (const bad of [undefined, null, 'png', 7, {}, images[0]]) typeError(() => z.pngEncodeBatch(bad), 'pngEncodeBatch(images): images must be an array of { data, width, height, colourType }');
for (const bad of [[null], ['png'], [7]]) typeError(() => z.pngEncodeBatch(bad), 'pngEncodeBatch(images): every image must be an object');
typeError(() => z.pngEncodeBatch([Object.assign({}, images[0], { width: -1 })]), 'pngEncodeBatch(images): width must be an unsigned integer');
typeError(() => z.pngEncodeBatch([Object.assign({}, images[0], { height: 1.5 })]), 'pngEncodeBatch(images): height must be an unsigned integer');
typeError(() => z.pngEncodeBatch([Object.assign({}, images[0], { palette: 'abc' })]), 'pngEncodeBatch(images): palette and transparency must be Uint8Array of at most 65535 bytes');
typeError(() => z.pngEncodeBatch([Object.assign({}, images[0], { data: 'abc' })]), 'pngEncodeBatch(rows, records, aux): every element of rows must be a Uint8Array');
typeError(() => z.pngEncode('png'), 'pngEncodeBatch(images): every image must be an object');
assert.deepStrictEqual(z.pngEncodeBatch([]), []);
console.log('pngwrite node checks passed');
