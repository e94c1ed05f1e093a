// bgzfIndex() and bgzfRead() of the N-API façade: the member index of a BGZF file and range reads through it.
// The fixture comes from the Python side: ZES_BGZF_READ_DIR holds file.gz, compressed.txt, uncompressed.txt, ranges.txt
// (one "pos len" per line) and slice0.bin, slice1.bin, slice2.bin.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const z = require(path.join(__dirname, '..', 'zlib.es_amd', 'host', 'zlib.js'));

const dir = process.env.ZES_BGZF_READ_DIR;
assert.ok(dir, 'ZES_BGZF_READ_DIR is not set');
const file = new Uint8Array(fs.readFileSync(path.join(dir, 'file.gz')));
const list = (name) => fs.readFileSync(path.join(dir, name), 'utf8').trim().split(/\s+/).map((s) => BigInt(s));
const index = z.bgzfIndex(file);
assert.ok(index.compressed instanceof BigUint64Array && index.uncompressed instanceof BigUint64Array);
assert.deepStrictEqual(Array.from(index.compressed), list('compressed.txt'));
assert.deepStrictEqual(Array.from(index.uncompressed), list('uncompressed.txt'));
const ranges = fs.readFileSync(path.join(dir, 'ranges.txt'), 'utf8').trim().split('\n').map((l) => l.trim().split(/\s+/).map(Number));
assert.strictEqual(ranges.length, 3);
ranges.forEach(([pos, len], k) => {
  const want = fs.readFileSync(path.join(dir, 'slice' + k + '.bin'));
  const got = z.bgzfRead(file, index, pos, len);
  assert.ok(got instanceof Uint8Array);
  assert.ok(Buffer.from(got).equals(want), 'bgzfRead(file, index, ' + pos + ', ' + len + ') differs from the expected slice');
  // the same with bigints, one of each
  assert.ok(Buffer.from(z.bgzfRead(file, index, BigInt(pos), len)).equals(want));
  assert.ok(Buffer.from(z.bgzfRead(file, index, pos, BigInt(len))).equals(want));
});
assert.ok(z.lastGunzipMembers() >= 1);
const total = Number(index.uncompressed[index.uncompressed.length - 1]);
assert.strictEqual(z.bgzfRead(file, index, total, 10).length, 0);
assert.throws(() => z.bgzfRead(file, index, total + 1, 1), /bad argument/);
assert.throws(() => z.bgzfRead(file, index, -1, 1), TypeError);
assert.throws(() => z.bgzfRead(file, { compressed: [0], uncompressed: [0] }, 0, 1), TypeError);
assert.throws(() => z.bgzfIndex(file.subarray(0, file.length - 3)), /gzip/);
assert.throws(() => z.bgzfIndex('text'), TypeError);
console.log('bgzf read node checks passed');
