// bgzip() and bgzipIndex() of the N-API façade: the bytes, the member positions, and that Node's own zlib reads the file.
// The fixture comes from the Python side: ZES_BGZIP_DIR holds in.bin, want.gz and offsets.txt.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const nodeZlib = require('zlib');
const z = require(path.join(__dirname, '..', 'zlib.es_amd', 'host', 'zlib.js'));

const dir = process.env.ZES_BGZIP_DIR;
assert.ok(dir, 'ZES_BGZIP_DIR is not set');
const input = new Uint8Array(fs.readFileSync(path.join(dir, 'in.bin')));
const want = fs.readFileSync(path.join(dir, 'want.gz'));
const offsets = fs.readFileSync(path.join(dir, 'offsets.txt'), 'utf8').trim().split(/\s+/).map(Number);
const got = z.bgzip(input);
assert.ok(got instanceof Uint8Array);
assert.ok(Buffer.from(got).equals(want), 'bgzip(in) differs from the expected file');
const indexed = z.bgzipIndex(input);
assert.ok(Buffer.from(indexed.data).equals(want), 'bgzipIndex(in).data differs from the expected file');
assert.deepStrictEqual(indexed.offsets, offsets);
assert.ok(nodeZlib.gunzipSync(Buffer.from(got)).equals(Buffer.from(input)), "Node's gunzipSync does not return the input");
// the empty input: the end-of-file marker alone
const empty = z.bgzipIndex(new Uint8Array(0));
assert.strictEqual(empty.data.length, 28);
assert.deepStrictEqual(empty.offsets, [0]);
assert.throws(() => z.bgzip('text'), TypeError);
console.log('bgzip node checks passed');
