// gunzip() of the N-API façade on a BGZF file: the bytes, and that the members went as one batch (lastGunzipMembers()).
// The fixture comes from the Python side: ZES_BGZF_DIR holds bgzf.gz, plain.gz, want.bin and members.txt.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const z = require(path.join(__dirname, '..', 'zlib.es_amd', 'host', 'zlib.js'));

const dir = process.env.ZES_BGZF_DIR;
assert.ok(dir, 'ZES_BGZF_DIR is not set');
const want = fs.readFileSync(path.join(dir, 'want.bin'));
const members = parseInt(fs.readFileSync(path.join(dir, 'members.txt'), 'utf8'), 10);
const got = z.gunzip(new Uint8Array(fs.readFileSync(path.join(dir, 'bgzf.gz'))));
assert.ok(Buffer.from(got).equals(want), 'gunzip(bgzf) differs from the expected bytes');
assert.strictEqual(z.lastGunzipMembers(), members);
// an ordinary gzip file of the same bytes goes member by member
const plain = z.gunzip(new Uint8Array(fs.readFileSync(path.join(dir, 'plain.gz'))));
assert.ok(Buffer.from(plain).equals(want), 'gunzip(plain) differs from the expected bytes');
assert.strictEqual(z.lastGunzipMembers(), 0);
console.log('bgzf node checks passed');
