// zip() of the N-API façade where it needs no device: the archive of no files, and the TypeErrors of the marshalling.
'use strict';
const assert = require('assert');
const path = require('path');
const z = require(path.join(__dirname, '..', 'zlib.es_amd', 'host', 'zlib.js'));
const esm = require('fs').readFileSync(path.join(__dirname, '..', 'zlib.es_amd', 'host', 'zlib.mjs'), 'utf8');

assert.strictEqual(typeof z.zip, 'function');
assert.strictEqual(z.zip.length, 1);
assert.ok(esm.includes('export const zip = z.zip;'));
const end = z.zip([]);
assert.ok(end instanceof Uint8Array && Buffer.from(end).equals(Buffer.concat([Buffer.from('PK\x05\x06', 'latin1'), Buffer.alloc(18)])));
assert.strictEqual(z.zipIndex(end).entries.length, 0);
const data = new Uint8Array(8);
const bad = [undefined, null, 'files', {}, [null], [{}], [{ name: 'a' }], [{ data }], [{ name: 1, data }], [{ name: 'a', data: 'text' }], [{ name: 'a', data: [1, 2] }],
             [{ name: 'n'.repeat(65536), data }], [{ name: new Uint8Array(65536), data }], [{ name: 'ok', data }, { name: 'a' }]];
for (const files of bad) assert.throws(() => z.zip(files), TypeError, JSON.stringify(files === undefined ? 'undefined' : files).slice(0, 60));
console.log('zip write argument checks passed');
