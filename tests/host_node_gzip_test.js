// gzip() / gunzip() of the N-API façade (zlib.es_amd/host/zlib.js) against Node's own zlib: round trips, Node's
// gzipSync output read back, several members, and the errors rethrown with the library's messages.
'use strict';
const assert = require('assert');
const path = require('path');
const nodeZlib = require('zlib');
const z = require(path.join(__dirname, '..', 'zlib.es_amd', 'host', 'zlib.js'));

function text(n, seed) {
  const a = new Uint8Array(n);
  let s = seed >>> 0;
  const words = ['alpha ', 'beta ', 'gamma ', 'delta\n', 'epsilon ', 'zeta, '];
  let i = 0;
  while (i < n) {
    s = (s * 1103515245 + 12345) >>> 0;
    const w = words[(s >>> 16) % words.length];
    for (let k = 0; k < w.length && i < n; k++) a[i++] = w.charCodeAt(k);
  }
  return a;
}

for (const n of [2, 1000, 131072 * 2 + 7, (4 << 20) + 3]) {
  const a = text(n, n);
  const g = z.gzip(a);
  assert.deepStrictEqual(Array.from(g.subarray(0, 10)), [0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff]);
  assert.ok(Buffer.from(nodeZlib.gunzipSync(g)).equals(Buffer.from(a)), 'node reads gzip() ' + n);
  assert.ok(Buffer.from(z.gunzip(g)).equals(Buffer.from(a)), 'round trip ' + n);
  for (const level of [1, 6, 9]) {
    const ng = nodeZlib.gzipSync(a, { level });
    assert.ok(Buffer.from(z.gunzip(new Uint8Array(ng))).equals(Buffer.from(a)), 'gunzip of node level ' + level + ' ' + n);
  }
}
const m1 = text(5000, 1), m2 = text(70000, 2);
const two = Buffer.concat([nodeZlib.gzipSync(m1), Buffer.alloc(3), nodeZlib.gzipSync(m2)]);
assert.ok(Buffer.from(z.gunzip(new Uint8Array(two))).equals(Buffer.concat([Buffer.from(m1), Buffer.from(m2)])), 'two members');
const bad = new Uint8Array(nodeZlib.gzipSync(m1));
bad[bad.length - 8] ^= 1;
assert.throws(() => z.gunzip(bad), /checksum/);
assert.throws(() => z.gunzip(new Uint8Array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11])), /gzip/);
assert.throws(() => z.gzip(new Uint8Array(1)), { message: 'Data is corrupted' });
console.log('gzip node checks passed');
