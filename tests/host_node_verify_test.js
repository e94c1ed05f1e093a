// The { verify: true } option of inflate, inflateAsync, inflateBatch and inflateBatchAsync: the stream's Adler-32 trailer
// is checked against the result.  The fixture comes from the Python side: ZES_VERIFY_DIR holds good.z, bad.z (the same
// stream with one trailer bit flipped) and raw.bin.
'use strict';
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const z = require(path.join(__dirname, '..', 'zlib.es_amd', 'host', 'zlib.js'));

const dir = process.env.ZES_VERIFY_DIR;
assert.ok(dir, 'ZES_VERIFY_DIR is not set');
const read = (name) => new Uint8Array(fs.readFileSync(path.join(dir, name)));
const good = read('good.z'), bad = read('bad.z'), raw = Buffer.from(read('raw.bin'));
const same = (got) => got instanceof Uint8Array && Buffer.from(got).equals(raw);
const mismatch = (e) => e instanceof Error && e.message === 'zes: checksum mismatch';  // (a RegExp would be matched against String(e))
const off = [undefined, {}, { verify: false }, null];

(async () => {
  // inflate
  assert.ok(same(z.inflate(good)) && same(z.inflate(good, { verify: true })));
  assert.ok(same(z.inflate(bad)));
  off.forEach((o) => assert.ok(same(z.inflate(bad, o))));
  assert.throws(() => z.inflate(bad, { verify: true }), mismatch);
  assert.throws(() => z.inflate(good.subarray(0, good.length - 1), { verify: true }), mismatch);
  // inflateAsync
  assert.ok(same(await z.inflateAsync(good)) && same(await z.inflateAsync(good, { verify: true })));
  assert.ok(same(await z.inflateAsync(bad)) && same(await z.inflateAsync(bad, { verify: false })));
  await assert.rejects(z.inflateAsync(bad, { verify: true }), mismatch);
  // inflateBatch
  const list = [good, bad, good];
  z.inflateBatch(list).forEach((r) => assert.ok(same(r)));
  off.forEach((o) => z.inflateBatch(list, o).forEach((r) => assert.ok(same(r))));
  let res = z.inflateBatch(list, { verify: true });
  assert.ok(same(res[0]) && same(res[2]));
  assert.ok(mismatch(res[1]));
  // inflateBatchAsync
  (await z.inflateBatchAsync(list)).forEach((r) => assert.ok(same(r)));
  res = await z.inflateBatchAsync(list, { verify: true });
  assert.ok(same(res[0]) && same(res[2]));
  assert.ok(mismatch(res[1]));
  // the option does not reach the deflate forms, and a body's own error comes first
  assert.ok(same(z.inflate(z.deflate(raw), { verify: true })));
  const broken = Uint8Array.from(good);
  broken[0] = 0x77;
  assert.throws(() => z.inflate(broken, { verify: true }), /Not compressed by deflate/);
  console.log('verify node checks passed');
})().catch((e) => {
  console.error(e);
  process.exit(1);
});
