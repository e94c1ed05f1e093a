'use strict';
// GENERATED from zlib.ts by strip_types.py — do not edit.
/**
 * zlib.ts — drop-in for zlib.es's public module (reference src/zlib.ts:11,25; types as in
 * dist/tsc/zlib.d.ts:4-5): the same two synchronous functions, the same thrown `Error`
 * messages, results bit-identical to the reference — computed on an AMD MI355X through the
 * N-API addon (zes_napi.cc -> include/zes.h -> HIP kernels).
 *
 * There is no JavaScript fallback: without the addon or a GPU the call throws.
 *
 * zlib.js next to this file is generated from it by strip_types.py (this image has no tsc);
 * keep to erasable syntax: annotations on parameters / return types only.
 *
 * Every Uint8Array a function here returns, allocPinned()'s included, must not be transferred or detached (postMessage
 * with a transfer list): its memory goes back to the addon's pool once the original ArrayBuffer object is collected, and
 * a transfer leaves that object without it while the receiver still uses the bytes.  Pass a copy instead.
 */
const addon = require('./build/zes_napi.node');

/**
 * Extra (not in the reference API): `verify: true` makes an inflate form check the stream's Adler-32 trailer against its
 * result; a trailer that is missing or does not match is the Error "zes: checksum mismatch".  The reference ignores the
 * trailer (src/zlib.ts:11-23), and so does every call without the option.  (A rest parameter below, not
 * `options?`: inflate.length stays 1, as the reference's; zlib.d.ts declares one optional argument.)
 */

function inflate(input, ...options) {
  return addon.inflate(input, options[0]);
}

function deflate(input) {
  return addon.deflate(input);
}

/**
 * The raw forms the wrapper above encloses, for callers that keep DEFLATE inside another container:
 * `deflateRaw` is the reference's internal `deflate(input)` (src/deflate.ts:14), `inflateRaw` its
 * `inflate(input, offset = 0)` (src/inflate.ts:16) — not exported by the reference's package entry.
 */
function deflateRaw(input) {
  return addon.deflateRaw(input);
}

function inflateRaw(input, offset) {
  return addon.inflateRaw(input, offset);
}

/**
 * Promise-returning forms (not in the reference API, SURVEY §8f.4): the same work on a libuv worker thread, so the
 * JS thread stays free while the GPU runs.  Resolve with the same bytes, reject with the same `Error` messages.
 * The input array must not be modified, and its ArrayBuffer must not be transferred or detached, until the promise settles.
 */
function deflateAsync(input) {
  return addon.deflateAsync(input);
}

function inflateAsync(input, ...options) {
  return addon.inflateAsync(input, options[0]);
}

/**
 * Batch forms (not in the reference API; SURVEY §7 step 3): an array of independent buffers in one call — what a
 * caller's loop over deflate()/inflate() (reference README.md:28-42) becomes when small buffers should share the GPU.
 * Element i of the result is the Uint8Array deflate(inputs[i]) / inflate(inputs[i]) would return, or — instead of a
 * throw — the `Error` it would have thrown (same message).  The Async forms run on a libuv worker thread.  With
 * `{ verify: true }` the inflate forms check every stream's Adler-32 trailer in one launch over all results; a buffer
 * that fails is the Error "zes: checksum mismatch" in its element.
 */
function deflateBatch(inputs) {
  return addon.deflateBatch(inputs);
}

function inflateBatch(inputs, ...options) {
  return addon.inflateBatch(inputs, options[0]);
}

function deflateBatchAsync(inputs) {
  return addon.deflateBatchAsync(inputs);
}

function inflateBatchAsync(inputs, ...options) {
  return addon.inflateBatchAsync(inputs, options[0]);
}

/**
 * Extra: a Uint8Array of n bytes in page-locked memory.  Inputs that live in such an array cross PCIe without the
 * library's staging copy (any Uint8Array is accepted everywhere; this is only faster).
 */
function allocPinned(n) {
  return addon.allocPinned(n);
}

/**
 * Extra (not in the reference API): gzip files (RFC 1952).  `gzip` writes one member with a fixed 10-byte header
 * (no name, MTIME 0) around deflateRaw(input); `gunzip` reads every member of a gzip file (CPython's
 * gzip.decompress) and checks every CRC-32 and size.  Errors are thrown with the library's messages.
 */
function gzip(input) {
  return addon.gzip(input);
}

function gunzip(input) {
  return addon.gunzip(input);
}

/**
 * Extra (not in the reference API): many independent gzip files in one call.  `gzipBatch` writes every input as one gzip file
 * (gzip()'s bytes, or stored blocks where those are shorter or the encoder refuses the length: every length writes) and
 * `gunzipBatch` decodes every file as gunzip() would alone; the device work does not grow with the number of items.  Element
 * i of the result is the file (the output) or — the call does not throw — the `Error` that says why not.
 */
function gzipBatch(inputs) {
  return addon.gzipBatch(inputs);
}

function gunzipBatch(files) {
  return addon.gunzipBatch(files);
}

/**
 * Extra (not in the reference API): BGZF files, the blocked gzip of bgzip / htslib.  `bgzip` writes one gzip member per
 * 65280-byte chunk of the input, each stating its own size, and the 28-byte end-of-file marker: a file htslib can index
 * and gunzip() decodes as one batch.  Every input length is valid.  `bgzipIndex` also returns the byte position of every
 * member in the result, the marker's last (member k holds input bytes from k * 65280): what virtual offsets are made of.
 */
function bgzip(input) {
  return addon.bgzip(input);
}

function bgzipIndex(input) {
  return addon.bgzipIndex(input);
}

/**
 * Extra: random access into a BGZF file.  `bgzfIndex` walks the file's members on the host (no device is touched) and
 * returns their byte positions (`compressed`) and the positions of their outputs in the uncompressed data
 * (`uncompressed`), members + 1 entries each, the last one the file's length and the uncompressed size.  `bgzfRead` returns
 * bytes [pos, pos + len) of the uncompressed data, clipped at its end: only the members that hold the range are uploaded
 * and decoded.  Virtual offsets and .gzi files are not handled.
 */
function bgzfIndex(file) {
  return addon.bgzfIndex(file);
}

function bgzfRead(file, index, pos, len) {
  return addon.bgzfRead(file, index, pos, len);
}

/**
 * Extra (not in the reference API): ZIP archives, reading.  `zipIndex` lists the archive's entries from its central
 * directory on the host (no device is touched, nothing is decoded): per entry the name as the archive holds it (`nameBytes`)
 * and as a string (`name`: UTF-8 when flag bit 11 says so, else byte for byte as code points — CP437 is not decoded), the
 * method, the flags, both sizes and the CRC-32; `raw` is the same list as the records the library reads (40 bytes an entry)
 * and is all that `zipRead` looks at.  `zipRead` extracts the entries `sel` names by number (all of them without it; any
 * order, duplicates fine) as one batch: only their bytes are uploaded, every DEFLATE body goes through the inflate tiers in
 * one call, and one launch checks every CRC-32.  Element i of the result is the entry's bytes or — instead of a throw — the
 * `Error` that says why not (a checksum mismatch, a local header that does not fit the directory, encryption, a method other
 * than stored and DEFLATE).  ZIP64 archives and archives over several disks are refused by `zipIndex`.  (A rest parameter,
 * not `sel?`: zlib.d.ts declares one optional argument.)
 */
function zipIndex(file) {
  const got = addon.zipIndex(file);
  const view = new DataView(got.raw.buffer, got.raw.byteOffset, got.raw.byteLength);
  const entries = [];
  for (let at = 0; at < got.raw.length; at += 40) {
    const nameOff = view.getUint32(at + 28, true), flags = view.getUint16(at + 36, true);
    const nameBytes = got.names.slice(nameOff, nameOff + view.getUint16(at + 32, true));
    entries.push({
      nameBytes, name: Buffer.from(nameBytes.buffer, nameBytes.byteOffset, nameBytes.length).toString(flags & 0x800 ? 'utf8' : 'latin1'),
      method: view.getUint16(at + 34, true), flags, compressedSize: view.getUint32(at + 16, true), size: view.getUint32(at + 20, true),
      crc32: view.getUint32(at + 24, true),
    });
  }
  return { entries, raw: got.raw };
}

function zipRead(file, index, ...sel) {
  return addon.zipRead(file, index, sel[0]);
}

/**
 * Extra (not in the reference API): `zip` writes a ZIP archive of `files` in one call: every entry is checksummed and encoded
 * on the device as one batch, deflated where that is shorter than the data and stored otherwise.  A `name` given as a string is
 * encoded as UTF-8 (a name with a byte >= 0x80 sets flag bit 11); a Uint8Array is taken as it is.  The same files give the
 * same bytes (date 1980-01-01); zipIndex() / zipRead() and any unzip read the result.  No ZIP64: at most 65534 entries, and
 * sizes and offsets below 4 GiB, else the library's "unsupported ZIP feature" Error.
 */
function zip(files) {
  if (!Array.isArray(files)) throw new TypeError('zip(files): files must be an array of { name, data }');
  const names = files.map((f) => (f && typeof f.name === 'string' ? new TextEncoder().encode(f.name) : f && f.name));
  return addon.zip(names, files.map((f) => f && f.data));
}

/**
 * Extra (not in the reference API): PNG images, reading.  `pngInfo` judges a file on the host (no device is touched, no CRC
 * is checked) and returns what its header says: size, bit depth, colour type, interlace method, the filter unit `bpp`,
 * `rowBytes`, the decoded `size` (height * rowBytes), and where the IDAT, PLTE and tRNS data lie.  `pngDecodeBatch` decodes
 * files as one batch on the device: one launch checks every chunk's CRC-32, every IDAT stream goes through the inflate tiers
 * in one call, and one launch undoes the scanline filters.  Element i of the result is `{ info, data }` or — instead of a
 * throw — the `Error` that says why not.  `data` holds the scanlines as the file stores them: 16-bit samples big-endian,
 * samples below 8 bits packed, palette indices as indices.  Interlaced (Adam7) files are listed by `pngInfo` and refused by
 * the decoders without `{ interlaced: true }` as the second argument (ZES_F_PNG_INTERLACED); with it they decode to the
 * scanlines of a non-interlaced file of the same pixels.  `pngDecode` is the batch of one file and throws its Error.
 * (The option is written `...options` and read as `options[0]`, as `inflate` writes its own: strip_types.py erases a
 * rest parameter's type but not the `?` of an optional one, and `.length` stays 1.  zlib.d.ts declares one optional
 * argument, `options?: PngOptions`; arguments behind it are not looked at.)
 */
const pngInfoAt = (raw, at) => {  // one zes_png_info record (72 bytes, include/zes.h)
  const v = new DataView(raw.buffer, raw.byteOffset + at, 72);
  const big = (o) => Number(v.getBigUint64(o, true));
  return {
    width: v.getUint32(0, true), height: v.getUint32(4, true), depth: v.getUint8(8), colourType: v.getUint8(9), interlace: v.getUint8(10),
    channels: v.getUint8(11), bpp: v.getUint8(12), rowBytes: big(16), size: big(24), idatCount: v.getUint32(32, true), idatBytes: big(40),
    paletteOffset: big(48), paletteLength: v.getUint32(36, true), transparencyOffset: big(56), transparencyLength: v.getUint32(64, true),
  };
};

function pngInfo(file) {
  return pngInfoAt(addon.pngInfo(file), 0);
}

function pngDecodeBatch(files, ...options) {
  const got = addon.pngDecodeBatch(files, options[0]);
  return got.results.map((r, i) => (r instanceof Error ? r : { info: pngInfoAt(got.info, 72 * i), data: r }));
}

function pngDecode(file, ...options) {
  const got = pngDecodeBatch([file], options[0])[0];
  if (got instanceof Error) throw got;
  return got;
}

/**
 * Extra (not in the reference API): PNG images as pixels.  `pngPixelsBatch` decodes files as `pngDecodeBatch` does and goes
 * one step further on the device: one more launch turns every image's scanlines into `width * height * 4` bytes of R, G, B,
 * A, row by row from the top — samples below 8 bits scaled to 0..255, 16-bit samples cut to their high byte, grey
 * replicated, palette indices looked up (an index beyond the palette is opaque black), tRNS applied as alpha (a tRNS whose
 * length does not fit the colour type is ignored).  Element i of the result is `{ info, data }` — `info` as `pngInfo` gives
 * it, `data` the pixels — or the `Error` that says why not.  No gamma, no colour management; interlaced files are refused
 * without `{ interlaced: true }` as the second argument (ZES_F_PNG_INTERLACED), as `pngDecodeBatch` refuses them.
 * `pngPixels` is the batch of one file and throws its Error.
 */
function pngPixelsBatch(files, ...options) {
  const got = addon.pngPixelsBatch(files, options[0]);
  return got.results.map((r, i) => (r instanceof Error ? r : { info: pngInfoAt(got.info, 72 * i), data: r }));
}

function pngPixels(file, ...options) {
  const got = pngPixelsBatch([file], options[0])[0];
  if (got instanceof Error) throw got;
  return got;
}

/**
 * Extra (not in the reference API): PNG images, writing.  `pngEncodeBatch` writes images as PNG files in one batch on the
 * device: one launch chooses and applies the scanline filters of every row of every image, one batch encode makes the zlib
 * streams, one launch lays the files out and two more make the chunk CRCs.  An image is `{ data, width, height, colourType,
 * depth = 8, filter = 5, palette, transparency }`: `data` the scanlines as `pngDecode` gives them (height * rowBytes bytes),
 * `filter` 0..4 that type on every row, 6 libpng's adaptive choice, 5 the same with rows 0, 64, 128, ... None or Sub, which
 * lets `pngDecode` work on the file's bands of 64 rows in parallel.  Element i of the result is the file or — instead of a
 * throw — the `Error` that says why not.  The same images give the same bytes.  `pngEncode` is the batch of one image and
 * throws its Error.
 */
function pngEncodeBatch(images) {
  if (!Array.isArray(images)) throw new TypeError('pngEncodeBatch(images): images must be an array of { data, width, height, colourType }');
  const none = new Uint8Array(0);
  const recs = new Uint8Array(16 * images.length);
  const view = new DataView(recs.buffer);
  const parts = [];
  images.forEach((im, i) => {
    if (!im || typeof im !== 'object') throw new TypeError('pngEncodeBatch(images): every image must be an object');
    const plte = im.palette || none, trns = im.transparency || none;
    if (!(plte instanceof Uint8Array) || !(trns instanceof Uint8Array) || plte.length > 65535 || trns.length > 65535)
      throw new TypeError('pngEncodeBatch(images): palette and transparency must be Uint8Array of at most 65535 bytes');
    for (const k of ['width', 'height', 'colourType'])
      if (!Number.isInteger(im[k]) || im[k] < 0 || im[k] > 0xFFFFFFFF) throw new TypeError('pngEncodeBatch(images): ' + k + ' must be an unsigned integer');
    view.setUint32(16 * i, im.width, true);
    view.setUint32(16 * i + 4, im.height, true);
    view.setUint8(16 * i + 8, im.depth === undefined ? 8 : im.depth);
    view.setUint8(16 * i + 9, im.colourType);
    view.setUint8(16 * i + 10, im.filter === undefined ? 5 : im.filter);
    view.setUint16(16 * i + 12, plte.length, true);
    view.setUint16(16 * i + 14, trns.length, true);
    parts.push(plte, trns);
  });
  const aux = new Uint8Array(parts.reduce((n, p) => n + p.length, 0));
  parts.reduce((at, p) => (aux.set(p, at), at + p.length), 0);
  return addon.pngEncodeBatch(images.map((im) => im.data), recs, aux);
}

function pngEncode(image) {
  const got = pngEncodeBatch([image])[0];
  if (got instanceof Error) throw got;
  return got;
}

/**
 * Extra (not in the reference API): TIFF images, reading.  `tiffInfo` judges directory `dir` (default 0) of a file on the host
 * (no device is touched) and returns its geometry: size, the tiles' or strips' size (`segmentWidth`, `segmentHeight`) and
 * count (`across`, `down`), `bits` (8, 16 or 32) and `samples` (1..4) a pixel, the Compression, Predictor, Photometric,
 * SampleFormat and ExtraSamples tags as the file states them, the decoded `size` and `dirs`, the length of the file's directory
 * chain.  `tiffRead` decodes a rectangle `{ x, y, w, h }` of that image (default: the whole image) on the device: only the
 * tiles or strips under the rectangle are uploaded, they go through the inflate tiers as one batch, and one launch undoes
 * Predictor 2, drops tile padding and puts the rows in place.  `data` holds `height` rows of `width * samples * bits / 8`
 * bytes, samples of 16 and 32 bits little-endian whatever the file's byte order.  Uncompressed and zlib-compressed
 * (Compression 8, 32946) files are read; anything else, and a tile or strip that fails, throws the Error that says why.
 * (`...dir` and `...options` are read as `dir[0]` and `options[0]`, as `pngDecode` reads its own.)
 */
const tiffInfoOf = (raw) => {  // a zes_tiff_image record (48 bytes, include/zes.h) and the chain's length
  const v = new DataView(raw.buffer, raw.byteOffset, 52);
  const u32 = (o) => v.getUint32(o, true), u16 = (o) => v.getUint16(o, true);
  return {
    width: u32(0), height: u32(4), segmentWidth: u32(8), segmentHeight: u32(12), across: u32(16), down: u32(20), bits: u16(24), samples: u16(26),
    compression: u16(28), predictor: u16(30), photometric: u16(32), sampleFormat: u16(34), extraSamples: u16(36), bigEndian: v.getUint8(38) !== 0,
    tiled: v.getUint8(39) !== 0, size: Number(v.getBigUint64(40, true)), dirs: u32(48),
  };
};

function tiffInfo(file, ...dir) {
  return tiffInfoOf(addon.tiffInfo(file, dir[0]));
}

function tiffRead(file, ...options) {
  const o = options[0];
  if (o !== undefined && (o === null || typeof o !== 'object' || Array.isArray(o))) throw new TypeError('tiffRead(file, options): options must be an object { dir?, rect? }');
  let rect;
  if (o && o.rect !== undefined) {
    const r = o.rect;
    if (!r || typeof r !== 'object' || ![r.x, r.y, r.w, r.h].every((k) => Number.isInteger(k) && k >= 0 && k <= 0xFFFFFFFF))
      throw new TypeError('tiffRead(file, options): rect must be { x, y, w, h } of unsigned integers');
    rect = Uint32Array.of(r.x, r.y, r.w, r.h);
  }
  const got = addon.tiffRead(file, o ? o.dir : undefined, rect);
  const info = tiffInfoOf(got.info);
  return { width: rect ? rect[2] : info.width, height: rect ? rect[3] : info.height, samples: info.samples, bits: info.bits, data: got.results[0] };
}

/**
 * Extra (not in the reference API): TIFF images, writing.  `tiffWrite` writes one image to one classic TIFF file with one
 * directory: `pixels` is what `tiffRead` gives for the whole image (`height` rows of `width * samples * bits / 8` bytes, samples
 * little-endian whatever `bigEndian` says) and `info` what `tiffInfo` gives (`dirs` is ignored; `across`, `down` and `size` are
 * computed when they are absent), so that info -> read -> write round-trips.  The tiles or strips are cut, differenced under
 * Predictor 2 and encoded as one batch on the device; a record the writer refuses throws the Error that says why.
 */
function tiffWrite(pixels, info) {
  if (info === null || typeof info !== 'object' || Array.isArray(info)) throw new TypeError('tiffWrite(pixels, info): info must be an object as tiffInfo gives it');
  const n = (k, dflt) => {
    const x = info[k] === undefined ? dflt : info[k];
    if (!Number.isInteger(x) || x < 0) throw new TypeError('tiffWrite(pixels, info): info.' + k + ' must be a non-negative integer');
    return x;
  };
  const raw = new Uint8Array(48);
  const v = new DataView(raw.buffer);
  const width = n('width'), height = n('height'), sw = n('segmentWidth'), sh = n('segmentHeight'), bits = n('bits'), samples = n('samples');
  const put32 = (o, x) => v.setUint32(o, x > 0xFFFFFFFF ? 0xFFFFFFFF : x, true), put16 = (o, x) => v.setUint16(o, x > 0xFFFF ? 0xFFFF : x, true);
  put32(0, width); put32(4, height); put32(8, sw); put32(12, sh);
  put32(16, n('across', sw ? Math.ceil(width / sw) : 0)); put32(20, n('down', sh ? Math.ceil(height / sh) : 0));
  put16(24, bits); put16(26, samples); put16(28, n('compression', 8)); put16(30, n('predictor', 1)); put16(32, n('photometric', samples >= 3 ? 2 : 1));
  put16(34, n('sampleFormat', 1)); put16(36, n('extraSamples', 0));
  v.setUint8(38, info.bigEndian ? 1 : 0); v.setUint8(39, info.tiled ? 1 : 0);
  v.setBigUint64(40, BigInt(n('size', width * height * samples * Math.floor(bits / 8))), true);
  return addon.tiffWrite(pixels, raw)[0];
}

/**
 * Extra: how many members the last gunzip() of this thread decoded as one batch (a BGZF file: all of them, the
 * end-of-file marker included); 0 when the members went one after the other.
 */
function lastGunzipMembers() {
  return addon.lastGunzipMembers();
}

/** Extra (not in the reference API): Adler-32 of a buffer, computed on the GPU. */
function adler32(input) {
  return addon.adler32(input);
}

/** Extra: bind this process to a GPU (defaults to device 0 on first use). */
function init(device) {
  addon.init(device);
}

/**
 * Extra: drive `n` GPUs from this one process (n omitted or <= 0: every visible one; returns the number in use).  After
 * this the batch forms partition their buffers over all of them by size — a caller's loop over deflate()/inflate()
 * (reference README.md:28-42) spread over the node — and single calls (deflateAsync from several promises at once) take
 * the GPUs in turn.  Results are the same bytes, buffer for buffer.
 */
function initDevices(n) {
  return addon.initDevices(n);
}

/** Extra: give the library's pooled GPU scratch back to the driver (a long-lived process after one large call). */
function trim() {
  addon.trim();
}

exports.inflate = inflate;
exports.deflate = deflate;
exports.deflateRaw = deflateRaw;
exports.inflateRaw = inflateRaw;
exports.deflateAsync = deflateAsync;
exports.inflateAsync = inflateAsync;
exports.deflateBatch = deflateBatch;
exports.inflateBatch = inflateBatch;
exports.deflateBatchAsync = deflateBatchAsync;
exports.inflateBatchAsync = inflateBatchAsync;
exports.allocPinned = allocPinned;
exports.gzip = gzip;
exports.gunzip = gunzip;
exports.gzipBatch = gzipBatch;
exports.gunzipBatch = gunzipBatch;
exports.bgzip = bgzip;
exports.bgzipIndex = bgzipIndex;
exports.bgzfIndex = bgzfIndex;
exports.bgzfRead = bgzfRead;
exports.zipIndex = zipIndex;
exports.zipRead = zipRead;
exports.zip = zip;
exports.pngInfo = pngInfo;
exports.pngDecodeBatch = pngDecodeBatch;
exports.pngDecode = pngDecode;
exports.pngPixelsBatch = pngPixelsBatch;
exports.pngPixels = pngPixels;
exports.pngEncodeBatch = pngEncodeBatch;
exports.pngEncode = pngEncode;
exports.tiffInfo = tiffInfo;
exports.tiffRead = tiffRead;
exports.tiffWrite = tiffWrite;
exports.lastGunzipMembers = lastGunzipMembers;
exports.adler32 = adler32;
exports.init = init;
exports.initDevices = initDevices;
exports.trim = trim;
