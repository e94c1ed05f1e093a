/** Same declarations as the reference's dist/tsc/zlib.d.ts:4-5, plus the raw, Promise and batch forms and the extras. */
/** No returned Uint8Array (allocPinned()'s included) may be transferred or detached: its memory is reused once the original ArrayBuffer object is collected. */
/** `verify: true`: the stream's Adler-32 trailer must be there and match the result, else the Error "zes: checksum mismatch". */
export declare type InflateOptions = { verify?: boolean };
export declare function inflate(input: Uint8Array, options?: InflateOptions): Uint8Array;
export declare function deflate(input: Uint8Array): Uint8Array;
export declare function deflateRaw(input: Uint8Array): Uint8Array;
export declare function inflateRaw(input: Uint8Array, offset?: number): Uint8Array;
export declare function deflateAsync(input: Uint8Array): Promise<Uint8Array>;
export declare function inflateAsync(input: Uint8Array, options?: InflateOptions): Promise<Uint8Array>;
export declare type BatchResult = Uint8Array | Error;
export declare function deflateBatch(inputs: Uint8Array[]): BatchResult[];
export declare function inflateBatch(inputs: Uint8Array[], options?: InflateOptions): BatchResult[];
export declare function deflateBatchAsync(inputs: Uint8Array[]): Promise<BatchResult[]>;
export declare function inflateBatchAsync(inputs: Uint8Array[], options?: InflateOptions): Promise<BatchResult[]>;
export declare function allocPinned(n: number): Uint8Array;
export declare function adler32(input: Uint8Array): number;
export declare function gzip(input: Uint8Array): Uint8Array;
export declare function gunzip(input: Uint8Array): Uint8Array;
/** Many independent gzip files in one batch: per item the file (the output) or the Error that says why not; every input length writes. */
export declare function gzipBatch(inputs: Uint8Array[]): BatchResult[];
export declare function gunzipBatch(files: Uint8Array[]): BatchResult[];
export declare function lastGunzipMembers(): number;
export declare function bgzip(input: Uint8Array): Uint8Array;
export declare function bgzipIndex(input: Uint8Array): { data: Uint8Array, offsets: number[] };
export declare function bgzfIndex(file: Uint8Array): { compressed: BigUint64Array, uncompressed: BigUint64Array };
export declare function bgzfRead(file: Uint8Array, index: { compressed: BigUint64Array, uncompressed: BigUint64Array }, pos: number | bigint, len: number | bigint): Uint8Array;
/** ZIP archives, read only: the entries out of the central directory (no device is touched), and batch extraction through that index. */
export declare type ZipEntry = { nameBytes: Uint8Array, name: string, method: number, flags: number, compressedSize: number, size: number, crc32: number };
export declare type ZipIndex = { entries: ZipEntry[], raw: Uint8Array };
export declare function zipIndex(file: Uint8Array): ZipIndex;
export declare function zipRead(file: Uint8Array, index: ZipIndex, sel?: number[] | Uint32Array): BatchResult[];
export declare function zip(files: { name: string | Uint8Array, data: Uint8Array }[]): Uint8Array;
/** PNG images, reading: the header's facts (no device is touched), and batch decoding to scanlines (samples as stored, filters undone). */
export declare type PngInfo = {
  width: number, height: number, depth: number, colourType: number, interlace: number, channels: number, bpp: number, rowBytes: number, size: number,
  idatCount: number, idatBytes: number, paletteOffset: number, paletteLength: number, transparencyOffset: number, transparencyLength: number,
};
export declare type PngImage = { info: PngInfo, data: Uint8Array };
export declare function pngInfo(file: Uint8Array): PngInfo;
/** `interlaced: true` lets Adam7-interlaced files decode too (refused otherwise); the result is that of a non-interlaced file of the same pixels. */
export declare type PngOptions = { interlaced?: boolean };
export declare function pngDecode(file: Uint8Array, options?: PngOptions): PngImage;
export declare type PngResult = PngImage | Error;
export declare function pngDecodeBatch(files: Uint8Array[], options?: PngOptions): PngResult[];
/** PNG images as pixels: `data` is width * height * 4 bytes of R, G, B, A (sub-byte samples scaled, 16-bit samples cut to the high byte, palette and tRNS applied). */
export declare function pngPixels(file: Uint8Array, options?: PngOptions): PngImage;
export declare function pngPixelsBatch(files: Uint8Array[], options?: PngOptions): PngResult[];
/** PNG images, writing: scanlines as pngDecode gives them to files, one batch on the device; filter 0..4 fixed, 6 adaptive, 5 (default) adaptive with restart rows. */
export declare type PngSource = {
  data: Uint8Array, width: number, height: number, colourType: number, depth?: number, filter?: number, palette?: Uint8Array, transparency?: Uint8Array,
};
export declare function pngEncode(image: PngSource): Uint8Array;
export declare function pngEncodeBatch(images: PngSource[]): BatchResult[];
/** TIFF images, reading: a directory's geometry on the host, and a rectangle of it decoded on the device (uncompressed and zlib-compressed tiles or strips, Predictor 2 undone, samples little-endian). */
export declare type TiffInfo = {
  width: number, height: number, segmentWidth: number, segmentHeight: number, across: number, down: number, bits: number, samples: number,
  compression: number, predictor: number, photometric: number, sampleFormat: number, extraSamples: number, bigEndian: boolean, tiled: boolean,
  size: number, dirs: number };
export declare type TiffRect = { x: number, y: number, w: number, h: number };
export declare type TiffOptions = { dir?: number, rect?: TiffRect };
export declare type TiffImage = { width: number, height: number, samples: number, bits: number, data: Uint8Array };
export declare function tiffInfo(file: Uint8Array, dir?: number): TiffInfo;
export declare function tiffRead(file: Uint8Array, options?: TiffOptions): TiffImage;
/** TIFF images, writing: one image to one classic TIFF file; `info` as tiffInfo gives it (across, down, size and dirs optional), so that info -> read -> write round-trips. */
export declare type TiffRecord = Omit<TiffInfo, 'across' | 'down' | 'size' | 'dirs'> & { across?: number, down?: number, size?: number, dirs?: number };
export declare function tiffWrite(pixels: Uint8Array, info: TiffRecord): Uint8Array;
export declare function init(device: number): void;
export declare function initDevices(n?: number): number;
export declare function trim(): void;
