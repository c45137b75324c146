/* bhr_output.h -- frame output of libbhr_hip.so: PNG encoding and the pipelined frame sink.
 *
 * Replaces the reference's host output path: save_image (render.py:420-425, PIL) for still images and
 * the two-thread PIL pool of render_video (render.py:4412-4413, 4458-4467), which caps the video driver
 * at a few frames per second once a frame renders in a millisecond.  Files are ordinary 8-bit RGB PNGs;
 * the decoded pixels equal (np.clip(frame, 0, 1) * 255).astype(np.uint8) of the reference exactly,
 * the compressed bytes differ (they also differ between PIL versions).
 */
#ifndef BHR_OUTPUT_H
#define BHR_OUTPUT_H

#include "bhr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Encode an (h, w, 3) u8 image.  level: zlib level 0..9 (PIL's default is 6).  threads > 1 deflates
 * row bands in parallel and splices them into one stream.  out must hold bhr_png_bound(w, h) bytes. */
BHR_API int64_t bhr_png_bound(int32_t w, int32_t h);
BHR_API int32_t bhr_png_encode(const uint8_t *rgb, int32_t w, int32_t h, int32_t level, int32_t threads,
                               uint8_t *out, int64_t cap, int64_t *out_len);
/* Image.fromarray(rgb).save(path): encode and write atomically (path.tmp, then rename). */
BHR_API int32_t bhr_png_write(const char *path, const uint8_t *rgb, int32_t w, int32_t h, int32_t level, int32_t threads);

/* The same three for 16 bits per sample: rgb is (h, w, 3) u16, native endian; the file is colour type 2 at bit depth 16 with the
 * samples big-endian, as PNG wants them.  Same adaptive filters (at a filter distance of 6 bytes: one pixel), parallel row bands
 * and atomic write.  The decoded samples equal the input exactly. */
BHR_API int64_t bhr_png_bound16(int32_t w, int32_t h);
BHR_API int32_t bhr_png_encode16(const uint16_t *rgb, int32_t w, int32_t h, int32_t level, int32_t threads,
                                 uint8_t *out, int64_t cap, int64_t *out_len);
BHR_API int32_t bhr_png_write16(const char *path, const uint16_t *rgb, int32_t w, int32_t h, int32_t level, int32_t threads);

/* PNG encoding on the device (csrc/png_device.hip).  The frame is filtered (the five PNG filters, the minimum sum of
 * absolute residuals per scanline) and entropy coded in HBM: one dynamic-Huffman deflate block and one IDAT chunk per
 * scanline, the prefix code of each scanline picked from a menu of 16 static codes (no LZ77 matches), chunk CRC-32 and
 * stream Adler-32 computed on the device.  Any PNG reader decodes the result to exactly the pixels of
 * bhr_read_final_u8; the files are ~15-25 % larger than zlib level 1 makes them and cost a fraction of a millisecond
 * of device time instead of ~50 ms of a host core per fhd frame.  Replaces the same reference code as the host
 * encoder (render.py:420-425, 4412-4467).
 *   bhr_png_device_bound: capacity that always suffices for a w x h frame.
 *   bhr_png_encode_device: quantise the context's FINAL layer and encode it; `out` (host) receives the file bytes.
 *   BHR_PNG_DEVICE as the `level` of bhr_sink_create: the sink encodes on the device, its workers only fetch the
 *     finished bytes (an exact-length copy on their own stream) and write the file. */
#define BHR_PNG_DEVICE (-1)
BHR_API int64_t bhr_png_device_bound(int32_t w, int32_t h);
/* Widest frame the device encoder takes (one scanline is coded by one block out of LDS): 17 000-odd pixels.
 * bhr_png_encode_device and bhr_sink_create(.., BHR_PNG_DEVICE, ..) fail with BHR_ERR_INVALID beyond it. */
BHR_API int32_t bhr_png_device_max_width(void);
BHR_API int32_t bhr_png_encode_device(bhr_ctx *ctx, uint8_t *out, int64_t cap, int64_t *out_len);
/* Entry k of the code menu, as the kernels use it (host only, no GPU needed; for inspection and tests):
 * codes[257] = (bit-reversed code << 4) | length for literals 0..255 and end-of-block, hdr_words[64] / *hdr_bits =
 * the deflate block header announcing that code, LSB first.  *n_tables receives the menu size. */
BHR_API int32_t bhr_png_device_menu(int32_t k, uint32_t *codes, uint32_t *hdr_words, uint32_t *hdr_bits, int32_t *n_tables);

/* 16-bit PNG on the device: the same scheme -- one scanline = one deflate block = one IDAT chunk, the five filters by the
 * minimum sum of absolute residuals (filter distance 6 bytes), Huffman coding only from a static menu, CRC-32 and Adler-32 on
 * the device -- over the context's 16-bit rows (bhr_read_final_u16; big-endian in the file).  The menu is the encoder's own:
 * 15 codes fitted to the mixture a filtered 16-bit scanline is (peaked high bytes, nearly uniform low bytes) + the flat code.
 * Any PNG reader decodes the file to exactly the samples of bhr_read_final_u16.
 *   bhr_png16_device_bound: capacity that always suffices for a w x h frame (0 beyond the width limit).
 *   bhr_png16_device_max_width: the same LDS budget holds half as many pixels as at 8 bits: 8530 (7680 fits).
 *   bhr_png16_encode_device: quantise the context's FINAL layer to 16 bits and encode it; BHR_ERR_INVALID beyond the width limit.
 *   bhr_sink_create_png16: an ordinary bhr_sink (submit, drain, destroy below) whose files are 16-bit PNGs; level is
 *     BHR_PNG_DEVICE or a zlib level 0..9 (the host encoder, bhr_png_encode16, on the sink's workers). */
BHR_API int64_t bhr_png16_device_bound(int32_t w, int32_t h);
BHR_API int32_t bhr_png16_device_max_width(void);
BHR_API int32_t bhr_png16_encode_device(bhr_ctx *ctx, uint8_t *out, int64_t cap, int64_t *out_len);

/* Frame sink.  bhr_sink_submit quantises the context's FINAL layer on the device (save_image's
 * truncation), starts an asynchronous copy into one of `slots` pinned host buffers and returns; `workers`
 * host threads wait for the copy, encode and write `path`.  The caller goes on to render the next frame
 * on the same stream meanwhile.  submit blocks only while every slot is busy. */
typedef struct bhr_sink bhr_sink;
BHR_API int32_t bhr_sink_create(bhr_ctx *ctx, int32_t slots, int32_t workers, int32_t level, bhr_sink **out);
/* The sink of 16-bit PNG files (see bhr_png16_encode_device above). */
BHR_API int32_t bhr_sink_create_png16(bhr_ctx *ctx, int32_t slots, int32_t workers, int32_t level, bhr_sink **out);
BHR_API int32_t bhr_sink_submit(bhr_sink *sink, const char *path);
/* Wait until every submitted frame is on disk; returns the first error a worker met, if any.
 * frames_written / bytes_written may be NULL. */
BHR_API int32_t bhr_sink_drain(bhr_sink *sink, int64_t *frames_written, int64_t *bytes_written);
BHR_API void bhr_sink_destroy(bhr_sink *sink);

/* Baseline JPEG encoding on the device (csrc/jpeg_device.hip): the Motion-JPEG path of the video driver.  One JFIF file
 * per frame, fixed so that tests/jpeg_ref.py restates it byte for byte:
 *   SOI, APP0 (JFIF 1.01, density 1:1), one DQT with two 8-bit tables, SOF0 (8 bit, Y 2x2, Cb 1x1, Cr 1x1 = 4:2:0, tables
 *   0 / 1 / 1), one DHT with the four standard Huffman tables of ITU T.81 Annex K (never built per frame), DRI, SOS,
 *   entropy-coded data, EOI.  No 4:4:4, no progressive, optimised or arithmetic coding, no grey scale.
 *   Quantisation tables: Annex K.1 scaled as libjpeg does, s = 5000 / q for q < 50, else 200 - 2 q,
 *     entry = clamp((base s + 50) / 100, 1, 255).
 *   Colour: from the u8 frame of bhr_read_final_u8, padded to multiples of 16 by repeating its last column and row.
 *     Full-range BT.601 in integers: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16; chroma from the 2x2 block's rounded mean
 *     RGB ((sum + 2) >> 2, as bhr_y4m_submit): Cb = clamp((-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16, 0, 255),
 *     Cr = clamp((32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16, 0, 255).
 *   DCT, int32 only: MI[u][x] = round(8192 c(u) / 2 cos((2x + 1) u pi / 16)); rows t = (MI . p + 1024) >> 11 on the
 *     level-shifted samples, columns f8 = (MI . t + 2048) >> 12 (eight times the coefficient),
 *     q = sign(f8) ((|f8| + 4 Q) / (8 Q)).  |t| < 2^15 and every sum stays below 2^31 for every 8-bit block.
 *   Entropy coding: MCU = Y00 Y01 Y10 Y11 Cb Cr in raster order; DC differences against the previous block of the same
 *     component, 0 at every restart; ZRL for runs above 15, EOB unless coefficient 63 is non-zero; 0x00 behind every 0xFF
 *     data byte; the last byte of an interval padded with 1-bits; RSTm, m counting modulo 8, between intervals.
 *   Restart interval R = bhr_jpeg_restart_interval(w) MCUs: the encoder's unit of parallelism (one wave codes one
 *     interval, one lane per 8x8 block) and part of the file format.  It is a function of the frame's width only; today
 *     it is 10 for every width (60 of a wave's 64 lanes busy; 816 intervals at 1920x1080, 12 960 at 7680x4320), and
 *     intervals run on across MCU rows.  Decoded pixels do not depend on it; it costs about 3 bytes per interval.
 * bhr_jpeg_device_bound: capacity that always suffices: a block codes in at most 20 + 63 x 26 = 1658 bits, an MCU in
 *   1244 bytes, doubled by stuffing, + a padding byte and two marker bytes per interval, + 640 bytes for the headers.
 * bhr_jpeg_tables (host only, no GPU needed; for inspection and tests): the two quantisation tables of `quality` in
 *   zig-zag order and the four Huffman tables in DHT order (DC luma, AC luma, DC chroma, AC chroma): BITS, and HUFFVAL
 *   padded with zeros to 162 entries.
 * bhr_jpeg_encode_device: quantise the context's FINAL layer and encode it, as bhr_png_encode_device does for PNG.  A
 *   row-block context encodes its own rows as a `rows`-high image.  There is no width limit below the format's 65535.
 * bhr_sink_create_jpeg: an ordinary bhr_sink (submit, drain, destroy below) whose submits encode JPEG on the device.
 * quality outside 1..100: BHR_ERR_INVALID. */
BHR_API int64_t bhr_jpeg_device_bound(int32_t w, int32_t h);
BHR_API int32_t bhr_jpeg_restart_interval(int32_t w);
BHR_API int32_t bhr_jpeg_tables(int32_t quality, uint8_t *qtab /* [2][64] */, uint8_t *huff_counts /* [4][16] */,
                                uint8_t *huff_values /* [4][162] */);
BHR_API int32_t bhr_jpeg_encode_device(bhr_ctx *ctx, int32_t quality, uint8_t *out, int64_t cap, int64_t *out_len);
BHR_API int32_t bhr_sink_create_jpeg(bhr_ctx *ctx, int32_t slots, int32_t workers, int32_t quality, bhr_sink **out);

/* Video stream without the PNG detour (replaces render.py:4497-4503, where the reference re-reads every PNG and
 * feeds libx264 through imageio/pyav with pixelformat yuv420p).  bhr_y4m_submit converts the context's FINAL layer
 * on the device -- the reference's u8 quantisation (render.py:4463), then BT.601 limited-range Y'CbCr with the
 * chroma of each 2x2 block taken from its rounded mean RGB (4:2:0, centre sited) -- copies the 1.5 bytes/pixel
 * asynchronously into a pinned ring and returns; ONE writer thread appends the frames in submission order to
 * `path` as YUV4MPEG2 ("YUV4MPEG2 W.. H.. F<num>:<den> Ip A1:1 C420jpeg XCOLORRANGE=LIMITED", then "FRAME\n" + Y, Cb, Cr
 * planes per frame).  `path` may be a FIFO or "-"-less file path; `ffmpeg -f yuv4mpegpipe -i path -c:v libx264 -pix_fmt
 * yuv420p out.mp4` turns it into the reference's MP4 (drivers.render_video does that when an ffmpeg binary exists).
 * Width and height must be even.  Integer arithmetic (exactly reproducible on the host):
 *   Y  = ((66 R + 129 G + 25 B + 128) >> 8) + 16,  Cb = ((-38 R - 74 G + 112 B + 128) >> 8) + 128,
 *   Cr = ((112 R - 94 G - 18 B + 128) >> 8) + 128,  chroma R,G,B = (sum of the 2x2 block + 2) >> 2. */
typedef struct bhr_y4m bhr_y4m;
BHR_API int32_t bhr_y4m_open(bhr_ctx *ctx, const char *path, int32_t fps_num, int32_t fps_den, int32_t slots, bhr_y4m **out);
BHR_API int32_t bhr_y4m_submit(bhr_y4m *stream);
/* Wait until every submitted frame has been written; first writer error, if any.  frames_written may be NULL. */
BHR_API int32_t bhr_y4m_drain(bhr_y4m *stream, int64_t *frames_written, int64_t *bytes_written);
/* Drains, closes the file and frees the stream. */
BHR_API void bhr_y4m_close(bhr_y4m *stream);

/* HDR video stream (csrc/hdr_stream.hip): 10-bit BT.2020 Y'CbCr 4:2:0 with a PQ (SMPTE ST 2084) or HLG (BT.2100) transfer,
 * made from the frame's scene-linear HDR plane h (bhr_set_grade with keep_hdr: BT.709 primaries, 0 <= h <= 65504, unclipped,
 * with the flare if the frame had one) -- a consumer of that plane beside the grade stage, so the SDR frame files and this
 * stream come out of one render of each frame.  bhr_y4m_open_hdr opens a stream that bhr_y4m_submit, _drain and _close serve
 * like the 8-bit one; its header line is "YUV4MPEG2 W.. H.. F<num>:<den> Ip A1:1 C420p10 XCOLORRANGE=LIMITED" and a frame is
 * "FRAME\n" + planar little-endian uint16 Y (W H) | Cb (W H / 4) | Cr: 3 W H bytes, what `ffmpeg -f yuv4mpegpipe` reads as
 * yuv420p10le and x265 takes as it is (-color_primaries bt2020 -color_trc smpte2084 | arib-std-b67 -colorspace bt2020nc).
 * Per pixel, all in f32, every operation rounded once (no contraction):
 *   v       = h * gain                                    gain = (float)exp2((double)exposure_stops)
 *   (R,G,B) = M . v, each row ((m0 r + m1 g) + m2 b)      BT.709 -> BT.2020 (BT.2087):
 *                                                         0.6274 0.3293 0.0433 / 0.0691 0.9195 0.0114 / 0.0164 0.0880 0.8956
 *   BHR_HDR_PQ   Y  = fminf(X * (white_nits / 10000), 1)  scene value 1.0 is white_nits on the display
 *                E' = ((c1 + c2 Y^m1) / (1 + c3 Y^m1))^m2,  every power x^e evaluated as exp2f(e * log2f(x))
 *                m1 = 2610/16384, m2 = 2523/4096*128, c1 = 3424/4096, c2 = 2413/4096*32, c3 = 2392/4096*32
 *   BHR_HDR_HLG  E  = fminf(X * 0.265, 1)                 scene value 1.0 is the 75 % reference white (BT.2408)
 *                E' = E <= 1/12 ? sqrtf(3 E) : a logf(12 E - b) + c     a = 0.17883277, b = 0.28466892, c = 0.55991073
 *   Y'  = (0.2627 R' + 0.6780 G') + 0.0593 B'             BT.2020 non-constant luminance
 *   DY  = clamp((int)floorf(876 Y' + 64.5f), 64, 940)
 * Chroma, one pair per 2x2 block, centre sited as in the 8-bit stream: the mean R'G'B' of the four pixels, summed as
 * ((a + b) + (c + d)) * 0.25f with a, b the upper and c, d the lower row, its own Y' as above, Cb = (B' - Y') / 1.8814,
 * Cr = (R' - Y') / 1.4746, DC = clamp((int)floorf(896 C + 512.5f), 64, 960).
 * Dither (bhr_set_dither) does not apply: the stream is quantised from floats, never from the context's u8 rows.
 * Light levels (PQ only; HLG carries no such metadata and reports 0, 0): per pixel nits = fminf(white_nits * max(R, G, B), 10000);
 * the stream keeps MaxCLL, the largest pixel over all frames written, and MaxFALL, the largest frame mean (the frame's sum is
 * kept in binary64).  bhr_y4m_light_levels: out = {MaxCLL, MaxFALL} of the frames written so far; call it after a drain.
 * bhr_y4m_submit on an HDR stream: BHR_ERR_STATE when the frame in the active slot kept no HDR plane.  bhr_y4m_open_hdr:
 * BHR_ERR_INVALID for a transfer other than the two, exposure_stops non-finite or outside [-16, 16], for PQ white_nits
 * non-finite or outside (0, 10000] (HLG ignores the field), reserved != 0, and what bhr_y4m_open refuses (odd sizes). */
#define BHR_HDR_PQ 1
#define BHR_HDR_HLG 2
typedef struct { int32_t transfer; float exposure_stops; float white_nits; int32_t reserved; } bhr_hdr_stream;
BHR_API int32_t bhr_y4m_open_hdr(bhr_ctx *ctx, const char *path, int32_t fps_num, int32_t fps_den, int32_t slots,
                                 const bhr_hdr_stream *cfg, bhr_y4m **out);
BHR_API int32_t bhr_y4m_light_levels(bhr_y4m *stream, double out[2]);

#ifdef __cplusplus
}
#endif
#endif /* BHR_OUTPUT_H */
