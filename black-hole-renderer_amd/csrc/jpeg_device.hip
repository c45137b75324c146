// jpeg_device.hip -- baseline JPEG encoding of the quantised frame ON THE DEVICE (include/bhr_output.h).
//
// The Motion-JPEG path of the video driver: the (rows, W, 3) u8 frame in HBM becomes the bytes of a complete JFIF file in
// HBM, and only those (about 0.2 byte per pixel at quality 90) cross PCIe.  The format is fixed by bhr_output.h and
// restated in NumPy by tests/jpeg_ref.py, which these kernels reproduce byte for byte:
//   * baseline sequential DCT, 8 bit, 4:2:0 (MCU = Y00 Y01 Y10 Y11 Cb Cr), the frame padded to multiples of 16 by repeating
//     its last column and row;
//   * full-range BT.601 in integers, chroma from the rounded mean RGB of each 2x2 block;
//   * an int32 fixed-point DCT: rows t = (MI . p + 1024) >> 11, columns f8 = (MI . t + 2048) >> 12 (eight times the
//     coefficient), q = sign(f8) ((|f8| + 4 Q) / (8 Q));
//   * the four standard Huffman tables of ITU T.81 Annex K, never built per frame (the decision of the PNG coder's menu);
//   * a restart interval of kR MCUs: intervals are coded independently, one wave each, and are the unit of parallelism.
// Three launches, the PNG encoder's plan (png_device.hip):
//   jpeg_encode_kernel  one wave per restart interval: colour conversion, DCT, quantisation, zig-zag into LDS; one lane per
//                       8x8 block turns its coefficients into bits (a wave prefix sum over the lengths places them), the
//                       bit string is merged into LDS words, byte-stuffed (a ballot prefix over the 0xFF bytes) and stored
//                       in the interval's fixed-stride scratch slot with its length;
//   jpeg_scan_kernel    exclusive scan of the lengths (+ 2 per RSTm marker): offsets, total length, error word, header, EOI;
//   jpeg_gather_kernel  every interval copied to its final offset behind its RSTm marker.
#include "bhr_internal.h"
#include "../../include/bhr_output.h"

#include <cstring>
#include <vector>

namespace {

constexpr int kR = 10;                       // MCUs per restart interval: 60 blocks, one per lane of a wave
constexpr int kWave = 64;
constexpr int kCoefStride = 66;              // int16 per coded block in LDS: 33 words, so that lanes walk distinct banks
constexpr int kBlockBits = 20 + 63 * 26;     // DC: 9-bit code + 11 bits; every AC: 16-bit code + 10 bits
constexpr int kMcuBytes = (6 * kBlockBits + 7) / 8;                  // 1244
constexpr int kBitsWords = (kR * kMcuBytes + 3) / 4 + 2;
constexpr int kSlotStride = (2 * kR * kMcuBytes + 1 + 15) & ~15;     // every byte 0xFF: doubled by stuffing
constexpr int kHeadRoom = 640;               // SOI .. SOS: 613 bytes with DRI
constexpr int kScanThreads = 1024;
static_assert(6 * kR <= kWave, "one lane per block of the interval");
static_assert(kMcuBytes == 1244, "bhr_output.h documents the bound with this figure");

struct JpegTables {
    uint16_t q[2][64];           // luma / chroma quantiser, natural order (8 v + u)
    uint32_t dc[2][16];          // (code << 5) | length by category
    uint32_t ac[2][256];         // (code << 5) | length by (run << 4) | size
    uint32_t head_len;
    uint8_t head[kHeadRoom];     // SOI, APP0, DQT, SOF0, DHT, DRI, SOS
};

struct JpegDev {
    JpegTables *d_tab[101] = {nullptr};       // by quality, made on first use (frames in flight keep reading theirs)
    // interval scratch, lengths and offsets, one set per frame slot: encodes of successive frames run on different streams
    uint8_t *d_scratch[BHR_MAX_FRAME_SLOTS] = {nullptr, nullptr};
    uint32_t *d_len[BHR_MAX_FRAME_SLOTS] = {nullptr, nullptr};
    uint32_t *d_offs[BHR_MAX_FRAME_SLOTS] = {nullptr, nullptr};
    uint32_t *d_meta = nullptr;               // [0] file length, [1] error (1: output buffer too small)
    uint8_t *d_out = nullptr;                 // scratch of bhr_jpeg_encode_device
    int64_t out_cap = 0;
};

template <typename T>
int32_t dev_alloc(T **p, size_t count) {
    *p = nullptr;
    hipError_t e = hipMalloc((void **)p, count * sizeof(T));
    if (e != hipSuccess) {
        *p = nullptr;
        return bhr_fail(BHR_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
    }
    return BHR_OK;
}

// ---------------------------------------------------------------------------------------------- host: the standard tables
// zig-zag position -> natural index (T.81 figure 5)
const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// T.81 Annex K.1, tables K.1 and K.2, in zig-zag order (as a DQT segment holds them)
const uint8_t kBaseQ[2][64] = {
    {16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26,  24, 22, 22,  24,  49,
     35, 37, 29, 40, 58, 51, 61, 60, 57, 51, 56, 55, 64, 72, 92, 78, 64,  68, 87, 69,  55,  56,
     80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99},
    {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// T.81 Annex K.3: BITS of tables K.3 (DC luminance), K.5 (AC luminance), K.4 (DC chrominance), K.6 (AC chrominance) -- the
// order of the DHT segment: Tc/Th = 0/0, 1/0, 0/1, 1/1
const uint8_t kHuffId[4] = {0x00, 0x10, 0x01, 0x11};
const uint8_t kHuffBits[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                  {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                  {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                  {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
// HUFFVAL of the AC tables up to where the codes reach 16 bits; the 16-bit codes take every remaining (run, size) symbol
// in ascending order
const uint8_t kAcLumHead[37] = {1,  2,   3,  0,  4,   17,  5,   18, 33, 49, 65,  6,   19,  81, 97, 7,  34, 113, 20,
                                50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98, 114, 130};
const uint8_t kAcChrHead[43] = {0,   1,   2, 3,  17, 4,  5,  33,  49, 6,  18, 65,  81,  7,  97, 113, 19, 34, 50, 129, 8,  20,
                                66,  145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241};

// HUFFVAL of table t (DHT order) into out[162]; returns the number of symbols
int huff_values(int t, uint8_t *out) {
    memset(out, 0, 162);
    if (t == 0 || t == 2) {
        for (int k = 0; k < 12; ++k) out[k] = (uint8_t)k;
        return 12;
    }
    const uint8_t *head = t == 1 ? kAcLumHead : kAcChrHead;
    const int n_head = t == 1 ? (int)sizeof(kAcLumHead) : (int)sizeof(kAcChrHead);
    bool used[256] = {false};
    int n = 0;
    for (; n < n_head; ++n) { out[n] = head[n]; used[head[n]] = true; }
    for (int run = 0; run < 16; ++run)
        for (int size = 1; size <= 10; ++size)
            if (!used[run * 16 + size]) out[n++] = (uint8_t)(run * 16 + size);
    return n;                                             // 162
}

// libjpeg's jpeg_quality_scaling and jpeg_add_quant_table (force_baseline); zig-zag order
void scaled_q(int quality, int t, uint8_t *out) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int k = 0; k < 64; ++k) {
        const int v = ((int)kBaseQ[t][k] * s + 50) / 100;
        out[k] = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
}

void fill_tables(JpegTables *t, int quality, int w, int h) {
    memset(t, 0, sizeof(*t));
    uint8_t qz[2][64], vals[4][162];
    int n_vals[4];
    for (int k = 0; k < 2; ++k) {
        scaled_q(quality, k, qz[k]);
        for (int z = 0; z < 64; ++z) t->q[k][kZigzag[z]] = qz[k][z];
    }
    for (int k = 0; k < 4; ++k) {
        n_vals[k] = huff_values(k, vals[k]);
        uint32_t code = 0;                                 // canonical code, T.81 Annex C
        int at = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int c = 0; c < kHuffBits[k][len - 1]; ++c, ++at, ++code) {
                const uint32_t e = (code << 5) | (uint32_t)len;
                if (k == 0 || k == 2) t->dc[k >> 1][vals[k][at]] = e;
                else t->ac[k >> 1][vals[k][at]] = e;
            }
            code <<= 1;
        }
    }
    uint8_t *p = t->head;
    auto put = [&](std::initializer_list<int> bytes) { for (int b : bytes) *p++ = (uint8_t)b; };
    put({0xFF, 0xD8});
    put({0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});      // JFIF 1.01, density 1:1, no thumbnail
    put({0xFF, 0xDB, 0, 2 + 2 * 65});
    for (int k = 0; k < 2; ++k) {
        *p++ = (uint8_t)k;
        memcpy(p, qz[k], 64);
        p += 64;
    }
    put({0xFF, 0xC0, 0, 17, 8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
    int dht = 2;
    for (int k = 0; k < 4; ++k) dht += 17 + n_vals[k];
    put({0xFF, 0xC4, dht >> 8, dht & 255});
    for (int k = 0; k < 4; ++k) {
        *p++ = kHuffId[k];
        memcpy(p, kHuffBits[k], 16);
        p += 16;
        memcpy(p, vals[k], (size_t)n_vals[k]);
        p += n_vals[k];
    }
    put({0xFF, 0xDD, 0, 4, kR >> 8, kR & 255});
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    t->head_len = (uint32_t)(p - t->head);
}

// ---------------------------------------------------------------------------------------------- device
// natural index (8 v + u) -> zig-zag position
__device__ const uint8_t kZigPos[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                        41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                        46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// One 1-D pass: o[u] = (sum_x MI[u][x] p[x] + round) >> shift, MI[u][x] = round(8192 c(u) / 2 cos((2x + 1) u pi / 16)).
// int32 throughout: |sum| <= 23168 * 128 in the row pass and 23168 * 2^15 in the column pass.
__device__ __forceinline__ void dct_pass(const int (&p)[8], int (&o)[8], int round, int shift) {
    constexpr int MI[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},     {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                              {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784}, {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                              {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                              {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567}, {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        int acc = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) acc += MI[u][x] * p[x];
        o[u] = (acc + round) >> shift;
    }
}

// The interval's bit string, most significant bit first: word k holds bytes 4k .. 4k + 3, byte 4k in its top bits.
struct BitSink {
    uint32_t *words;
    unsigned long long acc;      // pending bits, left aligned behind the nb bits of word wi that precede them
    uint32_t nb, wi;
    __device__ __forceinline__ void put(uint32_t v, uint32_t n) {      // n <= 27, v < 2^n
        acc |= (unsigned long long)v << (64u - nb - n);
        nb += n;
        if (nb >= 32u) {
            atomicOr(&words[wi], (uint32_t)(acc >> 32));
            acc <<= 32;
            nb -= 32u;
            ++wi;
        }
    }
    __device__ __forceinline__ void finish() {
        if (nb && (uint32_t)(acc >> 32)) atomicOr(&words[wi], (uint32_t)(acc >> 32));
    }
};

__device__ __forceinline__ uint32_t category(int v) { return v ? 32u - (uint32_t)__clz(abs(v)) : 0u; }

// Huffman-codes one block (z: 64 coefficients in zig-zag order, the last non-zero one at `last`); returns its bits.
template <bool kEmit>
__device__ __forceinline__ uint32_t code_block(const int16_t *z, int pred, const uint32_t *dc, const uint32_t *ac, int last, BitSink &sink) {
    uint32_t bits = 0;
    auto symbol = [&](uint32_t entry, int v, uint32_t s) {     // code of `entry`, then the s low bits of v (v - 1 if negative)
        const uint32_t extra = (uint32_t)(v > 0 ? v : v + (1 << s) - 1) & ((1u << s) - 1u), n = (entry & 31u) + s;
        bits += n;
        if (kEmit) sink.put(((entry >> 5) << s) | extra, n);
    };
    const int d = (int)z[0] - pred;
    uint32_t s = category(d);
    symbol(dc[s], d, s);
    int run = 0;
    for (int k = 1; k <= last; ++k) {
        const int v = z[k];
        if (v == 0) { ++run; continue; }
        for (; run > 15; run -= 16) symbol(ac[0xF0], 0, 0);    // ZRL
        s = category(v);
        symbol(ac[(run << 4) | (int)s], v, s);
        run = 0;
    }
    if (last < 63) symbol(ac[0], 0, 0);                          // EOB
    return bits;
}

// K1: one wave per restart interval.
__global__ __launch_bounds__(kWave) void jpeg_encode_kernel(const uint8_t *__restrict__ rgb, int w, int h, int mcus_x, int n_mcus,
                                                            const JpegTables *__restrict__ tab, uint8_t *__restrict__ scratch,
                                                            uint32_t *__restrict__ lens) {
    // samples (6 kR blocks of 64 int16, block-major) until the column pass has read them, then the bit string
    __shared__ __align__(16) uint32_t bits_or_samples[kBitsWords];
    __shared__ __align__(16) int16_t coef[6 * kR * kCoefStride];
    __shared__ uint32_t huff_dc[2][16], huff_ac[2][256];
    __shared__ uint16_t quant[2][64];
    static_assert(sizeof(bits_or_samples) >= 6 * kR * 64 * sizeof(int16_t), "the samples fit the bit buffer");
    int16_t *smp = (int16_t *)bits_or_samples;
    const int lane = threadIdx.x, interval = blockIdx.x, m0 = interval * kR, nm = min(kR, n_mcus - m0);

    for (int i = lane; i < 2 * 256; i += kWave) (&huff_ac[0][0])[i] = (&tab->ac[0][0])[i];
    if (lane < 32) (&huff_dc[0][0])[lane] = (&tab->dc[0][0])[lane];
    for (int i = lane; i < 2 * 64; i += kWave) (&quant[0][0])[i] = (&tab->q[0][0])[i];

    {   // colour: one lane per 2x2 pixels of the MCU -> four Y, one Cb, one Cr, level shifted
        const int qy = lane >> 3, qx = lane & 7;
        for (int m = 0; m < nm; ++m) {
            const int my = (m0 + m) / mcus_x, mx = (m0 + m) - my * mcus_x;
            int16_t *blk = smp + m * 6 * 64;
            int sr = 0, sg = 0, sb = 0;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int yy = 2 * qy + dy, xx = 2 * qx + dx;                          // inside the 16x16 MCU
                    const int y = min(16 * my + yy, h - 1), x = min(16 * mx + xx, w - 1);  // the last row / column repeats
                    const uint8_t *p = rgb + ((size_t)y * w + x) * 3;
                    const int r = p[0], g = p[1], b = p[2];
                    const int Y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
                    blk[((yy >> 3) * 2 + (xx >> 3)) * 64 + (yy & 7) * 8 + (xx & 7)] = (int16_t)(Y - 128);
                    sr += r; sg += g; sb += b;
                }
            const int r = (sr + 2) >> 2, g = (sg + 2) >> 2, b = (sb + 2) >> 2;
            const int cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
            const int cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
            blk[4 * 64 + qy * 8 + qx] = (int16_t)(min(max(cb, 0), 255) - 128);
            blk[5 * 64 + qy * 8 + qx] = (int16_t)(min(max(cr, 0), 255) - 128);
        }
    }
    __syncthreads();
    for (int item = lane; item < nm * 48; item += kWave) {         // rows, in place: item = (block, y)
        int16_t *row = smp + item * 8;
        int p[8], t[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) p[x] = row[x];
        dct_pass(p, t, 1 << 10, 11);
#pragma unroll
        for (int u = 0; u < 8; ++u) row[u] = (int16_t)t[u];          // |t| < 2^15
    }
    __syncthreads();
    for (int item = lane; item < nm * 48; item += kWave) {         // columns: item = (block, u) -> quantised, zig-zag
        const int blk = item >> 3, u = item & 7;
        const int16_t *col = smp + blk * 64 + u;
        const uint16_t *q = quant[(blk % 6) < 4 ? 0 : 1];
        int t[8], f8[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) t[y] = col[8 * y];
        dct_pass(t, f8, 1 << 11, 12);
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const int Q = q[8 * v + u], a = (abs(f8[v]) + 4 * Q) / (8 * Q);
            coef[blk * kCoefStride + kZigPos[8 * v + u]] = (int16_t)(f8[v] < 0 ? -a : a);
        }
    }
    __syncthreads();
    for (int i = lane; i < kBitsWords; i += kWave) bits_or_samples[i] = 0u;   // the samples are dead: their space takes the bits
    __syncthreads();

    // entropy coding: lane = block of the interval, in stream order
    const bool coding = lane < 6 * nm;
    const int b = lane % 6, ti = b < 4 ? 0 : 1;
    const int16_t *z = coef + lane * kCoefStride;
    int pred = 0, last = 0;
    uint32_t my_bits = 0;
    BitSink sink;
    sink.words = bits_or_samples;
    if (coding) {
        // DC prediction: the previous block of the same component in the interval, 0 at its start
        if (b >= 1 && b <= 3) pred = z[-kCoefStride];
        else if (lane >= 6) pred = z[-(b == 0 ? 3 : 6) * kCoefStride];
        for (last = 63; last > 0 && z[last] == 0; --last) {}
        my_bits = code_block<false>(z, pred, huff_dc[ti], huff_ac[ti], last, sink);
    }
    uint32_t incl = my_bits;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, kWave);
        if (lane >= d) incl += o;
    }
    const uint32_t total_bits = __shfl(incl, kWave - 1, kWave);
    if (coding) {
        const uint32_t pos = incl - my_bits;
        sink.acc = 0;
        sink.nb = pos & 31u;
        sink.wi = pos >> 5;
        (void)code_block<true>(z, pred, huff_dc[ti], huff_ac[ti], last, sink);
        sink.finish();
    }
    __syncthreads();
    if (lane == 0 && (total_bits & 7u)) {                          // the last byte is padded with 1-bits
        const uint32_t n = 8u - (total_bits & 7u);
        bits_or_samples[total_bits >> 5] |= ((1u << n) - 1u) << (32u - (total_bits & 31u) - n);
    }
    __syncthreads();

    // byte stuffing: a 0x00 behind every 0xFF; the ballot's prefix count places the bytes
    const uint32_t n_bytes = (total_bits + 7u) >> 3;
    uint8_t *dst = scratch + (size_t)interval * kSlotStride;
    uint32_t stuffed = 0;
    for (uint32_t base = 0; base < n_bytes; base += kWave) {
        const uint32_t i = base + lane;
        const bool valid = i < n_bytes;
        const uint32_t byte = valid ? (bits_or_samples[i >> 2] >> (24u - 8u * (i & 3u))) & 255u : 0u;
        const bool ff = valid && byte == 255u;
        const unsigned long long mask = __ballot(ff);
        const uint32_t at = i + stuffed + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (valid) {
            dst[at] = (uint8_t)byte;
            if (ff) dst[at + 1] = 0;
        }
        stuffed += (uint32_t)__popcll(mask);
    }
    if (lane == 0) lens[interval] = n_bytes + stuffed;
}

// K2: interval offsets (exclusive scan of length + 2 marker bytes), total length, error word, header and EOI.
__global__ __launch_bounds__(kScanThreads) void jpeg_scan_kernel(const uint32_t *__restrict__ lens, int n, const JpegTables *__restrict__ tab,
                                                                 uint32_t *__restrict__ offs, uint32_t *__restrict__ meta,
                                                                 uint8_t *__restrict__ out, long long cap) {
    __shared__ unsigned long long sc[kScanThreads];
    __shared__ unsigned long long carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = tab->head_len;
    __syncthreads();
    for (int base = 0; base < n; base += kScanThreads) {
        const int i = base + tid;
        // interval i > 0 is preceded by its RSTm marker: the marker's two bytes count with the interval before it
        const unsigned long long len = i < n ? (unsigned long long)lens[i] + (i + 1 < n ? 2ull : 0ull) : 0ull;
        sc[tid] = len;
        __syncthreads();
        for (int d = 1; d < kScanThreads; d <<= 1) {
            const unsigned long long v = tid >= d ? sc[tid - d] : 0ull;
            __syncthreads();
            sc[tid] += v;
            __syncthreads();
        }
        if (i < n) offs[i] = (uint32_t)(carry + sc[tid] - len);
        __syncthreads();
        if (tid == 0) carry += sc[kScanThreads - 1];
        __syncthreads();
    }
    const unsigned long long total = carry + 2;                       // + EOI
    const bool too_big = total > (unsigned long long)cap || total > 0xFFFFFFF0ull;
    if (tid == 0) {
        meta[0] = (uint32_t)total;
        meta[1] = too_big ? 1u : 0u;
        meta[2] = 0u;
        meta[3] = 0u;
    }
    if (!too_big) {
        for (uint32_t i = tid; i < tab->head_len; i += kScanThreads) out[i] = tab->head[i];
        if (tid == 0) { out[carry] = 0xFF; out[carry + 1] = 0xD9; }
    }
}

// K3: every interval to its place, RSTm (m = interval index - 1 modulo 8) in front of all but the first.
__global__ __launch_bounds__(kWave) void jpeg_gather_kernel(const uint8_t *__restrict__ scratch, const uint32_t *__restrict__ lens,
                                                            const uint32_t *__restrict__ offs, const uint32_t *__restrict__ meta,
                                                            uint8_t *__restrict__ out) {
    if (meta[1]) return;                                               // the file does not fit the output buffer
    const int interval = blockIdx.x, lane = threadIdx.x;
    const uint8_t *src = scratch + (size_t)interval * kSlotStride;
    uint8_t *dst = out + offs[interval];
    const uint32_t len = lens[interval];
    if (interval > 0 && lane < 2) dst[lane - 2] = lane == 0 ? (uint8_t)0xFF : (uint8_t)(0xD0 + ((interval - 1) & 7));
    for (uint32_t i = lane; i < len; i += kWave) dst[i] = src[i];
}

JpegDev *dev_of(bhr_ctx *ctx) { return (JpegDev *)ctx->jpeg_dev; }

int64_t mcus_of(int w, int h) { return (int64_t)((w + 15) / 16) * ((h + 15) / 16); }
int64_t intervals_of(int w, int h) { return (mcus_of(w, h) + kR - 1) / kR; }

// State, the tables of `quality` and the active frame slot's scratch (idempotent).  Every pointer is checked on its own.
int32_t prepare(bhr_ctx *ctx, int quality) {
    const int w = ctx->cfg.width, h = ctx->rows;
    JpegDev *d = dev_of(ctx);
    if (!d) {
        d = new JpegDev();
        ctx->jpeg_dev = d;
    }
    if (!d->d_tab[quality]) {
        std::vector<JpegTables> t(1);
        fill_tables(&t[0], quality, w, h);
        JpegTables *dt = nullptr;
        BHR_TRY(dev_alloc(&dt, 1));
        hipError_t e = hipMemcpyAsync(dt, &t[0], sizeof(JpegTables), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);          // the host copy goes out of scope
        if (e != hipSuccess) {
            (void)hipFree(dt);
            return bhr_fail(BHR_ERR_HIP, "device JPEG encoder: uploading the tables: %s", hipGetErrorString(e));
        }
        d->d_tab[quality] = dt;
    }
    const int k = ctx->active_slot;
    const size_t n = (size_t)intervals_of(w, h);
    if (!d->d_scratch[k]) BHR_TRY(dev_alloc(&d->d_scratch[k], n * kSlotStride));
    if (!d->d_len[k]) BHR_TRY(dev_alloc(&d->d_len[k], n));
    if (!d->d_offs[k]) BHR_TRY(dev_alloc(&d->d_offs[k], n));
    if (!d->d_meta) BHR_TRY(dev_alloc(&d->d_meta, 4));
    return BHR_OK;
}

int32_t check_args(const bhr_ctx *ctx, int quality, const char *who) {
    if (quality < 1 || quality > 100) return bhr_fail(BHR_ERR_INVALID, "%s: quality %d outside 1..100", who, quality);
    if (ctx->cfg.width > 65535 || ctx->rows > 65535)
        return bhr_fail(BHR_ERR_INVALID, "%s: a JPEG frame is at most 65535 pixels wide and high, this one is %dx%d", who, ctx->cfg.width, ctx->rows);
    return BHR_OK;
}

}  // namespace

void bhr_jpeg_dev_free(bhr_ctx *ctx) {
    JpegDev *d = dev_of(ctx);
    if (!d) return;
    for (JpegTables *t : d->d_tab)
        if (t) (void)hipFree(t);
    for (int k = 0; k < BHR_MAX_FRAME_SLOTS; ++k) {
        if (d->d_scratch[k]) (void)hipFree(d->d_scratch[k]);
        if (d->d_len[k]) (void)hipFree(d->d_len[k]);
        if (d->d_offs[k]) (void)hipFree(d->d_offs[k]);
    }
    if (d->d_meta) (void)hipFree(d->d_meta);
    if (d->d_out) (void)hipFree(d->d_out);
    delete d;
    ctx->jpeg_dev = nullptr;
}

// Encodes the (rows, W, 3) u8 image at d_rgb into d_out (cap bytes) on ctx->stream; d_meta_out (4 words, device) receives
// {file length, error, 0, 0}.  The interval scratch is the active frame slot's.
int32_t bhr_launch_jpeg_encode(bhr_ctx *ctx, int32_t quality, const uint8_t *d_rgb, uint8_t *d_out, int64_t cap, uint32_t *d_meta_out) {
    BHR_TRY(check_args(ctx, quality, "device JPEG encoder"));
    BHR_TRY(prepare(ctx, quality));
    JpegDev *d = dev_of(ctx);
    const int w = ctx->cfg.width, h = ctx->rows, k = ctx->active_slot;
    const int n_mcus = (int)mcus_of(w, h), n_int = (int)intervals_of(w, h);
    const JpegTables *tab = d->d_tab[quality];
    hipLaunchKernelGGL(jpeg_encode_kernel, dim3(n_int), dim3(kWave), 0, ctx->stream, d_rgb, w, h, (w + 15) / 16, n_mcus, tab,
                       d->d_scratch[k], d->d_len[k]);
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, d->d_len[k], n_int, tab, d->d_offs[k], d_meta_out,
                       d_out, (long long)cap);
    hipLaunchKernelGGL(jpeg_gather_kernel, dim3(n_int), dim3(kWave), 0, ctx->stream, d->d_scratch[k], d->d_len[k], d->d_offs[k],
                       d_meta_out, d_out);
    BHR_HIP(hipGetLastError());
    return BHR_OK;
}

extern "C" {

int32_t bhr_jpeg_restart_interval(int32_t w) { return w > 0 ? kR : 0; }

int64_t bhr_jpeg_device_bound(int32_t w, int32_t h) {
    if (w <= 0 || h <= 0) return 0;
    // an MCU codes in at most kMcuBytes, doubled by stuffing; per interval a padding byte and two marker bytes; the header
    return mcus_of(w, h) * 2 * kMcuBytes + intervals_of(w, h) * 3 + kHeadRoom;
}

int32_t bhr_jpeg_tables(int32_t quality, uint8_t *qtab, uint8_t *huff_counts, uint8_t *huff_values_out) {
    if (quality < 1 || quality > 100) return bhr_fail(BHR_ERR_INVALID, "bhr_jpeg_tables: quality %d outside 1..100", quality);
    if (!qtab || !huff_counts || !huff_values_out) return bhr_fail(BHR_ERR_INVALID, "bhr_jpeg_tables: null argument");
    for (int k = 0; k < 2; ++k) scaled_q(quality, k, qtab + 64 * k);
    for (int k = 0; k < 4; ++k) {
        memcpy(huff_counts + 16 * k, kHuffBits[k], 16);
        (void)huff_values(k, huff_values_out + 162 * k);
    }
    return BHR_OK;
}

int32_t bhr_jpeg_encode_device(bhr_ctx *ctx, int32_t quality, uint8_t *out, int64_t cap, int64_t *out_len) {
    if (!ctx || !out || !out_len) return bhr_fail(BHR_ERR_INVALID, "bhr_jpeg_encode_device: null argument");
    BHR_TRY(check_args(ctx, quality, "bhr_jpeg_encode_device"));
    BHR_TRY(bhr_enter(ctx));
    BHR_TRY(prepare(ctx, quality));
    JpegDev *d = dev_of(ctx);
    const int64_t bound = bhr_jpeg_device_bound(ctx->cfg.width, ctx->rows);
    if (d->out_cap < bound) {
        if (d->d_out) (void)hipFree(d->d_out);
        d->d_out = nullptr;
        d->out_cap = 0;
        BHR_TRY(dev_alloc(&d->d_out, (size_t)bound));
        d->out_cap = bound;
    }
    BHR_TRY(bhr_ensure_outputs(ctx, BHR_OUT_U8));
    BHR_TRY(bhr_launch_jpeg_encode(ctx, quality, bhr_slot(ctx).d_final_u8, d->d_out, bound, d->d_meta));
    uint32_t meta[4] = {0, 0, 0, 0};
    BHR_HIP(hipMemcpyAsync(meta, d->d_meta, sizeof(meta), hipMemcpyDeviceToHost, ctx->stream));
    BHR_HIP(hipStreamSynchronize(ctx->stream));
    if (meta[1]) return bhr_fail(BHR_ERR_STATE, "bhr_jpeg_encode_device: the encoded frame exceeds bhr_jpeg_device_bound");
    if ((int64_t)meta[0] > cap)
        return bhr_fail(BHR_ERR_INVALID, "bhr_jpeg_encode_device: %u bytes do not fit the caller's %lld", meta[0], (long long)cap);
    BHR_HIP(hipMemcpyAsync(out, d->d_out, meta[0], hipMemcpyDeviceToHost, ctx->stream));
    BHR_HIP(hipStreamSynchronize(ctx->stream));
    *out_len = (int64_t)meta[0];
    return BHR_OK;
}

}  // extern "C"
