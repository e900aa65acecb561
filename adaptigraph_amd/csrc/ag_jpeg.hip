// ag_jpeg.hip — baseline JPEG scans of device images (the frames ag_draw writes, or packed RGB): colour conversion, subsampling, forward DCT,
// quantisation, Huffman coding with restart intervals, byte stuffing and the RSTm markers, all on the device; the host adds the header and, for
// a video, the AVI container (adaptigraph_amd/jpeg.py).  It stands in for the cv2.imwrite(".jpg") / video merge the reference ends its records
// with (src/dynamics/rollout/graph.py:163-225, rollout.py:194-203, src/planning/plan.py:328-339).  The arithmetic is the host statement's
// (jpeg.py:jpeg_scan_host), integer operation for integer operation, so the bytes are the statement's.
//
// Five launches on the caller's stream, nothing read on the host, every scratch word that is read written earlier in the same call:
// (1) dct_kernel: one wave per 8 x 8 block (four blocks per workgroup), lane (y, x) one sample: colour (and the 2 x 2 chroma mean of 4:2:0),
//     the row pass and the column pass through LDS, quantisation, the coefficient stored as int16 at its zig-zag position.
// (2) code_kernel: one workgroup per restart segment (at most kMaxRestart MCUs = 96 blocks).  A wave takes a block at a time, lane k coefficient k:
//     a ballot of the non-zero lanes gives every coefficient its zero run, lane 0 codes the DC difference, lane 63 the EOB; the lanes' bit counts
//     are summed (pass one), the blocks' counts scanned over the workgroup (block_exclusive_scan), and in pass two every lane ORs its bits into
//     the segment's bit buffer in LDS (integer OR-atomics: exact in any order).  Thread 0 pads with 1-bits; the threads then count the 0xFF
//     bytes of a contiguous piece each, scan, and write the stuffed bytes and the marker into the segment's slot, and the segment's length.
// (3, 4) sum_kernel, offset_kernel: the two-pass scan of ag_block_dev.h over the segment lengths; frame f's first segment gives offsets[f].
// (5) gather_kernel: one wave per segment copies its slot to its place in the contiguous stream.
//
// Ranges.  DCT: |row sum| <= 23 168 * 128 < 2^22, |t| <= 2 897, |u| <= 23 168 * 2 897 < 2^27, + d / 2 <= 255 * 2^15: all int32 (jpeg.py's text).  A
// quantised coefficient is at most 1 020 in magnitude: category <= 10, a DC difference category <= 11.  A block is at most 22 + 63 * 26 = 1 660
// bits < 208 bytes = 52 words: the bit buffer is 52 words per block and every OR lands inside it (put32 checks the word all the same).
#include "ag_block_dev.h"
#include "ag_host.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxRestart = AG_JPEG_MAX_RESTART;
constexpr int kBlockWords = AG_JPEG_BLOCK_BYTES / 4;
constexpr int kMaxBlocks = kMaxRestart * 6;
constexpr int kWords = kMaxBlocks * kBlockWords;
static_assert(AG_JPEG_BLOCK_BYTES % 4 == 0 && 3 * AG_JPEG_BLOCK_BYTES * 8 >= 3 * (22 + 63 * 26) + 7,
              "the bits of a segment (three blocks at least) and its padding fit its blocks' words");
static_assert(kMaxBlocks <= kBlock, "one thread per block in the scan of the blocks' bit counts");

__constant__ int kDct[64] = {2896, 2896,  2896,  2896,  2896,  2896,  2896,  2896,  4017, 3406,  2276,  799,   -799,  -2276, -3406, -4017,
                             3784, 1567,  -1567, -3784, -3784, -1567, 1567,  3784,  3406, -799,  -4017, -2276, 2276,  4017,  799,   -3406,
                             2896, -2896, -2896, 2896,  2896,  -2896, -2896, 2896,  2276, -4017, 799,   3406,  -3406, -799,  4017,  -2276,
                             1567, -3784, 3784,  -1567, -1567, 3784,  -3784, 1567,  799,  -2276, 3406,  -4017, 4017,  -3406, 2276,  -799};
// ITU-T T.81 Annex K.1 (natural order): luminance, chrominance
__constant__ int kQuantBase[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// the zig-zag position of the coefficient with natural index i
__constant__ uint8_t kZigzagPos[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                       10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// ---- the Annex K.3 Huffman tables: (codes per length 1 .. 16, symbols in code order) -> (code << 8) | length by symbol, at compile time ----
struct HuffSpec {
    uint8_t bits[16];
    uint8_t vals[162];
};
struct HuffTable {
    uint32_t entry[256];
};
constexpr HuffTable make_table(const HuffSpec &s)
{
    HuffTable t{};
    uint32_t code = 0;
    int at = 0;
    for (int n = 1; n <= 16; ++n) {
        for (int i = 0; i < s.bits[n - 1]; ++i) {
            t.entry[s.vals[at]] = (code << 8) | (uint32_t)n;
            ++code;
            ++at;
        }
        code <<= 1;
    }
    return t;
}
constexpr HuffSpec kDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kAcLuma = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr HuffSpec kAcChroma = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
__constant__ HuffTable kDcTable[2] = {make_table(kDcLuma), make_table(kDcChroma)};
__constant__ HuffTable kAcTable[2] = {make_table(kAcLuma), make_table(kAcChroma)};

struct Geometry {
    int bpm, mcus_x, n_mcu, nseg;      // blocks per MCU, MCU columns, MCUs and segments per frame
    long long blocks, segments;        // of the whole call
    size_t slot;                       // bytes of a segment's slot
};

Geometry geometry(int F, int H, int W, int subsampling, int restart)
{
    Geometry g;
    const int side = subsampling == AG_JPEG_444 ? 8 : 16;
    g.bpm = subsampling == AG_JPEG_444 ? 3 : 6;
    g.mcus_x = (W + side - 1) / side;
    g.n_mcu = g.mcus_x * ((H + side - 1) / side);
    g.nseg = (g.n_mcu + restart - 1) / restart;
    g.blocks = (long long)F * g.n_mcu * g.bpm;
    g.segments = (long long)F * g.nseg;
    g.slot = (size_t)2 * AG_JPEG_BLOCK_BYTES * g.bpm * restart + 2;
    return g;
}

bool bad_shape(int F, int H, int W, int subsampling, int restart)
{
    return F < 1 || H < 1 || H > AG_RENDER_MAX_SIDE || W < 1 || W > AG_RENDER_MAX_SIDE || (subsampling != AG_JPEG_444 && subsampling != AG_JPEG_420) ||
           restart < 1 || restart > AG_JPEG_MAX_RESTART;
}

// ---- (1) colour, subsampling, DCT, quantisation ----
__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// component `comp` (0 Y, 1 Cb, 2 Cr) of the pixel (px, py) of frame f, the coordinates clamped to the image
__device__ __forceinline__ int sample(const uint8_t *__restrict__ images, int f, int H, int W, int channels, int px, int py, int comp)
{
    px = px < W ? px : W - 1;
    py = py < H ? py : H - 1;
    const size_t at = ((size_t)f * H + py) * W + px;
    int r, g, b;
    if (channels == 4) {
        const uint32_t p = reinterpret_cast<const uint32_t *>(images)[at];      // bytes R, G, B, A
        r = p & 0xff; g = (p >> 8) & 0xff; b = (p >> 16) & 0xff;
    } else {
        r = images[3 * at]; g = images[3 * at + 1]; b = images[3 * at + 2];
    }
    if (comp == 0) return clamp255((19595 * r + 38470 * g + 7471 * b + 32768) >> 16);
    if (comp == 1) return clamp255((-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32768) >> 16);
    return clamp255((32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32768) >> 16);
}

__global__ __launch_bounds__(kBlock) void dct_kernel(const uint8_t *__restrict__ images, int H, int W, int channels, int quality, int subsampling,
                                                     int mcus_x, int n_mcu, long long blocks, int16_t *__restrict__ coef)
{
    __shared__ int s_m[64], s_x[4][64], s_t[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, y = lane >> 3, x = lane & 7;
    if (tid < 64) s_m[tid] = kDct[tid];
    const long long blk = (long long)blockIdx.x * 4 + wave;
    const bool live = blk < blocks;
    const int bpm = subsampling == AG_JPEG_444 ? 3 : 6;
    const int j = (int)(blk % bpm);
    const long long mcu_all = blk / bpm;
    const int f = (int)(mcu_all / n_mcu), m = (int)(mcu_all % n_mcu), my = m / mcus_x, mx = m % mcus_x;
    const bool chroma = subsampling == AG_JPEG_444 ? j >= 1 : j >= 4;
    int v = 0;
    if (live) {
        if (subsampling == AG_JPEG_444) {
            v = sample(images, f, H, W, channels, mx * 8 + x, my * 8 + y, j);
        } else if (j < 4) {
            v = sample(images, f, H, W, channels, mx * 16 + (j & 1) * 8 + x, my * 16 + (j >> 1) * 8 + y, 0);
        } else {
            const int px = mx * 16 + 2 * x, py = my * 16 + 2 * y, comp = j - 3;
            v = (sample(images, f, H, W, channels, px, py, comp) + sample(images, f, H, W, channels, px + 1, py, comp) +
                 sample(images, f, H, W, channels, px, py + 1, comp) + sample(images, f, H, W, channels, px + 1, py + 1, comp) + 2) >> 2;
        }
    }
    s_x[wave][lane] = v - 128;
    __syncthreads();      // the samples and the matrix are in
    int t = 0;
#pragma unroll
    for (int n = 0; n < 8; ++n) t += s_m[x * 8 + n] * s_x[wave][y * 8 + n];      // t[y][k = x]
    s_t[wave][lane] = (t + 512) >> 10;
    __syncthreads();      // the row pass is in
    int u = 0;
#pragma unroll
    for (int n = 0; n < 8; ++n) u += s_m[y * 8 + n] * s_t[wave][n * 8 + x];      // u[j = y][k = x]
    if (!live) return;
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    int entry = (kQuantBase[chroma ? 1 : 0][lane] * scale + 50) / 100;
    entry = entry < 1 ? 1 : entry > 255 ? 255 : entry;
    const int d = entry << 16, a = u < 0 ? -u : u, q = (a + (d >> 1)) / d;
    coef[blk * 64 + kZigzagPos[lane]] = (int16_t)(u < 0 ? -q : q);
}

// ---- (2) one restart segment: Huffman coding, padding, stuffing, marker ----
__device__ __forceinline__ int bit_count(int v) { return v == 0 ? 0 : 32 - __clz(v < 0 ? -v : v); }

// ORs the n <= 32 bits of v (nothing above them) into the bit buffer at bit position p, most significant first
__device__ __forceinline__ void put32(uint32_t *buf, int p, uint32_t v, int n)
{
    const int w = p >> 5, off = p & 31;
    if (n <= 0 || w < 0 || w >= kWords) return;      // (word w + 1 exists: the buffer has kWords + 1)
    if (off + n <= 32) {
        atomicOr(&buf[w], v << (32 - off - n));
    } else {
        const int r = off + n - 32;
        atomicOr(&buf[w], v >> r);
        atomicOr(&buf[w + 1], v << (32 - r));
    }
}
__device__ __forceinline__ void put64(uint32_t *buf, int p, unsigned long long v, int n)
{
    if (n > 32) {
        put32(buf, p, (uint32_t)(v >> 32), n - 32);
        put32(buf, p + n - 32, (uint32_t)v, 32);
    } else {
        put32(buf, p, (uint32_t)v, n);
    }
}

// what lane k of the wave that codes block b emits: lane 0 the DC difference, lane k the non-zero coefficient k behind the ZRLs of its zero run,
// lane 63 the EOB if coefficient 63 is zero; -> the bits and their number (at most 59), 0 for nothing
__device__ __forceinline__ int lane_event(const int16_t *__restrict__ c, int b, int lane, int bpm, const uint32_t (*s_ac)[256], const uint32_t (*s_dc)[12],
                                          unsigned long long *bits)
{
    const int v = c[(size_t)b * 64 + lane];
    const unsigned long long mask = __ballot(v != 0);
    const int j = b % bpm;
    const int tb = (bpm == 3 ? j >= 1 : j >= 4) ? 1 : 0;
    *bits = 0;
    if (lane == 0) {
        const int pb = bpm == 3 ? b - 3 : j == 0 ? b - 3 : j < 4 ? b - 1 : b - 6;      // the block of the same component before
        const int diff = v - (pb >= 0 ? (int)c[(size_t)pb * 64] : 0);
        int size = bit_count(diff);
        size = size > 11 ? 11 : size;
        const uint32_t amp = (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << size) - 1u), e = s_dc[tb][size];
        *bits = ((unsigned long long)(e >> 8) << size) | amp;
        return (int)(e & 0xff) + size;
    }
    if (v != 0) {
        const unsigned long long below = mask & ((1ull << lane) - 1ull) & ~1ull;
        const int prev = below ? 63 - __clzll((long long)below) : 0, run = lane - prev - 1, nz = run >> 4;
        int size = bit_count(v);
        size = size > 10 ? 10 : size;
        const uint32_t amp = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u), e = s_ac[tb][((run & 15) << 4) | size], z = s_ac[tb][0xf0];
        const int zl = (int)(z & 0xff), n = (int)(e & 0xff) + size;
        unsigned long long zrl = 0;
        for (int i = 0; i < nz; ++i) zrl = (zrl << zl) | (z >> 8);
        *bits = (zrl << n) | ((unsigned long long)(e >> 8) << size) | amp;
        return nz * zl + n;
    }
    if (lane == 63) {
        const uint32_t e = s_ac[tb][0];
        *bits = e >> 8;
        return (int)(e & 0xff);
    }
    return 0;
}

__device__ __forceinline__ int wave_exclusive_scan(int v, int lane)
{
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    return x - v;
}

__global__ __launch_bounds__(kBlock) void code_kernel(const int16_t *__restrict__ coef, int bpm, int n_mcu, int nseg, int restart, size_t slot,
                                                      uint8_t *__restrict__ slots, int32_t *__restrict__ seg_len)
{
    __shared__ uint32_t s_bits[kWords + 1];
    __shared__ uint32_t s_ac[2][256], s_dc[2][12];
    __shared__ int s_len[kMaxBlocks], s_off[kMaxBlocks];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long g = blockIdx.x;
    const int f = (int)(g / nseg), s = (int)(g % nseg), mcu0 = s * restart;
    const int nb = (n_mcu - mcu0 < restart ? n_mcu - mcu0 : restart) * bpm;      // 1 .. kMaxBlocks blocks
    const int16_t *c = coef + ((size_t)f * n_mcu + mcu0) * bpm * 64;
    for (int i = tid; i < nb * kBlockWords + 1; i += kBlock) s_bits[i] = 0;
    s_ac[0][tid] = kAcTable[0].entry[tid];
    s_ac[1][tid] = kAcTable[1].entry[tid];
    if (tid < 24) s_dc[tid / 12][tid % 12] = kDcTable[tid / 12].entry[tid % 12];
    __syncthreads();      // the tables and a zeroed bit buffer
    unsigned long long bits;
    for (int b = wave; b < nb; b += kBlock / 64) {
        const int total = wave_sum(lane_event(c, b, lane, bpm, s_ac, s_dc, &bits));
        if (lane == 0) s_len[b] = total;
    }
    __syncthreads();      // the blocks' bit counts
    int seg_bits;
    const int off = block_exclusive_scan(tid < nb ? s_len[tid] : 0, &seg_bits);
    if (tid < nb) s_off[tid] = off;
    __syncthreads();      // the blocks' bit offsets
    for (int b = wave; b < nb; b += kBlock / 64) {
        const int n = lane_event(c, b, lane, bpm, s_ac, s_dc, &bits);
        put64(s_bits, s_off[b] + wave_exclusive_scan(n, lane), bits, n);
    }
    const int pad = (-seg_bits) & 7, n_bytes = (seg_bits + pad) >> 3;
    if (tid == 0) put32(s_bits, seg_bits, (1u << pad) - 1u, pad);
    __syncthreads();      // the segment's bytes
    // stuffing: thread t takes the bytes t piece .. (t + 1) piece - 1
    const int piece = (n_bytes + kBlock - 1) / kBlock, lo = tid * piece < n_bytes ? tid * piece : n_bytes,
              hi = lo + piece < n_bytes ? lo + piece : n_bytes;
    int ff = 0;
    for (int i = lo; i < hi; ++i) ff += ((s_bits[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu) == 0xffu;
    int ff_all;
    const int ff_before = block_exclusive_scan(ff, &ff_all);
    uint8_t *dst = slots + (size_t)g * slot;
    int at = lo + ff_before;
    for (int i = lo; i < hi; ++i) {
        const uint32_t byte = (s_bits[i >> 2] >> (24 - 8 * (i & 3))) & 0xffu;
        dst[at++] = (uint8_t)byte;
        if (byte == 0xffu) dst[at++] = 0;
    }
    if (tid == 0) {
        int n = n_bytes + ff_all;
        if (s + 1 < nseg) {
            dst[n] = 0xff;
            dst[n + 1] = (uint8_t)(0xd0 + (s & 7));
            n += 2;
        }
        seg_len[g] = n;
    }
}

// ---- (3, 4) the segments' offsets: the two-pass scan of ag_block_dev.h ----
__global__ __launch_bounds__(kScanRows) void sum_kernel(const int32_t *__restrict__ seg_len, long long segments, int32_t *__restrict__ blk_sum)
{
    const long long g = (long long)blockIdx.x * kScanRows + threadIdx.x;
    int total;
    block_exclusive_scan(g < segments ? seg_len[g] : 0, &total);
    if (threadIdx.x == 0) blk_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kScanRows) void offset_kernel(const int32_t *__restrict__ seg_len, long long segments, int nseg,
                                                          const int32_t *__restrict__ blk_sum, int32_t *__restrict__ seg_off,
                                                          int64_t *__restrict__ offsets)
{
    const int base = block_offset(blk_sum);
    const long long g = (long long)blockIdx.x * kScanRows + threadIdx.x;
    const int len = g < segments ? seg_len[g] : 0;
    int total;
    const int off = base + block_exclusive_scan(len, &total);
    if (g >= segments) return;
    seg_off[g] = off;
    if (g % nseg == 0) offsets[g / nseg] = off;
    if (g == segments - 1) offsets[segments / nseg] = (int64_t)off + len;
}

// ---- (5) the contiguous stream ----
__global__ __launch_bounds__(kBlock) void gather_kernel(const uint8_t *__restrict__ slots, size_t slot, const int32_t *__restrict__ seg_len,
                                                        const int32_t *__restrict__ seg_off, long long segments, uint8_t *__restrict__ out)
{
    const long long g = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (g >= segments) return;
    const uint8_t *src = slots + (size_t)g * slot;
    uint8_t *dst = out + seg_off[g];
    const int n = seg_len[g];
    for (int i = threadIdx.x & 63; i < n; i += 64) dst[i] = src[i];
}

struct Scratch {
    int16_t *coef;
    uint8_t *slots;
    int32_t *seg_len, *seg_off, *blk_sum;
};

size_t carve(Carver &c, const Geometry &g, Scratch &s)
{
    s.coef = c.take<int16_t>((size_t)g.blocks * 64);
    s.slots = c.take<uint8_t>((size_t)g.segments * g.slot);
    s.seg_len = c.take<int32_t>((size_t)g.segments);
    s.seg_off = c.take<int32_t>((size_t)g.segments);
    s.blk_sum = c.take<int32_t>(ag_scan_blocks((size_t)g.segments));
    return align_up(c.off, 256);
}

}  // namespace

extern "C" {

size_t ag_jpeg_out_bytes(int F, int H, int W, int subsampling, int restart)
{
    if (bad_shape(F, H, W, subsampling, restart)) return 0;
    const Geometry g = geometry(F, H, W, subsampling, restart);
    return (size_t)g.segments * g.slot;
}

size_t ag_jpeg_scratch_bytes(int F, int H, int W, int subsampling, int restart)
{
    if (bad_shape(F, H, W, subsampling, restart)) return 0;
    Carver c(nullptr, 0);
    Scratch s;
    return carve(c, geometry(F, H, W, subsampling, restart), s);
}

int ag_jpeg_encode(const uint8_t *images, int F, int H, int W, int channels, int quality, int subsampling, int restart, void *scratch,
                   size_t scratch_bytes, uint8_t *out, size_t out_bytes, int64_t *offsets, ag_stream_t stream)
{
    if (!images || !scratch || !out || !offsets) return ag_fail(AG_ERR_ARG, "ag_jpeg_encode: null argument");
    if (F < 1) return ag_fail(AG_ERR_ARG, "ag_jpeg_encode: F = %d, must be >= 1", F);
    if (H < 1 || H > AG_RENDER_MAX_SIDE || W < 1 || W > AG_RENDER_MAX_SIDE)
        return ag_fail(AG_ERR_ARG, "ag_jpeg_encode: H = %d, W = %d outside 1 .. %d (AG_RENDER_MAX_SIDE)", H, W, AG_RENDER_MAX_SIDE);
    if (channels != 3 && channels != 4) return ag_fail(AG_ERR_ARG, "ag_jpeg_encode: channels = %d, must be 3 or 4", channels);
    if (quality < 1 || quality > 100) return ag_fail(AG_ERR_ARG, "ag_jpeg_encode: quality = %d outside 1 .. 100", quality);
    if (subsampling != AG_JPEG_444 && subsampling != AG_JPEG_420)
        return ag_fail(AG_ERR_ARG, "ag_jpeg_encode: subsampling %d is neither AG_JPEG_444 nor AG_JPEG_420", subsampling);
    if (restart < 1 || restart > AG_JPEG_MAX_RESTART)
        return ag_fail(AG_ERR_ARG, "ag_jpeg_encode: restart = %d outside 1 .. %d (AG_JPEG_MAX_RESTART)", restart, AG_JPEG_MAX_RESTART);
    if (channels == 4 && (reinterpret_cast<uintptr_t>(images) & 3)) return ag_fail(AG_ERR_ARG, "ag_jpeg_encode: RGBA images must be 4-byte aligned");
    const Geometry g = geometry(F, H, W, subsampling, restart);
    const size_t need_out = ag_jpeg_out_bytes(F, H, W, subsampling, restart), need = ag_jpeg_scratch_bytes(F, H, W, subsampling, restart);
    if (need_out > 0x7fffffffULL || (g.blocks + 3) / 4 > 0x7fffffffLL)
        return ag_fail(AG_ERR_ARG, "ag_jpeg_encode: %d frames of %d x %d exceed one call (worst case %zu bytes; the offsets are 32-bit inside)", F, H, W,
                       need_out);
    if (scratch_bytes < need) return ag_fail(AG_ERR_ARG, "ag_jpeg_encode: scratch of %zu bytes, %zu needed (ag_jpeg_scratch_bytes)", scratch_bytes, need);
    if (out_bytes < need_out) return ag_fail(AG_ERR_ARG, "ag_jpeg_encode: out of %zu bytes, %zu needed (ag_jpeg_out_bytes)", out_bytes, need_out);
    Carver c(scratch, scratch_bytes);
    Scratch s;
    carve(c, g, s);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned scan_blocks = (unsigned)((g.segments + kScanRows - 1) / kScanRows);
    hipLaunchKernelGGL(dct_kernel, dim3((unsigned)((g.blocks + 3) / 4)), dim3(kBlock), 0, st, images, H, W, channels, quality, subsampling, g.mcus_x,
                       g.n_mcu, g.blocks, s.coef);
    AG_HIP(hipGetLastError());
    hipLaunchKernelGGL(code_kernel, dim3((unsigned)g.segments), dim3(kBlock), 0, st, s.coef, g.bpm, g.n_mcu, g.nseg, restart, g.slot, s.slots, s.seg_len);
    AG_HIP(hipGetLastError());
    hipLaunchKernelGGL(sum_kernel, dim3(scan_blocks), dim3(kScanRows), 0, st, s.seg_len, g.segments, s.blk_sum);
    AG_HIP(hipGetLastError());
    hipLaunchKernelGGL(offset_kernel, dim3(scan_blocks), dim3(kScanRows), 0, st, s.seg_len, g.segments, g.nseg, s.blk_sum, s.seg_off, offsets);
    AG_HIP(hipGetLastError());
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)((g.segments + 3) / 4)), dim3(kBlock), 0, st, s.slots, g.slot, s.seg_len, s.seg_off, g.segments, out);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

}  // extern "C"
