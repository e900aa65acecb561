// ag_segment.hip — object masks from colour images: colour keys in integer HSV, square morphology, connected-component labelling with its
// component table, selection by area and hole filling, and the reference's keep rule ~(table & ~objects) (src/planning/perception.py:176-209:
// what it does with the masks its detection and segmentation models return).  The arithmetic is stated by adaptigraph_amd/segment.py in numpy
// integers and repeated here operation for operation; every result is an integer and equal to the statement's, bit for bit.
//
// Labelling (ag_segment_label), five launches whatever the image shows:
// (1) tile_kernel: one workgroup per kTileH x kTileW tile, one wave per row at a time.  A 64-bit ballot is the row; a pixel starts at the first
//     pixel of its run (the highest zero bit below it), so a run is one set already.  Runs of neighbouring rows are joined by a union-find in
//     LDS, one union per contact of two runs, then flattened; a pixel leaves with the image index of its tile component's lowest pixel.
// (2) merge_kernel: one thread per pixel of a tile's first row or first column joins it with its neighbours across the border, in global memory.
// (3) flatten_kernel: every pixel follows its chain to the root; the roots (pixels whose label is their own index) are counted per workgroup.
// (4) rank_kernel: the two-pass scan of ag_block_dev.h numbers the roots 1 .. count in ascending index order, per image.
// (5) relabel_kernel: a pixel takes its root's number.
// Union by minimum: a set's root is its lowest index, and a union hangs the higher root under the lower one with atomicMin.  Whatever the order
// of the unions, the root of a finished component is therefore its lowest row-major pixel: the labels do not depend on the order of execution.
//
// Coherence of (2).  Workgroups of one launch, on different XCDs, read and write the same label words.  Every such access is an agent-scope
// atomic: atomicMin for the union and a relaxed agent-scope atomic load for the find, neither served from an L1 or from another XCD's stale L2
// line.  A stale value would still be a correct ancestor (labels only decrease and a word only ever holds an ancestor of its pixel), but the loop
// that retries a union must see its own atomicMin's effect to end, so no plain load touches these words inside the launch.  Nothing waits for
// another workgroup: no flags, no tickets, no spinning; a union retries only while labels decrease, which they do finitely often.  The kernel
// boundary in front of (3) makes everything visible, so (3) to (5) use plain loads; (3) writes the roots to a second image, not in place.
#include "ag_block_dev.h"
#include "ag_host.h"

namespace {

constexpr int kBlock = 256;
constexpr int kTileH = AG_SEGMENT_TILE_H, kTileW = AG_SEGMENT_TILE_W;
constexpr int kRowsPerWave = kTileH / (kBlock / 64);
static_assert(kTileW == 64, "a tile row is one wave: its ballot is the row");
static_assert(kTileH % (kBlock / 64) == 0, "every wave takes the same number of rows");
static_assert(kBlock == kScanRows, "the root count is one scan row per thread");
constexpr int kMaxKeys = AG_SEGMENT_MAX_KEYS;
constexpr int kMaxKeep = AG_SEGMENT_MAX_KEEP;
constexpr long long kMaxPixels = 0x7fffffffLL - kBlock;      // H W of one image: every index, and the index of a thread past the end, is an int32

struct Keys {
    int32_t box[kMaxKeys][6];      // h_lo, h_hi, s_lo, s_hi, v_lo, v_hi
    int n;
};

// ---- colour keys ----
__device__ __forceinline__ int floor_div(int a, int b)      // b > 0; numpy's //, not C's /
{
    const int q = a / b;
    return (a % b < 0) ? q - 1 : q;
}
__device__ __forceinline__ int mod360(int a)
{
    const int m = a % 360;
    return m < 0 ? m + 360 : m;
}

__global__ __launch_bounds__(kBlock) void color_kernel(const uint8_t *__restrict__ images, int HW, int channels, Keys keys, uint8_t *__restrict__ mask)
{
    const int p = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    if (p >= HW) return;
    const size_t at = (size_t)blockIdx.y * (size_t)HW + (size_t)p;
    int r, g, b;
    if (channels == 4) {
        const uchar4 q = reinterpret_cast<const uchar4 *>(images)[at];
        r = q.x, g = q.y, b = q.z;
    } else {
        r = images[at * 3], g = images[at * 3 + 1], b = images[at * 3 + 2];
    }
    const int mx = max(r, max(g, b)), mn = min(r, min(g, b)), d = mx - mn;
    const int s = mx == 0 ? 0 : (255 * d + mx / 2) / mx;
    int h = 0;
    if (d != 0) {
        if (mx == r) h = mod360(floor_div(60 * (g - b) + d / 2, d));
        else if (mx == g) h = mod360(floor_div(60 * (b - r) + d / 2, d) + 120);
        else h = mod360(floor_div(60 * (r - g) + d / 2, d) + 240);
    }
    bool hit = false;
    for (int k = 0; k < keys.n; ++k) {
        const int32_t *q = keys.box[k];
        const bool hue = q[0] <= q[1] ? (h >= q[0] && h <= q[1]) : (h >= q[0] || h <= q[1]);
        hit = hit || (hue && s >= q[2] && s <= q[3] && mx >= q[4] && mx <= q[5]);
    }
    mask[at] = hit ? 1 : 0;
}

// ---- morphology: the (2r + 1) square as a row pass and a column pass; outside the image is background ----
__global__ __launch_bounds__(kBlock) void morph_kernel(const uint8_t *__restrict__ in, int H, int W, int r, int dilate, int column, uint8_t *__restrict__ out)
{
    const int HW = H * W, p = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    if (p >= HW) return;
    const size_t img = (size_t)blockIdx.y * (size_t)HW;
    const int y = p / W, x = p - y * W;
    const int at = column ? y : x, n = column ? H : W, step = column ? W : 1;
    bool v = !dilate;
    for (int k = -r; k <= r; ++k) {
        const bool inside = at + k >= 0 && at + k < n;
        const bool set = inside && in[img + (size_t)(p + k * step)] != 0;
        v = dilate ? (v || set) : (v && set);
    }
    out[img + p] = v ? 1 : 0;
}

// ---- the keep rule ----
__global__ __launch_bounds__(kBlock) void keep_rule_kernel(const uint8_t *__restrict__ table, const uint8_t *__restrict__ objects, int HW,
                                                          uint8_t *__restrict__ out)
{
    const int p = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    if (p >= HW) return;
    const size_t at = (size_t)blockIdx.y * (size_t)HW + (size_t)p;
    const bool t = table[at] != 0, o = objects != nullptr && objects[at] != 0;
    out[at] = !(t && !o) ? 1 : 0;
}

// ---- (1) tile-local components ----
__device__ __forceinline__ int lds_find(int *lab, int a)
{
    for (;;) {
        const int v = __hip_atomic_load(&lab[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (v == a) return a;
        a = v;
    }
}
__device__ __forceinline__ void lds_union(int *lab, int a, int b)
{
    for (;;) {
        a = lds_find(lab, a);
        b = lds_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }      // a > b: hang a under b
        const int old = atomicMin(&lab[a], b);
        if (old == a) return;
        a = old;      // a had a parent by then: join that one with b
    }
}

__global__ __launch_bounds__(kBlock) void tile_kernel(const uint8_t *__restrict__ mask, int H, int W, int conn8, int invert, int32_t *__restrict__ parent)
{
    __shared__ int s_lab[kTileH * kTileW];
    __shared__ unsigned long long s_row[kTileH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t img = (size_t)blockIdx.z * (size_t)H * (size_t)W;
    const int x = (int)blockIdx.x * kTileW + lane, y0 = (int)blockIdx.y * kTileH;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int i = 0; i < kRowsPerWave; ++i) {
        const int ly = wave * kRowsPerWave + i, y = y0 + ly;
        const bool fg = x < W && y < H && ((mask[img + (size_t)y * W + x] != 0) != (invert != 0));
        const unsigned long long row = __ballot(fg);
        if (lane == 0) s_row[ly] = row;
        const unsigned long long gaps = ~row & below;      // the background pixels in front of this one: the run starts behind the last
        const int start = gaps ? 64 - __clzll((long long)gaps) : 0;
        s_lab[ly * kTileW + lane] = fg ? ly * kTileW + start : -1;
    }
    __syncthreads();
    for (int i = 0; i < kRowsPerWave; ++i) {
        const int ly = wave * kRowsPerWave + i;
        if (ly == 0) continue;
        const unsigned long long cur = s_row[ly], up = s_row[ly - 1];
        if (!((cur >> lane) & 1ull)) continue;
        const bool u = (up >> lane) & 1ull, ul = lane > 0 && ((up >> (lane - 1)) & 1ull), ur = lane < 63 && ((up >> (lane + 1)) & 1ull);
        const bool l = lane > 0 && ((cur >> (lane - 1)) & 1ull), r = lane < 63 && ((cur >> (lane + 1)) & 1ull);
        const int a = ly * kTileW + lane;
        // one union per contact of two runs: the left neighbour, where it is set and touches the same run above, has made it already
        if (u && !(l && ul)) lds_union(s_lab, a, a - kTileW);
        if (conn8) {
            if (ul && !u && !l) lds_union(s_lab, a, a - kTileW - 1);
            if (ur && !u && !r) lds_union(s_lab, a, a - kTileW + 1);
        }
    }
    __syncthreads();
    for (int i = 0; i < kRowsPerWave; ++i) {
        const int ly = wave * kRowsPerWave + i, y = y0 + ly;
        if (x >= W || y >= H) continue;
        const int v = s_lab[ly * kTileW + lane];
        int out = -1;
        if (v >= 0) {
            const int root = lds_find(s_lab, v);      // a foreground pixel of this tile, so inside the image
            out = (y0 + root / kTileW) * W + (int)blockIdx.x * kTileW + root % kTileW;
        }
        parent[img + (size_t)y * W + x] = out;
    }
}

// ---- (2) unions across the tile borders: agent-scope atomics only ----
__device__ __forceinline__ int global_find(int32_t *lab, int a)
{
    for (;;) {
        const int v = __hip_atomic_load(&lab[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v == a) return a;
        a = v;
    }
}
__device__ __forceinline__ void global_union(int32_t *lab, int a, int b)
{
    for (;;) {
        a = global_find(lab, a);
        b = global_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&lab[a], b);
        if (old == a) return;
        a = old;
    }
}

__global__ __launch_bounds__(kBlock) void merge_kernel(const uint8_t *__restrict__ mask, int H, int W, int conn8, int invert, long long n_rows,
                                                      long long total, int32_t *__restrict__ parent)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const size_t img = (size_t)blockIdx.y * (size_t)H * (size_t)W;
    const uint8_t *m = mask + img;
    int32_t *lab = parent + img;
    const bool inv = invert != 0;
    auto set = [&](int yy, int xx) { return yy >= 0 && yy < H && xx >= 0 && xx < W && ((m[(size_t)yy * W + xx] != 0) != inv); };
    const bool first_row = i < n_rows * W;      // a pixel of a tile's first row, else of a tile's first column
    int x, y;
    if (first_row) {
        y = (int)(i / W + 1) * kTileH;
        x = (int)(i % W);
    } else {
        const long long j = i - n_rows * W;
        x = (int)(j / H + 1) * kTileW;
        y = (int)(j % H);
    }
    if (!set(y, x)) return;
    const int p = y * W + x;
    if (first_row) {
        const bool u = set(y - 1, x);
        if (u) global_union(lab, p, p - W);
        if (conn8 && !u) {      // (a set pixel above is the neighbour of both diagonals in its own row)
            if (set(y - 1, x - 1)) global_union(lab, p, p - W - 1);
            if (set(y - 1, x + 1)) global_union(lab, p, p - W + 1);
        }
    } else {
        const bool l = set(y, x - 1);
        if (l) global_union(lab, p, p - 1);
        if (conn8 && !l) {      // (a set pixel to the left is the neighbour of both diagonals in its own column)
            if (set(y - 1, x - 1) && !set(y - 1, x)) global_union(lab, p, p - W - 1);
            if (set(y + 1, x - 1) && !set(y + 1, x)) global_union(lab, p, p + W - 1);
        }
    }
}

// ---- (3) roots, and how many each workgroup holds ----
__global__ __launch_bounds__(kBlock) void flatten_kernel(const int32_t *__restrict__ parent, int HW, int blk_stride, int32_t *__restrict__ root,
                                                        int32_t *__restrict__ zeroed, int32_t *__restrict__ blk_sum)
{
    const int p = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    const size_t img = (size_t)blockIdx.y * (size_t)HW;
    int is_root = 0;
    if (p < HW) {
        const int32_t *lab = parent + img;
        int v = lab[p];
        if (v >= 0)
            for (int n = lab[v]; n != v; n = lab[v]) v = n;
        root[img + p] = v;
        if (zeroed) zeroed[img + p] = 0;
        is_root = v == p;
    }
    int total;
    block_exclusive_scan(is_root, &total);
    if (threadIdx.x == 0) blk_sum[(size_t)blockIdx.y * blk_stride + blockIdx.x] = total;
}

// ---- (4) the roots' numbers 1 .. count, in index order ----
__global__ __launch_bounds__(kBlock) void rank_kernel(const int32_t *__restrict__ root, int HW, int blk_stride, const int32_t *__restrict__ blk_sum,
                                                     int32_t *__restrict__ rank, int32_t *__restrict__ count)
{
    const int base = block_offset(blk_sum + (size_t)blockIdx.y * blk_stride);
    const int p = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    const size_t img = (size_t)blockIdx.y * (size_t)HW;
    const int is_root = p < HW && root[img + p] == p;
    int total;
    const int r = base + block_exclusive_scan(is_root, &total) + 1;
    if (is_root) rank[img + p] = r;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) count[blockIdx.y] = base + total;
}

// ---- (5) ----
__global__ __launch_bounds__(kBlock) void relabel_kernel(const int32_t *__restrict__ root, const int32_t *__restrict__ rank, int HW,
                                                        int32_t *__restrict__ labels)
{
    const int p = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    if (p >= HW) return;
    const size_t img = (size_t)blockIdx.y * (size_t)HW;
    const int r = root[img + p];
    labels[img + p] = r < 0 ? 0 : rank[img + r];
}

// ---- runs of equal values among the 64 consecutive pixels of a wave ----
// value: >= 0 a member, < 0 none.  Returns the length of the run that starts at this lane (the pixels behind it in the same image row with the
// same value, up to the wave's end), or 0 where no run starts.  Every lane of the wave must call it.
__device__ __forceinline__ int run_length(int value, int x, int lane)
{
    const int prev = __shfl_up(value, 1);
    const bool edge = lane == 0 || prev != value || x == 0;
    const unsigned long long edges = __ballot(edge);
    const unsigned long long rest = lane == 63 ? 0ull : edges & ~((2ull << lane) - 1ull);
    const int len = (rest ? __ffsll((long long)rest) - 1 : 64) - lane;
    return (edge && value >= 0) ? len : 0;
}

// ---- the component table ----
constexpr unsigned long long kBig = 0x7fffffffffffffffULL;

__global__ __launch_bounds__(kBlock) void table_init_kernel(const int32_t *__restrict__ count, int max_labels, int64_t *__restrict__ table)
{
    const int k = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    if (k >= max_labels) return;
    const bool live = k < count[blockIdx.y];
    int64_t *row = table + ((size_t)blockIdx.y * max_labels + k) * 8;
    for (int j = 0; j < 8; ++j) row[j] = (live && (j == 1 || j == 2)) ? (int64_t)kBig : 0;
}

__global__ __launch_bounds__(kBlock) void table_kernel(const int32_t *__restrict__ labels, const int32_t *__restrict__ count, int H, int W, int max_labels,
                                                      int64_t *__restrict__ table)
{
    const int HW = H * W, p = (int)blockIdx.x * kBlock + (int)threadIdx.x, lane = threadIdx.x & 63;
    const size_t img = (size_t)blockIdx.y * (size_t)HW;
    const int n = min(count[blockIdx.y], max_labels);
    const int l = p < HW ? labels[img + p] : 0;
    const int y = p < HW ? p / W : 0, x = p < HW ? p - y * W : 0;
    const int len = run_length((l >= 1 && l <= n) ? l : -1, x, lane);      // a run is one row's: its sums are closed forms
    if (len == 0) return;
    unsigned long long *row = reinterpret_cast<unsigned long long *>(table + ((size_t)blockIdx.y * max_labels + (l - 1)) * 8);
    const unsigned long long x0 = x, x1 = x + len - 1, n_ = len;
    atomicAdd(&row[0], n_);
    atomicMin(&row[1], x0);
    atomicMin(&row[2], (unsigned long long)y);
    atomicMax(&row[3], x1);
    atomicMax(&row[4], (unsigned long long)y);
    atomicAdd(&row[5], n_ * x0 + n_ * (n_ - 1) / 2);
    atomicAdd(&row[6], n_ * (unsigned long long)y);
    if (y == 0 || y == H - 1 || x == 0 || x + len - 1 == W - 1) atomicOr(&row[7], 1ull);
}

// ---- selection: areas at the root pixels, the k largest by key = area << 32 | ~root (equal areas: the lower root, the lower label) ----
__global__ __launch_bounds__(kBlock) void area_kernel(const int32_t *__restrict__ root, int HW, int W, int32_t *__restrict__ area)
{
    const int p = (int)blockIdx.x * kBlock + (int)threadIdx.x, lane = threadIdx.x & 63;
    const size_t img = (size_t)blockIdx.y * (size_t)HW;
    const int r = p < HW ? root[img + p] : -1;
    const int len = run_length(r, p < HW ? p % W : 0, lane);
    if (len) atomicAdd(&area[img + r], len);
}

__device__ __forceinline__ unsigned long long area_key(int area, int root) { return ((unsigned long long)(unsigned)area << 32) | (0xffffffffu - (unsigned)root); }
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v) { return ~block_min_u64(~v); }

__global__ __launch_bounds__(kBlock) void topk_block_kernel(const int32_t *__restrict__ root, const int32_t *__restrict__ area, int HW, int min_area, int k,
                                                           unsigned long long *__restrict__ cand)
{
    const int p = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    const size_t img = (size_t)blockIdx.y * (size_t)HW;
    unsigned long long key = 0;
    if (p < HW && root[img + p] == p && area[img + p] >= min_area) key = area_key(area[img + p], p);
    unsigned long long prev = ~0ull;
    unsigned long long *dst = cand + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kMaxKeep;
    for (int j = 0; j < k; ++j) {      // (keys are distinct: "below the last one" removes exactly it)
        prev = block_max_u64(key < prev ? key : 0ull);
        if (threadIdx.x == 0) dst[j] = prev;
    }
}

__global__ __launch_bounds__(kBlock) void topk_image_kernel(const unsigned long long *__restrict__ cand, int n_blk, int k, unsigned long long *__restrict__ thresh)
{
    const unsigned long long *src = cand + (size_t)blockIdx.x * n_blk * kMaxKeep;
    const long long n = (long long)n_blk * k;
    unsigned long long prev = ~0ull;
    for (int j = 0; j < k; ++j) {
        unsigned long long best = 0;
        for (long long i = threadIdx.x; i < n; i += kBlock) {
            const unsigned long long v = src[(i / k) * kMaxKeep + i % k];
            if (v < prev && v > best) best = v;
        }
        prev = block_max_u64(best);
    }
    if (threadIdx.x == 0) thresh[blockIdx.x] = prev;      // the k-th largest key, or 0 where fewer than k components qualify
}

__global__ __launch_bounds__(kBlock) void select_kernel(const int32_t *__restrict__ root, const int32_t *__restrict__ area, int HW, int min_area,
                                                       const unsigned long long *__restrict__ thresh, uint8_t *__restrict__ out)
{
    const int p = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    if (p >= HW) return;
    const size_t img = (size_t)blockIdx.y * (size_t)HW;
    const int r = root[img + p];
    bool keep = false;
    if (r >= 0) {
        const int a = area[img + r];
        keep = a >= min_area && (thresh == nullptr || area_key(a, r) >= thresh[blockIdx.y]);
    }
    out[img + p] = keep ? 1 : 0;
}

// ---- holes: the background components (root image of the inverted mask) that no pixel of the image border belongs to ----
__global__ __launch_bounds__(kBlock) void border_kernel(const int32_t *__restrict__ root, int H, int W, int32_t *__restrict__ open)
{
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x, w = W, h = H;
    if (i >= 2 * w + 2 * h) return;
    const size_t img = (size_t)blockIdx.y * (size_t)H * (size_t)W;
    int x, y;
    if (i < w) x = (int)i, y = 0;
    else if (i < 2 * w) x = (int)(i - w), y = H - 1;
    else if (i < 2 * w + h) x = 0, y = (int)(i - 2 * w);
    else x = W - 1, y = (int)(i - 2 * w - h);
    const int r = root[img + (size_t)y * W + x];
    if (r >= 0) atomicOr(&open[img + r], 1);
}

__global__ __launch_bounds__(kBlock) void fill_kernel(const uint8_t *__restrict__ mask, const int32_t *__restrict__ root, const int32_t *__restrict__ open,
                                                     int HW, uint8_t *__restrict__ out)
{
    const int p = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    if (p >= HW) return;
    const size_t img = (size_t)blockIdx.y * (size_t)HW;
    const int r = root[img + p];
    out[img + p] = (mask[img + p] != 0 || (r >= 0 && open[img + r] == 0)) ? 1 : 0;
}

// ---- host ----
struct Scratch {
    int32_t *parent, *root, *word, *blk_sum;      // word: the ranks, the areas or the open flags, by root pixel
    unsigned long long *cand, *thresh;
    uint8_t *tmp0, *tmp1;
    int n_blk, blk_stride;
};

size_t carve(Carver &c, int C, int H, int W, Scratch &s)
{
    const size_t HW = (size_t)H * W, n = (size_t)C * HW;
    s.n_blk = (int)((HW + kBlock - 1) / kBlock);
    s.blk_stride = (int)ag_scan_blocks(HW);
    s.parent = c.take<int32_t>(n);
    s.root = c.take<int32_t>(n);
    s.word = c.take<int32_t>(n);
    s.blk_sum = c.take<int32_t>((size_t)C * s.blk_stride);
    s.cand = c.take<unsigned long long>((size_t)C * s.n_blk * kMaxKeep);
    s.thresh = c.take<unsigned long long>((size_t)C);
    s.tmp0 = c.take<uint8_t>(n);
    s.tmp1 = c.take<uint8_t>(n);
    return align_up(c.off, 256);
}

bool bad_shape(int C, int H, int W)
{
    return C < 1 || C > 65535 || H < 1 || W < 1 || (long long)H * W > kMaxPixels || (H + kTileH - 1) / kTileH > 65535;
}

int check_call(const char *name, int C, int H, int W, const void *scratch, size_t scratch_bytes, bool needs_scratch)
{
    if (C < 1 || C > 65535) return ag_fail(AG_ERR_ARG, "%s: C = %d outside 1 .. 65535", name, C);
    if (H < 1 || W < 1) return ag_fail(AG_ERR_ARG, "%s: H = %d, W = %d, must be >= 1", name, H, W);
    if ((long long)H * W > kMaxPixels)
        return ag_fail(AG_ERR_ARG, "%s: H * W = %lld exceeds %lld: a pixel's index is an int32", name, (long long)H * W, kMaxPixels);
    if ((H + kTileH - 1) / kTileH > 65535) return ag_fail(AG_ERR_ARG, "%s: H = %d is more than 65535 tiles of %d rows", name, H, kTileH);
    if (needs_scratch) {
        if (!scratch) return ag_fail(AG_ERR_ARG, "%s: null scratch", name);
        const size_t need = ag_segment_scratch_bytes(C, H, W);
        if (scratch_bytes < need) return ag_fail(AG_ERR_WS, "%s: scratch of %zu bytes, %zu needed (ag_segment_scratch_bytes)", name, scratch_bytes, need);
    }
    return AG_OK;
}

// launches (1) to (3): the root image of `mask` (of its background with `invert`), s.word zeroed where `zero_word`
int roots(const uint8_t *mask, int C, int H, int W, int conn8, int invert, bool zero_word, const Scratch &s, hipStream_t st)
{
    const int HW = H * W;
    const dim3 tiles((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH), (unsigned)C), pixels((unsigned)s.n_blk, (unsigned)C);
    hipLaunchKernelGGL(tile_kernel, tiles, dim3(kBlock), 0, st, mask, H, W, conn8, invert, s.parent);
    AG_HIP(hipGetLastError());
    const long long n_rows = (H - 1) / kTileH, n_cols = (W - 1) / kTileW, total = n_rows * W + n_cols * H;
    if (total > 0) {      // (by the image's size alone)
        hipLaunchKernelGGL(merge_kernel, dim3((unsigned)((total + kBlock - 1) / kBlock), (unsigned)C), dim3(kBlock), 0, st, mask, H, W, conn8, invert, n_rows,
                           total, s.parent);
        AG_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(flatten_kernel, pixels, dim3(kBlock), 0, st, s.parent, HW, s.blk_stride, s.root, zero_word ? s.word : nullptr, s.blk_sum);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

}  // namespace

extern "C" {

void ag_segment_tile_sizes(int *tile_h, int *tile_w)
{
    if (tile_h) *tile_h = kTileH;
    if (tile_w) *tile_w = kTileW;
}

size_t ag_segment_scratch_bytes(int C, int H, int W)
{
    if (bad_shape(C, H, W)) return 0;
    Carver c(nullptr, 0);
    Scratch s;
    return carve(c, C, H, W, s);
}

int ag_segment_color_mask(const uint8_t *images, int C, int H, int W, int channels, const int32_t *keys, int n_keys, uint8_t *mask, ag_stream_t stream)
{
    if (!images || !mask || (!keys && n_keys > 0)) return ag_fail(AG_ERR_ARG, "ag_segment_color_mask: null argument");
    if (int rc = check_call("ag_segment_color_mask", C, H, W, nullptr, 0, false)) return rc;
    if (channels != 3 && channels != 4) return ag_fail(AG_ERR_ARG, "ag_segment_color_mask: channels = %d, must be 3 or 4", channels);
    if (n_keys < 0 || n_keys > kMaxKeys) return ag_fail(AG_ERR_ARG, "ag_segment_color_mask: %d keys outside 0 .. %d (AG_SEGMENT_MAX_KEYS)", n_keys, kMaxKeys);
    if (channels == 4 && (reinterpret_cast<uintptr_t>(images) & 3)) return ag_fail(AG_ERR_ARG, "ag_segment_color_mask: RGBA images must be 4-byte aligned");
    Keys k{};
    k.n = n_keys;
    for (int i = 0; i < n_keys; ++i)
        for (int j = 0; j < 6; ++j) k.box[i][j] = keys[i * 6 + j];
    hipLaunchKernelGGL(color_kernel, dim3((unsigned)((H * W + kBlock - 1) / kBlock), (unsigned)C), dim3(kBlock), 0, static_cast<hipStream_t>(stream), images,
                       H * W, channels, k, mask);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_segment_morph(const uint8_t *mask, int C, int H, int W, int op, int radius, void *scratch, size_t scratch_bytes, uint8_t *out, ag_stream_t stream)
{
    if (!mask || !out) return ag_fail(AG_ERR_ARG, "ag_segment_morph: null argument");
    if (int rc = check_call("ag_segment_morph", C, H, W, scratch, scratch_bytes, true)) return rc;
    if (op < AG_SEGMENT_ERODE || op > AG_SEGMENT_CLOSE) return ag_fail(AG_ERR_ARG, "ag_segment_morph: op %d is not one of AG_SEGMENT_ERODE .. _CLOSE", op);
    if (radius < 0 || radius > AG_SEGMENT_MAX_RADIUS)
        return ag_fail(AG_ERR_ARG, "ag_segment_morph: radius = %d outside 0 .. %d (AG_SEGMENT_MAX_RADIUS)", radius, AG_SEGMENT_MAX_RADIUS);
    Carver c(scratch, scratch_bytes);
    Scratch s;
    carve(c, C, H, W, s);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)s.n_blk, (unsigned)C);
    // erode / dilate: row pass, column pass; opening = erode, dilate; closing = dilate, erode.  `out` is written by the last pass only (it may be `mask`).
    const int first = (op == AG_SEGMENT_DILATE || op == AG_SEGMENT_CLOSE) ? 1 : 0, two = op >= AG_SEGMENT_OPEN;
    hipLaunchKernelGGL(morph_kernel, grid, dim3(kBlock), 0, st, mask, H, W, radius, first, 0, s.tmp0);
    AG_HIP(hipGetLastError());
    hipLaunchKernelGGL(morph_kernel, grid, dim3(kBlock), 0, st, s.tmp0, H, W, radius, first, 1, two ? s.tmp1 : out);
    AG_HIP(hipGetLastError());
    if (two) {
        hipLaunchKernelGGL(morph_kernel, grid, dim3(kBlock), 0, st, s.tmp1, H, W, radius, !first, 0, s.tmp0);
        AG_HIP(hipGetLastError());
        hipLaunchKernelGGL(morph_kernel, grid, dim3(kBlock), 0, st, s.tmp0, H, W, radius, !first, 1, out);
        AG_HIP(hipGetLastError());
    }
    return AG_OK;
}

int ag_segment_label(const uint8_t *mask, int C, int H, int W, int connectivity, void *scratch, size_t scratch_bytes, int32_t *labels, int32_t *count,
                     ag_stream_t stream)
{
    if (!mask || !labels || !count) return ag_fail(AG_ERR_ARG, "ag_segment_label: null argument");
    if (int rc = check_call("ag_segment_label", C, H, W, scratch, scratch_bytes, true)) return rc;
    if (connectivity != 4 && connectivity != 8) return ag_fail(AG_ERR_ARG, "ag_segment_label: connectivity = %d, must be 4 or 8", connectivity);
    Carver c(scratch, scratch_bytes);
    Scratch s;
    carve(c, C, H, W, s);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = roots(mask, C, H, W, connectivity == 8, 0, false, s, st)) return rc;
    const dim3 grid((unsigned)s.n_blk, (unsigned)C);
    hipLaunchKernelGGL(rank_kernel, grid, dim3(kBlock), 0, st, s.root, H * W, s.blk_stride, s.blk_sum, s.word, count);
    AG_HIP(hipGetLastError());
    hipLaunchKernelGGL(relabel_kernel, grid, dim3(kBlock), 0, st, s.root, s.word, H * W, labels);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_segment_components(const int32_t *labels, const int32_t *count, int C, int H, int W, int max_labels, int64_t *table, ag_stream_t stream)
{
    if (!labels || !count || !table) return ag_fail(AG_ERR_ARG, "ag_segment_components: null argument");
    if (int rc = check_call("ag_segment_components", C, H, W, nullptr, 0, false)) return rc;
    if (max_labels < 1) return ag_fail(AG_ERR_ARG, "ag_segment_components: max_labels = %d, must be >= 1", max_labels);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(table_init_kernel, dim3((unsigned)((max_labels + kBlock - 1) / kBlock), (unsigned)C), dim3(kBlock), 0, st, count, max_labels, table);
    AG_HIP(hipGetLastError());
    hipLaunchKernelGGL(table_kernel, dim3((unsigned)((H * W + kBlock - 1) / kBlock), (unsigned)C), dim3(kBlock), 0, st, labels, count, H, W, max_labels,
                       table);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_segment_select(const uint8_t *mask, int C, int H, int W, int connectivity, int min_area, int keep_largest, void *scratch, size_t scratch_bytes,
                      uint8_t *out, ag_stream_t stream)
{
    if (!mask || !out) return ag_fail(AG_ERR_ARG, "ag_segment_select: null argument");
    if (int rc = check_call("ag_segment_select", C, H, W, scratch, scratch_bytes, true)) return rc;
    if (connectivity != 4 && connectivity != 8) return ag_fail(AG_ERR_ARG, "ag_segment_select: connectivity = %d, must be 4 or 8", connectivity);
    if (keep_largest < 0 || keep_largest > kMaxKeep)
        return ag_fail(AG_ERR_ARG, "ag_segment_select: keep_largest = %d outside 0 (all) .. %d (AG_SEGMENT_MAX_KEEP)", keep_largest, kMaxKeep);
    Carver c(scratch, scratch_bytes);
    Scratch s;
    carve(c, C, H, W, s);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = roots(mask, C, H, W, connectivity == 8, 0, true, s, st)) return rc;
    const dim3 grid((unsigned)s.n_blk, (unsigned)C);
    hipLaunchKernelGGL(area_kernel, grid, dim3(kBlock), 0, st, s.root, H * W, W, s.word);
    AG_HIP(hipGetLastError());
    if (keep_largest > 0) {
        hipLaunchKernelGGL(topk_block_kernel, grid, dim3(kBlock), 0, st, s.root, s.word, H * W, min_area, keep_largest, s.cand);
        AG_HIP(hipGetLastError());
        hipLaunchKernelGGL(topk_image_kernel, dim3((unsigned)C), dim3(kBlock), 0, st, s.cand, s.n_blk, keep_largest, s.thresh);
        AG_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(select_kernel, grid, dim3(kBlock), 0, st, s.root, s.word, H * W, min_area, keep_largest > 0 ? s.thresh : nullptr, out);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_segment_fill_holes(const uint8_t *mask, int C, int H, int W, int connectivity, void *scratch, size_t scratch_bytes, uint8_t *out, ag_stream_t stream)
{
    if (!mask || !out) return ag_fail(AG_ERR_ARG, "ag_segment_fill_holes: null argument");
    if (int rc = check_call("ag_segment_fill_holes", C, H, W, scratch, scratch_bytes, true)) return rc;
    if (connectivity != 4 && connectivity != 8) return ag_fail(AG_ERR_ARG, "ag_segment_fill_holes: connectivity = %d, must be 4 or 8", connectivity);
    Carver c(scratch, scratch_bytes);
    Scratch s;
    carve(c, C, H, W, s);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = roots(mask, C, H, W, connectivity == 4, 1, true, s, st)) return rc;      // the background, under the dual connectivity
    hipLaunchKernelGGL(border_kernel, dim3((unsigned)((2 * (long long)W + 2 * (long long)H + kBlock - 1) / kBlock), (unsigned)C), dim3(kBlock), 0, st, s.root, H,
                       W, s.word);
    AG_HIP(hipGetLastError());
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)s.n_blk, (unsigned)C), dim3(kBlock), 0, st, mask, s.root, s.word, H * W, out);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_segment_keep(const uint8_t *table, const uint8_t *objects, int C, int H, int W, uint8_t *out, ag_stream_t stream)
{
    if (!table || !out) return ag_fail(AG_ERR_ARG, "ag_segment_keep: null argument");
    if (int rc = check_call("ag_segment_keep", C, H, W, nullptr, 0, false)) return rc;
    hipLaunchKernelGGL(keep_rule_kernel, dim3((unsigned)((H * W + kBlock - 1) / kBlock), (unsigned)C), dim3(kBlock), 0, static_cast<hipStream_t>(stream), table,
                       objects, H * W, out);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

}  // extern "C"
