// ag_tabletop.hip — the tabletop cloud from depth images (src/planning/perception.py:151-256): un-project + board frame + crop, voxel merge,
// the statistical outlier filter's 20-nearest-neighbour mean, and the ordered compaction all of them end in.  The arithmetic is the host
// statement's (adaptigraph_amd/perception.py), operation for operation: float64 on float32 inputs, every product and sum rounded separately
// (the library is built with -ffp-contract=off).
//
// A cloud is (n_max, 3) fp32 rows plus a DEVICE count; launches are sized by n_max and every kernel reads the count.  No kernel waits on
// another workgroup, every loop is bounded by a size (never by a sentinel in the data), and every index read from memory is range-checked
// before it addresses anything.
//
// Ordered compaction (crop, voxel leaders, outlier filter, height filter): a stage writes one flag byte per item and the number of set flags
// per 256-item block (`sums`); compact_scatter_kernel then lets every block add up the sums in front of it (block_offset of ag_block_dev.h), ranks
// its own flags by ballot + popcount and copies the flagged rows — input order, no atomics; the last block writes the new count.
//
// Neighbour mean: the points are counting-sorted into a uniform grid (cell edge h from the bounding box and the count: about eight points per
// cell of a planar or a volumetric cloud, then refined twice from the number of OCCUPIED cells, at most nc_max cells).  One thread per point keeps its K best candidates under the total order (d2, j)
// in registers and widens its search ring by ring; a point lies inside its own cell, so every point outside ring r is farther than r h and the
// list is exact once its k-th distance is <= r h (taken with a 1e-6 margin against the rounding of the cell index), or once the rings cover the
// grid.  A point unresolved after kMaxRing rings is an isolated outlier: it goes onto a work list (a counter: the ORDER of that list decides
// nothing) and is finished by brute_kernel, one wave per point over the whole cloud.  Either way the selected set and the values are those of
// the O(n^2) scan.
#include "ag_block_dev.h"
#include "ag_host.h"

namespace {

constexpr int kBlock = 256;
constexpr int K = AG_TABLETOP_MAX_NEIGHBORS;
constexpr int kMaxRing = 3;
constexpr int kWide = 1024;             // the single-block kernels (bounds, cell scan, statistics)
constexpr int kBruteBlocks = 2048;
constexpr double kPerCell = 8.0;       // points per occupied cell the grid aims at
constexpr int kRefineRounds = 2;

typedef unsigned long long u64;

struct GridParams {
    double o[3], e[3], h;      // origin (the cloud's minimum), extents, cell edge
    int dim[3], ncell;
};

__device__ __forceinline__ int cloud_count(const int32_t *count, int n_max) { return max(0, min(*count, n_max)); }

// ------------------------------------------------------------------------------------------------------------------ ordered compaction
__device__ __forceinline__ void store_flag(bool in_range, bool f, int i, uint8_t *flags, int32_t *sums)
{
    if (in_range) flags[i] = f ? 1 : 0;
    const int c = __syncthreads_count(in_range && f);
    if (threadIdx.x == 0) sums[blockIdx.x] = c;
}

__global__ __launch_bounds__(kBlock) void flag_sums_kernel(const uint8_t *__restrict__ flags, const int32_t *__restrict__ count, int n_max,
                                                           int32_t *__restrict__ sums)
{
    const int i = blockIdx.x * kBlock + threadIdx.x, n = cloud_count(count, n_max);
    const int c = __syncthreads_count(i < n && flags[i] != 0);
    if (threadIdx.x == 0) sums[blockIdx.x] = c;
}

// progress (nullable): the new count, bit-complemented when it equals the old one (nothing removed)
__global__ __launch_bounds__(kBlock) void compact_scatter_kernel(const float *__restrict__ src, const uint8_t *__restrict__ flags,
                                                                 const int32_t *__restrict__ sums, const int32_t *__restrict__ count, int n_max,
                                                                 float *__restrict__ dst, int32_t *__restrict__ count_out,
                                                                 int32_t *__restrict__ progress)
{
    static_assert(kBlock == kScanRows, "sums holds one count per block of the two-pass scan");
    __shared__ int s_cnt[kBlock / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = block_offset(sums);
    const int n = cloud_count(count, n_max), i = b * kBlock + tid;
    const bool f = i < n && flags[i] != 0;
    const u64 bal = __ballot(f);
    if (lane == 0) s_cnt[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
        before += w < wave ? s_cnt[w] : 0;
        total += s_cnt[w];
    }
    if (f) {
        const size_t pos = (size_t)(base + before + ballot_rank(bal, lane));
        if (pos < (size_t)n_max) {
            dst[3 * pos] = src[3 * (size_t)i]; dst[3 * pos + 1] = src[3 * (size_t)i + 1]; dst[3 * pos + 2] = src[3 * (size_t)i + 2];
        }
    }
    if (b == (int)gridDim.x - 1 && tid == 0) {
        const int m = base + total;
        *count_out = m;
        if (progress) *progress = m == n ? ~m : m;
    }
}

// ------------------------------------------------------------------------------------------------------------------ depth images -> points
// cams (C, 21) doubles: Kinv, R (row-major), t.  limits: lo, hi, then the box as (axis, [min, max]).  tmp gets every strided pixel's point.
__global__ __launch_bounds__(kBlock) void depth_points_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ mask,
                                                              const double *__restrict__ cams, const double *__restrict__ limits, int C, int H, int W,
                                                              int stride, int Hs, int Ws, float *__restrict__ tmp, uint8_t *__restrict__ flags,
                                                              int32_t *__restrict__ sums, int32_t *__restrict__ n_items)
{
    const int t = blockIdx.x * kBlock + threadIdx.x, total = C * Hs * Ws;
    bool keep = false;
    if (t < total) {
        const int c = t / (Hs * Ws), r = t % (Hs * Ws), v = (r / Ws) * stride, u = (r % Ws) * stride;
        const size_t at = ((size_t)c * H + v) * W + u;
        const double d = (double)depth[at];
        const double *k = cams + 21 * (size_t)c, *R = k + 9, *tr = k + 18;
        const double a = (double)u * d, b = (double)v * d;
        double pc[3], p[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) pc[q] = (k[3 * q] * a + k[3 * q + 1] * b) + k[3 * q + 2] * d;
#pragma unroll
        for (int q = 0; q < 3; ++q) p[q] = ((R[3 * q] * pc[0] + R[3 * q + 1] * pc[1]) + R[3 * q + 2] * pc[2]) + tr[q];
        keep = d > limits[0] && d < limits[1] && (mask == nullptr || mask[at] != 0);
#pragma unroll
        for (int q = 0; q < 3; ++q) keep = keep && p[q] >= limits[2 + 2 * q] && p[q] <= limits[3 + 2 * q];      // (a NaN fails every comparison)
        tmp[3 * (size_t)t] = (float)p[0]; tmp[3 * (size_t)t + 1] = (float)p[1]; tmp[3 * (size_t)t + 2] = (float)p[2];
    }
    store_flag(t < total, keep, t, flags, sums);
    if (t == 0) *n_items = total;
}

// ------------------------------------------------------------------------------------------------------------------ bounds and the grid
// the largest grid of cell edge >= h that fits nc_max cells (h grows by a quarter per trip; a box no edge fits becomes one cell)
__device__ void fit_grid(GridParams *g, double h, int nc_max)
{
    const double e1 = fmax(g->e[0], fmax(g->e[1], g->e[2]));
    double d[3] = {1.0, 1.0, 1.0};
    bool fits = false;
    for (int it = 0; it < 256 && !fits; ++it) {
        for (int a = 0; a < 3; ++a) d[a] = floor(g->e[a] / h) + 1.0;
        fits = d[0] * d[1] * d[2] <= (double)nc_max;
        if (!fits) h *= 1.25;
    }
    if (!fits) { h = 2.0 * e1 + 1.0; d[0] = d[1] = d[2] = 1.0; }
    g->h = h;
    for (int a = 0; a < 3; ++a) g->dim[a] = (int)d[a];
    g->ncell = g->dim[0] * g->dim[1] * g->dim[2];
}

// first guess from the box and the count: about kPerCell points per cell if the cloud filled its box's largest face, or its volume
__device__ void choose_grid(const float *mn, const float *mx, int n, int nc_max, GridParams *g)
{
    double h = 1.0;
    for (int a = 0; a < 3; ++a) {
        g->o[a] = n > 0 ? (double)mn[a] : 0.0;
        g->e[a] = n > 0 ? (double)mx[a] - (double)mn[a] : 0.0;
        if (!(g->e[a] >= 0.0) || g->e[a] > 1e300) g->e[a] = 0.0;      // non-finite input: one cell along that axis, the brute-force pass does the rest
    }
    const double *e = g->e;
    const double e1 = fmax(e[0], fmax(e[1], e[2])), e3 = fmin(e[0], fmin(e[1], e[2])), e2 = fmax(0.0, (e[0] + e[1] + e[2]) - e1 - e3);
    if (n > 0) {
        const double per = kPerCell / (double)n;
        h = fmax(sqrt(per * e1 * e2), cbrt(per * e1 * e2 * e3));
        if (!(h > 0.0)) h = per * e1;
        if (!(h > 0.0)) h = 1.0;
    }
    fit_grid(g, h, nc_max);
}

// one workgroup: per-axis minimum and maximum of the cloud (exact in any order), and — nc_max > 0 — the neighbour grid
__global__ __launch_bounds__(kWide) void bounds_kernel(const float *__restrict__ pts, const int32_t *__restrict__ count, int n_max,
                                                       float *__restrict__ mn_out, int nc_max, GridParams *__restrict__ grid)
{
    __shared__ float s_mn[kWide / 64][3], s_mx[kWide / 64][3];
    const int tid = threadIdx.x, n = cloud_count(count, n_max);
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = tid; i < n; i += kWide)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = pts[3 * (size_t)i + a];
            mn[a] = fminf(mn[a], v); mx[a] = fmaxf(mx[a], v);
        }
#pragma unroll
    for (int a = 0; a < 3; ++a) { mn[a] = wave_fmin(mn[a]); mx[a] = wave_fmax(mx[a]); }
    if ((tid & 63) == 0)
        for (int a = 0; a < 3; ++a) { s_mn[tid >> 6][a] = mn[a]; s_mx[tid >> 6][a] = mx[a]; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kWide / 64; ++w)
            for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], s_mn[w][a]); mx[a] = fmaxf(mx[a], s_mx[w][a]); }
        for (int a = 0; a < 3; ++a) mn_out[a] = mn[a];
        if (nc_max > 0) choose_grid(mn, mx, n, nc_max, grid);
    }
}

__device__ __forceinline__ int cell_coord(double x, double o, double h, int dim)
{
    const double q = floor((x - o) / h);
    return q >= (double)(dim - 1) ? dim - 1 : (q > 0.0 ? (int)q : 0);      // (a NaN lands in cell 0)
}

__device__ __forceinline__ int cell_index(const GridParams &g, float x, float y, float z, int *cx, int *cy, int *cz)
{
    *cx = cell_coord((double)x, g.o[0], g.h, g.dim[0]);
    *cy = cell_coord((double)y, g.o[1], g.h, g.dim[1]);
    *cz = cell_coord((double)z, g.o[2], g.h, g.dim[2]);
    return (*cz * g.dim[1] + *cy) * g.dim[0] + *cx;
}

__global__ __launch_bounds__(kBlock) void cell_count_kernel(const float *__restrict__ pts, const int32_t *__restrict__ count, int n_max,
                                                            const GridParams *__restrict__ grid, int nc_max, int32_t *__restrict__ cell_count)
{
    const int i = blockIdx.x * kBlock + threadIdx.x, n = cloud_count(count, n_max);
    if (i >= n) return;
    const GridParams g = *grid;
    int cx, cy, cz;
    const int c = cell_index(g, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], &cx, &cy, &cz);
    if (c >= 0 && c < nc_max) atomicAdd(&cell_count[c], 1);
}

// one workgroup, after a count: a cloud that fills only a sheet or a curve of its box leaves most cells empty and crowds the others.  With more
// than 1.5 kPerCell points per OCCUPIED cell the edge shrinks as for a sheet (occupancy ~ h^2), as far as nc_max cells allow; the caller counts
// again.  The grid only decides speed: any h gives the same neighbours.
__global__ __launch_bounds__(kWide) void grid_refine_kernel(const int32_t *__restrict__ cell_count, const int32_t *__restrict__ count, int n_max,
                                                            int nc_max, GridParams *__restrict__ grid)
{
    __shared__ int s_occ[kWide / 64];
    const int tid = threadIdx.x, ncell = max(1, min(grid->ncell, nc_max));
    int occ = 0;
    for (int c = tid; c < ncell; c += kWide) occ += cell_count[c] > 0 ? 1 : 0;
    occ = wave_sum(occ);
    if ((tid & 63) == 0) s_occ[tid >> 6] = occ;
    __syncthreads();
    if (tid != 0) return;
    occ = 0;
    for (int w = 0; w < kWide / 64; ++w) occ += s_occ[w];
    const int n = cloud_count(count, n_max);
    if (occ < 1 || (double)n <= 1.5 * kPerCell * (double)occ) return;
    GridParams g = *grid;
    const double h_old = g.h;
    fit_grid(&g, h_old * sqrt(kPerCell * (double)occ / (double)n), nc_max);
    if (g.h < h_old) *grid = g;
}

// one workgroup: exclusive scan of the cell counts -> cell_start[0 .. ncell], every thread a contiguous run of cells
__global__ __launch_bounds__(kWide) void cell_scan_kernel(const int32_t *__restrict__ cell_count, const GridParams *__restrict__ grid, int nc_max,
                                                          int32_t *__restrict__ cell_start)
{
    __shared__ int s_run[kWide];
    const int tid = threadIdx.x, ncell = max(1, min(grid->ncell, nc_max));
    const int per = (ncell + kWide - 1) / kWide, c0 = min(tid * per, ncell), c1 = min(c0 + per, ncell);
    int run = 0;
    for (int c = c0; c < c1; ++c) run += cell_count[c];
    s_run[tid] = run;
    __syncthreads();
    for (int off = 1; off < kWide; off <<= 1) {      // inclusive scan of the runs
        const int v = tid >= off ? s_run[tid - off] : 0;
        __syncthreads();
        s_run[tid] += v;
        __syncthreads();
    }
    int at = s_run[tid] - run;
    for (int c = c0; c < c1; ++c) { cell_start[c] = at; at += cell_count[c]; }
    if (tid == kWide - 1) cell_start[ncell] = s_run[tid];
}

// slots inside a cell are handed out by a counter: their order decides nothing (selection is by the total order (d2, j))
__global__ __launch_bounds__(kBlock) void cell_fill_kernel(const float *__restrict__ pts, const int32_t *__restrict__ count, int n_max,
                                                           const GridParams *__restrict__ grid, int nc_max, const int32_t *__restrict__ cell_start,
                                                           int32_t *__restrict__ cell_count, float4 *__restrict__ sorted)
{
    const int i = blockIdx.x * kBlock + threadIdx.x, n = cloud_count(count, n_max);
    if (i >= n) return;
    const GridParams g = *grid;
    const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    int cx, cy, cz;
    const int c = cell_index(g, x, y, z, &cx, &cy, &cz);
    if (c < 0 || c >= nc_max) return;
    const int slot = cell_start[c] + atomicSub(&cell_count[c], 1) - 1;
    if (slot >= 0 && slot < n) sorted[slot] = make_float4(x, y, z, __int_as_float(i));
}

// ------------------------------------------------------------------------------------------------------------------ the K best candidates
__device__ __forceinline__ bool before(double a, int ja, double b, int jb) { return a < b || (a == b && ja < jb); }

struct Best {
    double d[K];
    int j[K];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int s = 0; s < K; ++s) { d[s] = INFINITY; j[s] = 0x7fffffff; }
    }
    __device__ __forceinline__ void offer(double v, int jj)
    {
        if (!before(v, jj, d[K - 1], j[K - 1])) return;
        d[K - 1] = v; j[K - 1] = jj;
#pragma unroll
        for (int s = K - 1; s > 0; --s) {
            const bool sw = before(d[s], j[s], d[s - 1], j[s - 1]);
            const double td = d[s];
            const int tj = j[s];
            d[s] = sw ? d[s - 1] : td; j[s] = sw ? j[s - 1] : tj;
            d[s - 1] = sw ? td : d[s - 1]; j[s - 1] = sw ? tj : j[s - 1];
        }
    }
    __device__ __forceinline__ double kth(int k) const
    {
        double v = INFINITY;
#pragma unroll
        for (int s = 0; s < K; ++s) v = s == k - 1 ? d[s] : v;
        return v;
    }
    __device__ __forceinline__ double mean_root(int k) const      // sum of the roots in ascending neighbour order, / k
    {
        double sum = 0.0;
#pragma unroll
        for (int s = 0; s < K; ++s)
            if (s < k) sum = sum + sqrt(d[s]);
        return sum / (double)k;
    }
};

__device__ __forceinline__ double dist2(double qx, double qy, double qz, float x, float y, float z)
{
    const double dx = qx - (double)x, dy = qy - (double)y, dz = qz - (double)z;
    return (dx * dx + dy * dy) + dz * dz;
}

// candidates of the slot range [s0, s1): four loads in flight per trip
__device__ __forceinline__ void scan_slots(const float4 *__restrict__ sorted, int s0, int s1, int n, double qx, double qy, double qz, Best &best)
{
    s0 = max(s0, 0); s1 = min(s1, n);
    for (int s = s0; s < s1; s += 4) {
        float4 c[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) c[e] = sorted[min(s + e, s1 - 1)];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (s + e < s1) best.offer(dist2(qx, qy, qz, c[e].x, c[e].y, c[e].z), __float_as_int(c[e].w));
    }
}

__global__ __launch_bounds__(kBlock) void knn_grid_kernel(const float4 *__restrict__ sorted, const int32_t *__restrict__ count, int n_max,
                                                          const GridParams *__restrict__ grid, int nc_max, const int32_t *__restrict__ cell_start,
                                                          int k_want, double *__restrict__ avg, int32_t *__restrict__ work,
                                                          int32_t *__restrict__ n_work)
{
    const int t = blockIdx.x * kBlock + threadIdx.x, n = cloud_count(count, n_max);
    if (t >= n) return;
    const GridParams g = *grid;
    if (g.ncell < 1 || g.ncell > nc_max) return;
    const int k = min(k_want, n);
    const float4 me = sorted[t];
    const int qi = __float_as_int(me.w);
    if (qi < 0 || qi >= n) return;
    const double qx = (double)me.x, qy = (double)me.y, qz = (double)me.z;
    int cx, cy, cz;
    cell_index(g, me.x, me.y, me.z, &cx, &cy, &cz);
    Best best;
    best.clear();
    bool done = false;
    for (int r = 0; r <= kMaxRing && !done; ++r) {
        for (int dz = -r; dz <= r; ++dz) {
            const int z = cz + dz;
            if (z < 0 || z >= g.dim[2]) continue;
            for (int dy = -r; dy <= r; ++dy) {
                const int y = cy + dy;
                if (y < 0 || y >= g.dim[1]) continue;
                const int row = (z * g.dim[1] + y) * g.dim[0];
                if (abs(dz) == r || abs(dy) == r) {      // a row of the shell: its cells are one run of slots
                    const int x0 = max(cx - r, 0), x1 = min(cx + r, g.dim[0] - 1);
                    scan_slots(sorted, cell_start[row + x0], cell_start[row + x1 + 1], n, qx, qy, qz, best);
                } else {                                  // an inner row: the shell's two end cells
                    if (cx - r >= 0) scan_slots(sorted, cell_start[row + cx - r], cell_start[row + cx - r + 1], n, qx, qy, qz, best);
                    if (cx + r < g.dim[0]) scan_slots(sorted, cell_start[row + cx + r], cell_start[row + cx + r + 1], n, qx, qy, qz, best);
                }
            }
        }
        const bool covers = cx - r <= 0 && cx + r >= g.dim[0] - 1 && cy - r <= 0 && cy + r >= g.dim[1] - 1 && cz - r <= 0 && cz + r >= g.dim[2] - 1;
        const double lim = (double)r * g.h * (1.0 - 1e-6);
        done = covers || best.kth(k) <= lim * lim;
    }
    if (done) avg[qi] = best.mean_root(k);
    else {
        const int at = atomicAdd(n_work, 1);
        if (at >= 0 && at < n_max) work[at] = qi;
    }
}

// one wave per listed point over the whole cloud: every lane keeps the K best of its share, then k rounds of a wave-wide minimum over the
// lanes' list heads (their lists sit in LDS so that a head can be addressed) give the neighbours in ascending order
__global__ __launch_bounds__(64) void brute_kernel(const float *__restrict__ pts, const int32_t *__restrict__ count, int n_max, int k_want,
                                                   const int32_t *__restrict__ work, const int32_t *__restrict__ n_work,
                                                   const GridParams *__restrict__ grid, double *__restrict__ avg, int32_t *__restrict__ info)
{
    __shared__ double s_d[K * 64];
    __shared__ int s_j[K * 64];
    const int lane = threadIdx.x, n = cloud_count(count, n_max), k = min(k_want, n), items = max(0, min(*n_work, n));
    if (blockIdx.x == 0 && lane == 0) { info[0] = items; info[1] = grid->ncell; }
    for (int w = blockIdx.x; w < items; w += gridDim.x) {
        const int qi = work[w];
        if (qi < 0 || qi >= n) continue;
        const double qx = (double)pts[3 * (size_t)qi], qy = (double)pts[3 * (size_t)qi + 1], qz = (double)pts[3 * (size_t)qi + 2];
        Best best;
        best.clear();
        for (int j0 = lane; j0 < n; j0 += 4 * 64) {
            float c[4][3];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const size_t j = (size_t)min(j0 + 64 * e, n - 1);
                c[e][0] = pts[3 * j]; c[e][1] = pts[3 * j + 1]; c[e][2] = pts[3 * j + 2];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j0 + 64 * e < n) best.offer(dist2(qx, qy, qz, c[e][0], c[e][1], c[e][2]), j0 + 64 * e);
        }
#pragma unroll
        for (int s = 0; s < K; ++s) { s_d[s * 64 + lane] = best.d[s]; s_j[s * 64 + lane] = best.j[s]; }
        int head = 0;
        double sum = 0.0;
        for (int r = 0; r < k; ++r) {
            const double hd = head < K ? s_d[head * 64 + lane] : INFINITY;
            const int hj = head < K ? s_j[head * 64 + lane] : 0x7fffffff;
            double md = hd;
            int mj = hj;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const double od = __shfl_xor(md, m);
                const int oj = __shfl_xor(mj, m);
                if (before(od, oj, md, mj)) { md = od; mj = oj; }
            }
            if (hd == md && hj == mj && mj != 0x7fffffff) ++head;      // point indices are unique: one lane
            sum = sum + sqrt(md);
        }
        if (lane == 0) avg[qi] = sum / (double)k;
    }
}

// ------------------------------------------------------------------------------------------------------------------ the outlier statistics
__device__ double block_sum_fixed(double v, double *s)      // a fixed tree over the kWide partial sums
{
    const int tid = threadIdx.x;
    __syncthreads();
    s[tid] = v;
    __syncthreads();
    for (int half = kWide / 2; half >= 1; half >>= 1) {
        if (tid < half) s[tid] = s[tid] + s[tid + half];
        __syncthreads();
    }
    return s[0];
}

// one workgroup: stats = [mean, std, threshold]; thread t sums items t, t + kWide, ... in ascending order
__global__ __launch_bounds__(kWide) void outlier_stats_kernel(const double *__restrict__ avg, const int32_t *__restrict__ count, int n_max,
                                                              double std_ratio, double *__restrict__ stats)
{
    __shared__ double s[kWide];
    const int tid = threadIdx.x, n = cloud_count(count, n_max);
    double part = 0.0;
    for (int i = tid; i < n; i += kWide) {
        const double a = avg[i];
        if (a > 0.0) part = part + a;
    }
    const double total = block_sum_fixed(part, s);
    const double mean = n > 0 ? total / (double)n : 0.0;
    part = 0.0;
    for (int i = tid; i < n; i += kWide) {
        const double a = avg[i];
        if (a > 0.0) part = part + (a - mean) * (a - mean);
    }
    const double sq = block_sum_fixed(part, s);
    if (tid == 0) {
        const double sd = n > 1 ? sqrt(sq / (double)(n - 1)) : 0.0;
        stats[0] = mean; stats[1] = sd; stats[2] = mean + std_ratio * sd;
    }
}

__global__ __launch_bounds__(kBlock) void outlier_flag_kernel(const double *__restrict__ avg, const int32_t *__restrict__ count, int n_max,
                                                              const double *__restrict__ stats, uint8_t *__restrict__ flags,
                                                              uint8_t *__restrict__ keep, int32_t *__restrict__ sums)
{
    const int i = blockIdx.x * kBlock + threadIdx.x, n = cloud_count(count, n_max);
    bool f = false;
    if (i < n && n > 1) {
        const double a = avg[i];
        f = a > 0.0 && a < stats[2];
    }
    if (i < n_max) keep[i] = f ? 1 : 0;
    store_flag(i < n_max, f, i, flags, sums);
}

__global__ __launch_bounds__(kBlock) void below_flag_kernel(const float *__restrict__ pts, const int32_t *__restrict__ count, int n_max,
                                                            const float *__restrict__ z_below, uint8_t *__restrict__ flags, int32_t *__restrict__ sums)
{
    const int i = blockIdx.x * kBlock + threadIdx.x, n = cloud_count(count, n_max);
    store_flag(i < n_max, i < n && pts[3 * (size_t)i + 2] < *z_below, i, flags, sums);
}

// ------------------------------------------------------------------------------------------------------------------ voxel merge
__global__ __launch_bounds__(kBlock) void voxel_key_kernel(const float *__restrict__ pts, const int32_t *__restrict__ count, int n_max,
                                                           const float *__restrict__ mn, double voxel, int64_t *__restrict__ keys,
                                                           int32_t *__restrict__ status)
{
    const int i = blockIdx.x * kBlock + threadIdx.x, n = cloud_count(count, n_max);
    if (i >= n_max) return;
    if (i >= n) { keys[i] = INT64_MAX; return; }      // behind every real key
    int64_t key = 0;
    bool wide = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double origin = (double)mn[a] - 0.5 * voxel;
        const double q = floor(((double)pts[3 * (size_t)i + a] - origin) / voxel);
        const bool ok = q >= 0.0 && q < (double)AG_TABLETOP_VOXEL_KEY_LIMIT;
        wide = wide || !ok;
        key = key * AG_TABLETOP_VOXEL_KEY_LIMIT + (ok ? (int64_t)q : 0);
    }
    keys[i] = key;
    if (wide) *status = 1;
}

// position j of the stably sorted keys: the first of a run is the voxel's lowest member (its leader), the run its members in ascending index
__global__ __launch_bounds__(kBlock) void voxel_mean_kernel(const float *__restrict__ pts, const int32_t *__restrict__ count, int n_max,
                                                            const int64_t *__restrict__ skeys, const int64_t *__restrict__ perm,
                                                            float *__restrict__ tmp, uint8_t *__restrict__ flags)
{
    const int j = blockIdx.x * kBlock + threadIdx.x, n = cloud_count(count, n_max);
    if (j >= n) return;
    const int64_t key = skeys[j], lead = perm[j];
    if (lead < 0 || lead >= n) return;
    const bool head = j == 0 || skeys[j - 1] != key;
    flags[lead] = head ? 1 : 0;
    if (!head) return;
    double sum[3] = {0.0, 0.0, 0.0};
    int members = 0;
    for (int e = j; e < n && skeys[e] == key; ++e) {
        const int64_t m = perm[e];
        if (m < 0 || m >= n) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a) sum[a] = sum[a] + (double)pts[3 * (size_t)m + a];
        ++members;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) tmp[3 * (size_t)lead + a] = (float)(sum[a] / (double)members);
}

// ------------------------------------------------------------------------------------------------------------------ workspace
int nc_max_for(int n_max)
{
    int nc = 64;      // room for a sheet in a box: four cells per point, a power of two in 64 .. 2^20
    while (nc < 4 * (long long)n_max && nc < (1 << 20)) nc *= 2;
    return nc;
}

struct Scratch {
    uint8_t *flags;
    int32_t *sums, *cell_count, *cell_start, *work, *words;      // words: [n_items, n_work]
    float *tmp, *mn;
    float4 *sorted;
    GridParams *grid;
    int nc_max, blocks;
};

size_t carve(void *ws, size_t bytes, int n_max, Scratch *s)
{
    Carver c(ws, bytes);
    const size_t n = (size_t)n_max;
    s->nc_max = nc_max_for(n_max);
    s->blocks = (n_max + kBlock - 1) / kBlock;
    s->flags = c.take<uint8_t>(n);
    s->sums = c.take<int32_t>((size_t)s->blocks + 1);
    s->tmp = c.take<float>(3 * n);
    s->mn = c.take<float>(4);
    s->grid = c.take<GridParams>(1);
    s->cell_count = c.take<int32_t>((size_t)s->nc_max + 1);
    s->cell_start = c.take<int32_t>((size_t)s->nc_max + 1);
    s->sorted = c.take<float4>(n);
    s->work = c.take<int32_t>(n);
    s->words = c.take<int32_t>(4);
    return align_up(c.off, 256);
}

int cloud_args(const char *who, bool have_all, int n_max, void *ws, size_t ws_bytes, Scratch *s)
{
    if (!have_all) return ag_fail(AG_ERR_ARG, "%s: null argument", who);
    if (n_max < 1 || n_max > AG_TABLETOP_MAX_POINTS)
        return ag_fail(AG_ERR_ARG, "%s: n_max = %d outside 1 .. %d (AG_TABLETOP_MAX_POINTS)", who, n_max, AG_TABLETOP_MAX_POINTS);
    const size_t need = carve(nullptr, 0, n_max, s);
    if (!ws || ws_bytes < need)
        return ag_fail(AG_ERR_WS, "%s: workspace of %zu bytes, ag_tabletop_workspace_bytes(%d) = %zu", who, ws ? ws_bytes : (size_t)0, n_max, need);
    carve(ws, ws_bytes, n_max, s);
    return AG_OK;
}

void launch_scatter(const Scratch &s, const float *src, const uint8_t *flags, const int32_t *count, int n_max, float *dst, int32_t *count_out,
                    int32_t *progress, hipStream_t st)
{
    hipLaunchKernelGGL(compact_scatter_kernel, dim3(s.blocks), dim3(kBlock), 0, st, src, flags, s.sums, count, n_max, dst, count_out, progress);
}

}  // namespace

extern "C" {

size_t ag_tabletop_workspace_bytes(int n_max)
{
    if (n_max < 1 || n_max > AG_TABLETOP_MAX_POINTS) return 0;
    Scratch s;
    return carve(nullptr, 0, n_max, &s);
}

int ag_depth_cloud(const float *depth, const uint8_t *mask, const double *cams, const double *limits, int C, int H, int W, int stride, float *pts,
                   int32_t *count, void *workspace, size_t workspace_bytes, ag_stream_t stream)
{
    if (C < 1 || H < 1 || W < 1 || stride < 1) return ag_fail(AG_ERR_ARG, "ag_depth_cloud: bad sizes C=%d H=%d W=%d stride=%d", C, H, W, stride);
    const int Hs = (H + stride - 1) / stride, Ws = (W + stride - 1) / stride;
    const long long total = (long long)C * Hs * Ws;
    if (total > AG_TABLETOP_MAX_POINTS)
        return ag_fail(AG_ERR_ARG, "ag_depth_cloud: %lld strided pixels exceed AG_TABLETOP_MAX_POINTS = %d", total, AG_TABLETOP_MAX_POINTS);
    Scratch s;
    if (int rc = cloud_args("ag_depth_cloud", depth && cams && limits && pts && count, (int)total, workspace, workspace_bytes, &s)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(depth_points_kernel, dim3(s.blocks), dim3(kBlock), 0, st, depth, mask, cams, limits, C, H, W, stride, Hs, Ws, s.tmp, s.flags,
                       s.sums, s.words);
    launch_scatter(s, s.tmp, s.flags, s.words, (int)total, pts, count, nullptr, st);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_cloud_voxel_keys(const float *pts, const int32_t *count, int n_max, const double *voxel_size, int64_t *keys, int32_t *status,
                        void *workspace, size_t workspace_bytes, ag_stream_t stream)
{
    Scratch s;
    if (int rc = cloud_args("ag_cloud_voxel_keys", pts && count && voxel_size && keys && status, n_max, workspace, workspace_bytes, &s)) return rc;
    const double voxel = *voxel_size;
    if (!(voxel > 0.0) || voxel > 1e300) return ag_fail(AG_ERR_ARG, "ag_cloud_voxel_keys: voxel_size = %g", voxel);
    hipStream_t st = static_cast<hipStream_t>(stream);
    ag_launch_zero_words(status, 1, st);
    hipLaunchKernelGGL(bounds_kernel, dim3(1), dim3(kWide), 0, st, pts, count, n_max, s.mn, 0, s.grid);
    hipLaunchKernelGGL(voxel_key_kernel, dim3(s.blocks), dim3(kBlock), 0, st, pts, count, n_max, s.mn, voxel, keys, status);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_cloud_voxel_merge(const float *pts, const int32_t *count, int n_max, const int64_t *sorted_keys, const int64_t *perm, float *out,
                         int32_t *count_out, void *workspace, size_t workspace_bytes, ag_stream_t stream)
{
    Scratch s;
    if (int rc = cloud_args("ag_cloud_voxel_merge", pts && count && sorted_keys && perm && out && count_out, n_max, workspace, workspace_bytes, &s))
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(voxel_mean_kernel, dim3(s.blocks), dim3(kBlock), 0, st, pts, count, n_max, sorted_keys, perm, s.tmp, s.flags);
    hipLaunchKernelGGL(flag_sums_kernel, dim3(s.blocks), dim3(kBlock), 0, st, s.flags, count, n_max, s.sums);
    launch_scatter(s, s.tmp, s.flags, count, n_max, out, count_out, nullptr, st);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_cloud_knn_mean(const float *pts, const int32_t *count, int n_max, int k, double *avg, int32_t *info, void *workspace,
                      size_t workspace_bytes, ag_stream_t stream)
{
    Scratch s;
    if (int rc = cloud_args("ag_cloud_knn_mean", pts && count && avg && info, n_max, workspace, workspace_bytes, &s)) return rc;
    if (k < 1 || k > AG_TABLETOP_MAX_NEIGHBORS)
        return ag_fail(AG_ERR_ARG, "ag_cloud_knn_mean: k = %d outside 1 .. %d (AG_TABLETOP_MAX_NEIGHBORS)", k, AG_TABLETOP_MAX_NEIGHBORS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    ag_launch_zero_words(s.cell_count, s.nc_max + 1, st);
    ag_launch_zero_words(s.words, 4, st);
    hipLaunchKernelGGL(bounds_kernel, dim3(1), dim3(kWide), 0, st, pts, count, n_max, s.mn, s.nc_max, s.grid);
    for (int round = 0; round < kRefineRounds; ++round) {
        hipLaunchKernelGGL(cell_count_kernel, dim3(s.blocks), dim3(kBlock), 0, st, pts, count, n_max, s.grid, s.nc_max, s.cell_count);
        hipLaunchKernelGGL(grid_refine_kernel, dim3(1), dim3(kWide), 0, st, s.cell_count, count, n_max, s.nc_max, s.grid);
        ag_launch_zero_words(s.cell_count, s.nc_max + 1, st);
    }
    hipLaunchKernelGGL(cell_count_kernel, dim3(s.blocks), dim3(kBlock), 0, st, pts, count, n_max, s.grid, s.nc_max, s.cell_count);
    hipLaunchKernelGGL(cell_scan_kernel, dim3(1), dim3(kWide), 0, st, s.cell_count, s.grid, s.nc_max, s.cell_start);
    hipLaunchKernelGGL(cell_fill_kernel, dim3(s.blocks), dim3(kBlock), 0, st, pts, count, n_max, s.grid, s.nc_max, s.cell_start, s.cell_count,
                       s.sorted);
    hipLaunchKernelGGL(knn_grid_kernel, dim3(s.blocks), dim3(kBlock), 0, st, s.sorted, count, n_max, s.grid, s.nc_max, s.cell_start, k, avg, s.work,
                       s.words + 1);
    hipLaunchKernelGGL(brute_kernel, dim3(n_max < kBruteBlocks ? n_max : kBruteBlocks), dim3(64), 0, st, pts, count, n_max, k, s.work, s.words + 1,
                       s.grid, avg, info);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_cloud_outlier_filter(const float *pts, const int32_t *count, int n_max, const double *avg, const double *std_ratio, double *stats,
                            uint8_t *keep, float *out, int32_t *count_out, void *workspace, size_t workspace_bytes, ag_stream_t stream)
{
    Scratch s;
    if (int rc = cloud_args("ag_cloud_outlier_filter", pts && count && avg && std_ratio && stats && keep && out && count_out, n_max, workspace,
                            workspace_bytes, &s))
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(outlier_stats_kernel, dim3(1), dim3(kWide), 0, st, avg, count, n_max, *std_ratio, stats);
    hipLaunchKernelGGL(outlier_flag_kernel, dim3(s.blocks), dim3(kBlock), 0, st, avg, count, n_max, stats, s.flags, keep, s.sums);
    launch_scatter(s, pts, s.flags, count, n_max, out, count_out, count_out + 1, st);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_cloud_select(const float *pts, const int32_t *count, int n_max, const uint8_t *flags, const float *z_below, float *out, int32_t *count_out,
                    void *workspace, size_t workspace_bytes, ag_stream_t stream)
{
    Scratch s;
    if (int rc = cloud_args("ag_cloud_select", pts && count && out && count_out, n_max, workspace, workspace_bytes, &s)) return rc;
    if ((flags == nullptr) == (z_below == nullptr)) return ag_fail(AG_ERR_ARG, "ag_cloud_select: give flags or z_below, one of them");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (flags) hipLaunchKernelGGL(flag_sums_kernel, dim3(s.blocks), dim3(kBlock), 0, st, flags, count, n_max, s.sums);
    else hipLaunchKernelGGL(below_flag_kernel, dim3(s.blocks), dim3(kBlock), 0, st, pts, count, n_max, z_below, s.flags, s.sums);
    launch_scatter(s, pts, flags ? flags : s.flags, count, n_max, out, count_out, nullptr, st);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

}  // extern "C"
