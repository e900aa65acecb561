// ag_cost_tiled.hip — chamfer (src/planning/losses.py:4-10) for clouds of any size: the tiled form of ag_cost.hip's kernels.
//
// ag_cost.hip keeps both clouds of a sample in the LDS of ONE workgroup: N + M <= 12 800, and a call with few samples uses few CUs.  Here a
// sample is split into query tiles of kChamTQ points (one workgroup each, four query points per thread in registers, as there) and the OTHER
// cloud streams through LDS in chunks of kChamTO points in ascending index order; the minimum is carried across chunks in registers.
// Bit equality with the resident kernels, wherever both apply:
//   - the per-pair arithmetic, the reduction tail and the backward's pieces are the same code (ag_cloud_dev.h), the sweep's inner loop the
//     same text as chamfer_sweep's in ag_cost.hip (why it is not one function: see there);
//   - min is exact in any order, and with indices a strict < over ascending indices sends ties to the lowest index in both forms;
//   - the sweep only WRITES sqrt(min) per query point (near[B][M + N]); a second kernel, one workgroup per sample, adds them in the order
//     the resident kernel adds them: thread tid takes points tid, tid + 256, ... (the resident tid + 1024 j + 256 k, k = 0..3 inside j, is
//     that sequence), then the xor-shuffle tree, then (w0 + w1) + (w2 + w3), then sum_y / n_y + sum_x / n_x.
// The backward is the gather form of chamfer_bwd_kernel with the other side's index row streamed in chunks: per query point the matches are
// added in ascending index order, then the point's own nearest term, then the same scaling.  No atomics anywhere, nothing to zero, no host
// synchronisation: every launch goes to the caller's stream.
#include "ag_cloud_dev.h"

namespace {

constexpr int kQ = kChamQ, kTQ = kChamTQ, kTO = kChamTO;
static_assert(kTQ == 256 * kQ, "a query tile is four points per thread of a 256-thread workgroup");
static_assert(kTO % 4 == 0, "chunks hold whole point pairs (forward) and whole int4 index groups (backward)");
constexpr float kInvalid = -1.f;            // near[] marker of an invalid query point (sqrt never returns a negative value)

// which (sample, side, tile) a workgroup of the flattened grid works on: per sample the tiles of side 0 first, then those of side 1
struct TileId { int b, side, tile; };
__device__ __forceinline__ TileId tile_of(unsigned blk, int tiles0, int tiles1)
{
    const unsigned per = (unsigned)(tiles0 + tiles1);
    const int b = (int)(blk / per), r = (int)(blk - (unsigned)b * per);
    return r < tiles0 ? TileId{b, 0, r} : TileId{b, 1, r - tiles0};
}

// forward sweep: side 0 = the target points y as queries against the particles x, side 1 = the particles against the target
template <bool IDX>
__global__ __launch_bounds__(256) void chamfer_tiled_sweep_kernel(const float *x, const float *y, const unsigned char *xmask,
                                                                  const unsigned char *ymask, int N, int M, int y_batched, float *near,
                                                                  int *idx_x, int *idx_y)
{
    __shared__ __attribute__((aligned(16))) float so[3 * kTO];      // the chunk: planes so, so + kTO, so + 2 kTO
    const int tid = threadIdx.x;
    const TileId t = tile_of(blockIdx.x, (M + kTQ - 1) / kTQ, (N + kTQ - 1) / kTQ);
    const int b = t.b, by = y_batched ? b : 0;
    const bool qy = t.side == 0;
    const int Q = qy ? M : N, On = qy ? N : M;
    const float *qb = qy ? y + (size_t)by * M * 3 : x + (size_t)b * N * 3;
    const float *ob = qy ? x + (size_t)b * N * 3 : y + (size_t)by * M * 3;
    const unsigned char *qm = qy ? (ymask ? ymask + (size_t)by * M : nullptr) : (xmask ? xmask + (size_t)b * N : nullptr);
    const unsigned char *om = qy ? (xmask ? xmask + (size_t)b * N : nullptr) : (ymask ? ymask + (size_t)by * M : nullptr);

    float a0[kQ], a1[kQ], a2[kQ], best[kQ];
    bool ok[kQ];
    int bi[kQ];
#pragma unroll
    for (int k = 0; k < kQ; ++k) {
        const int q = t.tile * kTQ + tid + 256 * k;
        const float v = (q < Q && (!qm || qm[q])) ? qb[3 * (size_t)q] : INFINITY;      // (a masked-out point is parked at +inf, as in the resident kernel)
        ok[k] = v != INFINITY;
        a0[k] = ok[k] ? v : 0.f; a1[k] = ok[k] ? qb[3 * (size_t)q + 1] : 0.f; a2[k] = ok[k] ? qb[3 * (size_t)q + 2] : 0.f;
        best[k] = INFINITY;
        bi[k] = -1;
    }
    for (int c0 = 0; c0 < On; c0 += kTO) {
        const int len = min(kTO, On - c0), lenp = (len + 1) & ~1;      // (even length: the pad point sits at +inf)
        if (c0) __syncthreads();                                        // every thread is done with the previous chunk
        for (int i = tid; i < 3 * lenp; i += 256) {
            const int n = i / 3, c = i - 3 * n, g = c0 + n;
            so[c * kTO + n] = (g >= On || (om && !om[g])) ? INFINITY : ob[3 * (size_t)c0 + i];
        }
        __syncthreads();
        for (int n = 0; n < lenp; n += 2) {
            const ag_f2 X = *reinterpret_cast<const ag_f2 *>(so + n), Y = *reinterpret_cast<const ag_f2 *>(so + kTO + n),
                        Z = *reinterpret_cast<const ag_f2 *>(so + 2 * kTO + n);
#pragma unroll
            for (int k = 0; k < kQ; ++k) {
                const ag_f2 d = pair_d2<ag_f2>(X - a0[k], Y - a1[k], Z - a2[k]);
                if constexpr (IDX) {
                    if (d.x < best[k]) { best[k] = d.x; bi[k] = c0 + n; }
                    if (d.y < best[k]) { best[k] = d.y; bi[k] = c0 + n + 1; }
                } else {
                    best[k] = fminf(best[k], fminf(d.x, d.y));
                }
            }
        }
    }
    float *nb = near + (size_t)b * ((size_t)N + M) + (qy ? 0 : M);      // a sample's row: its M target points, then its N particles
    int *ib = IDX ? (qy ? idx_y + (size_t)b * M : idx_x + (size_t)b * N) : nullptr;
#pragma unroll
    for (int k = 0; k < kQ; ++k) {
        const int q = t.tile * kTQ + tid + 256 * k;
        if (q >= Q) continue;
        nb[q] = ok[k] ? sqrtf(best[k]) : kInvalid;
        if constexpr (IDX) ib[q] = ok[k] ? bi[k] : -1;
    }
}

// one workgroup per sample: the two means, added in the resident kernel's order
__global__ __launch_bounds__(256) void chamfer_tiled_finish_kernel(const float *near, int N, int M, float *out)
{
    __shared__ float red[4][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *ny_ = near + (size_t)b * ((size_t)N + M), *nx_ = ny_ + M;
    float s_y = 0.f, s_x = 0.f, c_y = 0.f, c_x = 0.f;
    for (int q = tid; q < M; q += 256) {
        const float v = ny_[q];
        if (v != kInvalid) { s_y += v; c_y += 1.f; }
    }
    for (int q = tid; q < N; q += 256) {
        const float v = nx_[q];
        if (v != kInvalid) { s_x += v; c_x += 1.f; }
    }
    float acc[4] = {s_y, s_x, c_y, c_x};
    four_wave_park(acc, red, lane, wave);
    __syncthreads();
    if (tid == 0) out[b] = chamfer_value(red);
}

// ---- backward (the gather form of ag_cloud_dev.h, the other side's index row streamed through LDS in chunks) ----
// side 0 = gx (the particles as queries, the target's index row idx_y streamed), side 1 = gy; tiles_y = 0 when gy is not wanted
__global__ __launch_bounds__(256) void chamfer_tiled_bwd_kernel(const float *x, const float *y, const unsigned char *xmask, const unsigned char *ymask,
                                                                const int *idx_x, const int *idx_y, const float *grad_out, int N, int M,
                                                                int y_batched, int tiles_y, float *gx, float *gy)
{
    __shared__ __attribute__((aligned(16))) int si[kTO];
    __shared__ float red[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const TileId t = tile_of(blockIdx.x, (N + kTQ - 1) / kTQ, tiles_y);
    const int b = t.b;
    const CloudSample c = cloud_sample(x, y, xmask, ymask, N, M, y_batched, b);
    const int *ixb = idx_x + (size_t)b * N, *iyb = idx_y + (size_t)b * M;
    float cnt[2] = {0.f, 0.f};      // the valid counts of x, of y, recounted from the masks
    for (int i = tid; i < N; i += 256)
        if (!c.xm || c.xm[i]) cnt[0] += 1.f;
    for (int i = tid; i < M; i += 256)
        if (!c.ym || c.ym[i]) cnt[1] += 1.f;
    float inv_x, inv_y;
    chamfer_inv_counts(cnt, red, lane, wave, inv_x, inv_y);
    const float g = grad_out[b];

    const bool sx = t.side == 0;
    const float *qp = sx ? c.xb : c.yb, *op = sx ? c.yb : c.xb;
    const unsigned char *qm = sx ? c.xm : c.ym;
    const int *idx_q = sx ? ixb : iyb, *io = sx ? iyb : ixb;
    const int Q = sx ? N : M, On = sx ? M : N;
    const float inv_q = sx ? inv_x : inv_y, inv_o = sx ? inv_y : inv_x;
    float *gq = sx ? gx + (size_t)b * N * 3 : gy + (size_t)b * M * 3;

    const int q0 = t.tile * kTQ + tid;
    ChamferBwdQuery r;
    chamfer_bwd_load(r, q0, qp, qm, Q);
    for (int c0 = 0; c0 < On; c0 += kTO) {
        const int len = min(kTO, On - c0), len4 = (len + 3) & ~3;      // (padded with -1 to a multiple of 4)
        if (c0) __syncthreads();
        for (int i = tid; i < len4; i += 256) si[i] = i < len ? io[c0 + i] : -1;
        __syncthreads();
        // (a point's coordinates are read only behind a match, and a match is an entry below On)
        for (int j = 0; j < len4; j += 4) chamfer_bwd_scan4(r, *reinterpret_cast<const int4 *>(si + j), op + 3 * (size_t)(c0 + j));
    }
    chamfer_bwd_store(r, q0, Q, idx_q, op, On, g, inv_q, inv_o, gq);
}

}  // namespace

// the flattened grid must fit gridDim.x
static long long tiled_blocks(int B, int tiles) { return (long long)B * tiles; }

int ag_launch_chamfer_tiled(const float *x, const float *y, const unsigned char *xmask, const unsigned char *ymask, int B, int N, int M,
                            int y_batched, float *out, int *idx_x, int *idx_y, float *near, hipStream_t s)
{
    const long long blocks = tiled_blocks(B, (N + kTQ - 1) / kTQ + (M + kTQ - 1) / kTQ);
    if (blocks > 0x7fffffffLL) return -1;
    if (idx_x)
        hipLaunchKernelGGL(chamfer_tiled_sweep_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, x, y, xmask, ymask, N, M, y_batched, near, idx_x,
                           idx_y);
    else
        hipLaunchKernelGGL(chamfer_tiled_sweep_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, x, y, xmask, ymask, N, M, y_batched, near,
                           nullptr, nullptr);
    hipLaunchKernelGGL(chamfer_tiled_finish_kernel, dim3(B), dim3(256), 0, s, near, N, M, out);
    return 0;
}

int ag_launch_chamfer_tiled_backward(const float *x, const unsigned char *xmask, const float *y, const unsigned char *ymask, const int *idx_x,
                                     const int *idx_y, const float *grad_out, int B, int N, int M, int y_batched, float *gx, float *gy,
                                     hipStream_t s)
{
    const int tiles_y = gy ? (M + kTQ - 1) / kTQ : 0;
    const long long blocks = tiled_blocks(B, (N + kTQ - 1) / kTQ + tiles_y);
    if (blocks > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL(chamfer_tiled_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, y, xmask, ymask, idx_x, idx_y, grad_out, N, M, y_batched,
                       tiles_y, gx, gy);
    ag_launch_sum_rows(gy, B, 3 * M, y_batched, s);
    return 0;
}
