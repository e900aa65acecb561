// ag_cost.hip — trajectory cost terms of the MPPI planner that touch every particle of every sampled rollout.
//
// chamfer (src/planning/losses.py:4-10):  x (B,N,3), y (By,M,3), By in {1,B}
//     dis[b,m,n] = ||x[b,n] - y[b,m]||_2 ;  out[b] = mean_m min_n dis + mean_n min_m dis
// The reference materialises two (B,M,N,3) repeats (12 GB at B=1024, N=M=1000); here one workgroup per sample keeps
// both clouds in LDS and does the N*M pair sweep twice (rows / columns) with broadcast reads.  sqrt is monotone, so
// min(sqrt(d2)) == sqrt(min d2) bit-for-bit; only the two means differ from torch by summation order.
#include "ag_cloud_dev.h"

namespace {

// xmask / ymask: optional per-point validity (u8, (B,N) / (By,M)); masked-out points take no part in either direction —
// this is mean_chamfer's `state[i][mask[i]]` compaction (losses.py:12-24) without the per-sample host loop.  Invalid
// points are parked at +inf in LDS (their squared distance to anything finite is +inf, so no min ever picks them) and
// skipped as query points.  A sample with no valid point on either side yields NaN (the reference raises there).

// one direction: for every valid point of `q` (SoA planes qx / qy / qz, Q points) the squared distance to its nearest point of `o` (On points, On even, padded
// with +inf); adds sqrt(min) to s and 1 to c in ascending point order per thread
// IDX: also record, per query point, the index of its nearest point (strict < in ascending order: ties go to the lowest index; -1 for an invalid query or
// when no finite distance exists) into idx[0..Q).  The minimum itself is the same value either way (fminf and the compare chain pick the same element of
// non-negative squared distances, NaN ignored by both), so `s` and `c` are the same bits with and without it.  The tiled sweep (ag_cost_tiled.hip) carries
// the same inner loop per chunk: shared as one function it cost that kernel 2-4 % (profiles/cloud_dev_ab.txt), so both spell it out over the one pair_d2.
template <bool IDX>
__device__ __forceinline__ void chamfer_sweep(const float *qx, const float *qy, const float *qz, int Q, const float *ox, const float *oy, const float *oz, int On,
                                              int tid, float &s, float &c, int *idx)
{
    for (int q0 = tid; q0 < Q; q0 += 256 * kChamQ) {
        float a0[kChamQ], a1[kChamQ], a2[kChamQ], best[kChamQ];
        bool ok[kChamQ];
        int bi[kChamQ];
#pragma unroll
        for (int k = 0; k < kChamQ; ++k) {
            const int q = q0 + 256 * k;
            const float v = q < Q ? qx[q] : INFINITY;
            ok[k] = v != INFINITY;
            a0[k] = ok[k] ? v : 0.f; a1[k] = ok[k] ? qy[q] : 0.f; a2[k] = ok[k] ? qz[q] : 0.f;
            best[k] = INFINITY;
            bi[k] = -1;
        }
        for (int n = 0; n < On; n += 2) {      // (two points per trip as packed fp32: three 8-byte broadcast reads per eight pairs)
            const ag_f2 X = *reinterpret_cast<const ag_f2 *>(ox + n), Y = *reinterpret_cast<const ag_f2 *>(oy + n), Z = *reinterpret_cast<const ag_f2 *>(oz + n);
#pragma unroll
            for (int k = 0; k < kChamQ; ++k) {
                const ag_f2 d = pair_d2<ag_f2>(X - a0[k], Y - a1[k], Z - a2[k]);
                if constexpr (IDX) {
                    if (d.x < best[k]) { best[k] = d.x; bi[k] = n; }
                    if (d.y < best[k]) { best[k] = d.y; bi[k] = n + 1; }
                } else {
                    best[k] = fminf(best[k], fminf(d.x, d.y));
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kChamQ; ++k) {
            if (ok[k]) { s += sqrtf(best[k]); c += 1.f; }
            if constexpr (IDX) {
                const int q = q0 + 256 * k;
                if (q < Q) idx[q] = ok[k] ? bi[k] : -1;
            }
        }
    }
}

// IDX: chamfer_fwd_idx — the same value plus idx_x (B,N) / idx_y (B,M), the nearest-neighbour indices the backward needs
template <bool IDX>
__global__ __launch_bounds__(256) void chamfer_kernel(const float *x, const float *y, const unsigned char *xmask,
                                                      const unsigned char *ymask, int N, int M, int y_batched, float *out, int *idx_x, int *idx_y)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ float red[4][4];
    const int Np = (N + 1) & ~1, Mp = (M + 1) & ~1;      // planes of even length (8-byte reads of point pairs): the pad point sits at +inf
    float *sx = sm, *sy = sm + 3 * Np;                    // x cloud: planes sx, sx + Np, sx + 2 Np; y cloud likewise
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const CloudSample c = cloud_sample(x, y, xmask, ymask, N, M, y_batched, b);
    for (int i = tid; i < 3 * Np; i += 256) {
        const int n = i / 3, p = i - 3 * n;
        sx[p * Np + n] = (n >= N || (c.xm && !c.xm[n])) ? INFINITY : c.xb[i];
    }
    for (int i = tid; i < 3 * Mp; i += 256) {
        const int m = i / 3, p = i - 3 * m;
        sy[p * Mp + m] = (m >= M || (c.ym && !c.ym[m])) ? INFINITY : c.yb[i];
    }
    __syncthreads();
    float s_y = 0.f, s_x = 0.f, c_y = 0.f, c_x = 0.f;
    int *iy = IDX ? idx_y + (size_t)b * M : nullptr, *ix = IDX ? idx_x + (size_t)b * N : nullptr;
    chamfer_sweep<IDX>(sy, sy + Mp, sy + 2 * Mp, M, sx, sx + Np, sx + 2 * Np, Np, tid, s_y, c_y, iy);      // for every target point: nearest particle
    chamfer_sweep<IDX>(sx, sx + Np, sx + 2 * Np, N, sy, sy + Mp, sy + 2 * Mp, Mp, tid, s_x, c_x, ix);      // for every particle: nearest target point
    float acc[4] = {s_y, s_x, c_y, c_x};
    four_wave_park(acc, red, lane, wave);
    __syncthreads();
    if (tid == 0) out[b] = chamfer_value(red);
}

// ---- chamfer backward (the gather form of ag_cloud_dev.h): both index rows sit in LDS (4 (N + M) bytes, 51 KB at the resident limit) ----
// one side: for every valid query point q of `qp` (Q points, row idx_q of the nearest other point) the gradient into gq; `io` is the OTHER side's
// index row in LDS (On entries, padded with -1 to On4, a multiple of 4); inv_q / inv_o = 1 / (valid count) of the query / other side
__device__ __forceinline__ void chamfer_bwd_side(const float *qp, const unsigned char *qm, const int *idx_q, int Q, const float *op, const int *io, int On,
                                                 int On4, float g, float inv_q, float inv_o, int tid, float *gq)
{
    for (int q0 = tid; q0 < Q; q0 += 256 * kChamQ) {
        ChamferBwdQuery r;
        chamfer_bwd_load(r, q0, qp, qm, Q);
        for (int j = 0; j < On4; j += 4) chamfer_bwd_scan4(r, *reinterpret_cast<const int4 *>(io + j), op + 3 * j);
        chamfer_bwd_store(r, q0, Q, idx_q, op, On, g, inv_q, inv_o, gq);
    }
}

// one workgroup per sample; gy (when not null) receives the sample's own gradient at row b (a broadcast y: the caller sums the rows)
__global__ __launch_bounds__(256) void chamfer_bwd_kernel(const float *x, const float *y, const unsigned char *xmask, const unsigned char *ymask,
                                                          const int *idx_x, const int *idx_y, const float *grad_out, int N, int M, int y_batched,
                                                          float *gx, float *gy)
{
    extern __shared__ __attribute__((aligned(16))) int si[];
    __shared__ float red[2][4];
    const int N4 = (N + 3) & ~3, M4 = (M + 3) & ~3;
    int *sIx = si, *sIy = si + N4;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const CloudSample c = cloud_sample(x, y, xmask, ymask, N, M, y_batched, b);
    const int *ixb = idx_x + (size_t)b * N, *iyb = idx_y + (size_t)b * M;
    float cnt[2] = {0.f, 0.f};      // valid points of x, of y
    for (int i = tid; i < N4; i += 256) {
        sIx[i] = i < N ? ixb[i] : -1;
        if (i < N && (!c.xm || c.xm[i])) cnt[0] += 1.f;
    }
    for (int i = tid; i < M4; i += 256) {
        sIy[i] = i < M ? iyb[i] : -1;
        if (i < M && (!c.ym || c.ym[i])) cnt[1] += 1.f;
    }
    float inv_x, inv_y;
    chamfer_inv_counts(cnt, red, lane, wave, inv_x, inv_y);      // (its barrier also ends the filling of the index rows)
    const float g = grad_out[b];
    chamfer_bwd_side(c.xb, c.xm, ixb, N, c.yb, sIy, M, M4, g, inv_x, inv_y, tid, gx + (size_t)b * N * 3);
    if (gy) chamfer_bwd_side(c.yb, c.ym, iyb, M, c.xb, sIx, N, N4, g, inv_y, inv_x, tid, gy + (size_t)b * M * 3);
}

// gy[i] = sum_b gy[b * len + i] in ascending b, in place (row 0 receives the sum)
__global__ __launch_bounds__(256) void cloud_sum_rows_kernel(float *gy, int B, int len)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    float s = gy[i];
    for (int b = 1; b < B; ++b) s += gy[(size_t)b * len + i];
    gy[i] = s;
}

}  // namespace

// a broadcast target's gradient: the backward kernels of the three cloud units write one gy row per sample, row 0 receives their sum
void ag_launch_sum_rows(float *gy, int B, int len, int y_batched, hipStream_t s)
{
    if (gy && !y_batched && B > 1) hipLaunchKernelGGL(cloud_sum_rows_kernel, dim3((len + 255) / 256), dim3(256), 0, s, gy, B, len);
}

template <bool IDX>
static int launch_chamfer_impl(const float *x, const float *y, const unsigned char *xmask, const unsigned char *ymask, int B, int N, int M,
                               int y_batched, float *out, int *idx_x, int *idx_y, hipStream_t s)
{
    const size_t smem = (size_t)3 * (((N + 1) & ~1) + ((M + 1) & ~1)) * sizeof(float);      // (planes padded to an even number of points)
    if (!ag_cloud_resident(N, M)) return -1;
    if (smem > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(chamfer_kernel<IDX>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
        return -2;
    hipLaunchKernelGGL(chamfer_kernel<IDX>, dim3(B), dim3(256), smem, s, x, y, xmask, ymask, N, M, y_batched, out, idx_x, idx_y);
    return 0;
}

int ag_launch_chamfer(const float *x, const float *y, const unsigned char *xmask, const unsigned char *ymask, int B, int N, int M,
                      int y_batched, float *out, hipStream_t s)
{
    return launch_chamfer_impl<false>(x, y, xmask, ymask, B, N, M, y_batched, out, nullptr, nullptr, s);
}

int ag_launch_chamfer_idx(const float *x, const float *y, const unsigned char *xmask, const unsigned char *ymask, int B, int N, int M,
                          int y_batched, float *out, int *idx_x, int *idx_y, hipStream_t s)
{
    return launch_chamfer_impl<true>(x, y, xmask, ymask, B, N, M, y_batched, out, idx_x, idx_y, s);
}

int ag_launch_chamfer_backward(const float *x, const unsigned char *xmask, const float *y, const unsigned char *ymask, const int *idx_x,
                               const int *idx_y, const float *grad_out, int B, int N, int M, int y_batched, float *gx, float *gy, hipStream_t s)
{
    if (!ag_cloud_resident(N, M)) return -1;
    const size_t smem = (size_t)(((N + 3) & ~3) + ((M + 3) & ~3)) * sizeof(int);      // the two index rows, padded to a multiple of 4
    if (smem > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(chamfer_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
        return -2;
    hipLaunchKernelGGL(chamfer_bwd_kernel, dim3(B), dim3(256), smem, s, x, y, xmask, ymask, idx_x, idx_y, grad_out, N, M, y_batched, gx, gy);
    ag_launch_sum_rows(gy, B, 3 * M, y_batched, s);
    return 0;
}
