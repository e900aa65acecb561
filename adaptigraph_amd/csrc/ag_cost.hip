// ag_cost.hip — trajectory cost terms of the MPPI planner that touch every particle of every sampled rollout.
//
// chamfer (src/planning/losses.py:4-10):  x (B,N,3), y (By,M,3), By in {1,B}
//     dis[b,m,n] = ||x[b,n] - y[b,m]||_2 ;  out[b] = mean_m min_n dis + mean_n min_m dis
// The reference materialises two (B,M,N,3) repeats (12 GB at B=1024, N=M=1000); here one workgroup per sample keeps
// both clouds in LDS and does the N*M pair sweep twice (rows / columns) with broadcast reads.  sqrt is monotone, so
// min(sqrt(d2)) == sqrt(min d2) bit-for-bit; only the two means differ from torch by summation order.
#include "ag_common.h"

namespace {

// xmask / ymask: optional per-point validity (u8, (B,N) / (By,M)); masked-out points take no part in either direction —
// this is mean_chamfer's `state[i][mask[i]]` compaction (losses.py:12-24) without the per-sample host loop.  Invalid
// points are parked at +inf in LDS (their squared distance to anything finite is +inf, so no min ever picks them) and
// skipped as query points.  A sample with no valid point on either side yields NaN (the reference raises there).
// r06: the sweep is VALU work (9 instructions per pair with separately rounded products: what torch's ((x - y) ** 2).sum(-1) computes) and was bound by its LDS
// reads instead — one query point per thread and trip, three broadcast reads per pair.  Now a thread keeps FOUR query points in registers and walks the other
// cloud two points per trip (structure-of-arrays in LDS: three 8-byte broadcast reads per eight pairs; the two points of a trip as packed fp32 operations): the
// same arithmetic per pair, the same minimum (min is exact in any order), the same order of a thread's additions — the same bits, 0.90 -> 0.4x ms per
// 1 024 x 1 000 x 1 000 call.
typedef float ag_f2 __attribute__((ext_vector_type(2)));
constexpr int kChamQ = 4;      // query points per thread and sweep

// one direction: for every valid point of `q` (SoA planes qx / qy / qz, Q points) the squared distance to its nearest point of `o` (On points, On even, padded
// with +inf); adds sqrt(min) to s and 1 to c in ascending point order per thread
// IDX: also record, per query point, the index of its nearest point (strict < in ascending order: ties go to the lowest index; -1 for an invalid query or
// when no finite distance exists) into idx[0..Q).  The minimum itself is the same value either way (fminf and the compare chain pick the same element of
// non-negative squared distances, NaN ignored by both), so `s` and `c` are the same bits with and without it.
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
        for (int n = 0; n < On; n += 2) {
            const ag_f2 X = *reinterpret_cast<const ag_f2 *>(ox + n), Y = *reinterpret_cast<const ag_f2 *>(oy + n), Z = *reinterpret_cast<const ag_f2 *>(oz + n);
#pragma unroll
            for (int k = 0; k < kChamQ; ++k) {
                const ag_f2 d0 = X - a0[k], d1 = Y - a1[k], d2 = Z - a2[k];
                const ag_f2 d = (d0 * d0 + d1 * d1) + d2 * d2;
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
    const int by = y_batched ? b : 0;
    const float *xb = x + (size_t)b * N * 3, *yb = y + (size_t)by * M * 3;
    const unsigned char *xm = xmask ? xmask + (size_t)b * N : nullptr, *ym = ymask ? ymask + (size_t)by * M : nullptr;
    for (int i = tid; i < 3 * Np; i += 256) {
        const int n = i / 3, c = i - 3 * n;
        sx[c * Np + n] = (n >= N || (xm && !xm[n])) ? INFINITY : xb[i];
    }
    for (int i = tid; i < 3 * Mp; i += 256) {
        const int m = i / 3, c = i - 3 * m;
        sy[c * Mp + m] = (m >= M || (ym && !ym[m])) ? INFINITY : yb[i];
    }
    __syncthreads();
    float s_y = 0.f, s_x = 0.f, c_y = 0.f, c_x = 0.f;
    int *iy = IDX ? idx_y + (size_t)b * M : nullptr, *ix = IDX ? idx_x + (size_t)b * N : nullptr;
    chamfer_sweep<IDX>(sy, sy + Mp, sy + 2 * Mp, M, sx, sx + Np, sx + 2 * Np, Np, tid, s_y, c_y, iy);      // for every target point: nearest particle
    chamfer_sweep<IDX>(sx, sx + Np, sx + 2 * Np, N, sy, sy + Mp, sy + 2 * Mp, Mp, tid, s_x, c_x, ix);      // for every particle: nearest target point
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s_y += __shfl_xor(s_y, o); s_x += __shfl_xor(s_x, o);
        c_y += __shfl_xor(c_y, o); c_x += __shfl_xor(c_x, o);
    }
    if (lane == 0) { red[0][wave] = s_y; red[1][wave] = s_x; red[2][wave] = c_y; red[3][wave] = c_x; }
    __syncthreads();
    if (tid == 0) {
        const float ny = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]), nx = (red[3][0] + red[3][1]) + (red[3][2] + red[3][3]);
        const float v = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / ny + ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / nx;
        out[b] = (nx > 0.f && ny > 0.f) ? v : NAN;
    }
}

// ---- chamfer backward (gather form, no atomics) ----
// For sample b with g = grad_out[b], Nx / My the valid counts, u(v) = v / ||v|| (u(0) = 0):
//   gx[n] = g (u(x_n - y_{idx_x[n]}) / Nx + sum_{m: idx_y[m] = n} u(x_n - y_m) / My)
//   gy[m] = g (u(y_m - x_{idx_y[m]}) / My + sum_{n: idx_x[n] = m} u(y_m - x_n) / Nx)
// The scatter sums are gathers: both index rows sit in LDS (4 (N + M) bytes, 51 KB at the 12 800-point limit: the coordinates stay in global
// memory and are read only for the few matching entries), and each query point scans the other side's index row in ascending order, four
// query points per thread and four entries per LDS read.  Every sum has one fixed order, so the result is the same bits on every call.

__device__ __forceinline__ void unit_add(float ax, float ay, float az, const float *o, float &sx, float &sy, float &sz)
{
    const float d0 = ax - o[0], d1 = ay - o[1], d2 = az - o[2];
    const float r = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
    if (r > 0.f) { sx += d0 / r; sy += d1 / r; sz += d2 / r; }
}

// one side: for every valid query point q of `qp` (Q points, row idx_q of the nearest other point) the gradient into gq; `io` is the OTHER side's
// index row in LDS (On entries, padded with -1 to a multiple of 4); inv_q / inv_o = 1 / (valid count) of the query / other side
__device__ __forceinline__ void chamfer_bwd_side(const float *qp, const unsigned char *qm, const int *idx_q, int Q, const float *op, const int *io, int On4,
                                                 float g, float inv_q, float inv_o, int tid, float *gq)
{
    for (int q0 = tid; q0 < Q; q0 += 256 * kChamQ) {
        int key[kChamQ];
        float a0[kChamQ], a1[kChamQ], a2[kChamQ], s0[kChamQ], s1[kChamQ], s2[kChamQ];
#pragma unroll
        for (int k = 0; k < kChamQ; ++k) {
            const int q = q0 + 256 * k;
            const bool ok = q < Q && (!qm || qm[q]);
            key[k] = ok ? q : -2;                            // -2 matches no index entry (entries are >= -1)
            a0[k] = ok ? qp[3 * q] : 0.f; a1[k] = ok ? qp[3 * q + 1] : 0.f; a2[k] = ok ? qp[3 * q + 2] : 0.f;
            s0[k] = s1[k] = s2[k] = 0.f;
        }
        for (int j = 0; j < On4; j += 4) {
            const int4 e = *reinterpret_cast<const int4 *>(io + j);
#pragma unroll
            for (int k = 0; k < kChamQ; ++k) {
                if (e.x == key[k]) unit_add(a0[k], a1[k], a2[k], op + 3 * (j + 0), s0[k], s1[k], s2[k]);
                if (e.y == key[k]) unit_add(a0[k], a1[k], a2[k], op + 3 * (j + 1), s0[k], s1[k], s2[k]);
                if (e.z == key[k]) unit_add(a0[k], a1[k], a2[k], op + 3 * (j + 2), s0[k], s1[k], s2[k]);
                if (e.w == key[k]) unit_add(a0[k], a1[k], a2[k], op + 3 * (j + 3), s0[k], s1[k], s2[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < kChamQ; ++k) {
            const int q = q0 + 256 * k;
            if (q >= Q) continue;
            float t0 = 0.f, t1 = 0.f, t2 = 0.f;
            const int nn = key[k] >= 0 ? idx_q[q] : -1;
            if (nn >= 0) unit_add(a0[k], a1[k], a2[k], op + 3 * nn, t0, t1, t2);
            const bool live = key[k] >= 0 && inv_q > 0.f;
            gq[3 * q + 0] = live ? g * (t0 * inv_q + s0[k] * inv_o) : 0.f;
            gq[3 * q + 1] = live ? g * (t1 * inv_q + s1[k] * inv_o) : 0.f;
            gq[3 * q + 2] = live ? g * (t2 * inv_q + s2[k] * inv_o) : 0.f;
        }
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
    const int by = y_batched ? b : 0;
    const float *xb = x + (size_t)b * N * 3, *yb = y + (size_t)by * M * 3;
    const unsigned char *xm = xmask ? xmask + (size_t)b * N : nullptr, *ym = ymask ? ymask + (size_t)by * M : nullptr;
    const int *ixb = idx_x + (size_t)b * N, *iyb = idx_y + (size_t)b * M;
    float cx = 0.f, cy = 0.f;
    for (int i = tid; i < N4; i += 256) {
        sIx[i] = i < N ? ixb[i] : -1;
        if (i < N && (!xm || xm[i])) cx += 1.f;
    }
    for (int i = tid; i < M4; i += 256) {
        sIy[i] = i < M ? iyb[i] : -1;
        if (i < M && (!ym || ym[i])) cy += 1.f;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { cx += __shfl_xor(cx, o); cy += __shfl_xor(cy, o); }
    if (lane == 0) { red[0][wave] = cx; red[1][wave] = cy; }
    __syncthreads();
    const float nx = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]), my = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    const bool live = nx > 0.f && my > 0.f;                  // an empty side: the value is NaN, the gradient zero
    const float inv_x = live ? 1.f / nx : 0.f, inv_y = live ? 1.f / my : 0.f, g = grad_out[b];
    chamfer_bwd_side(xb, xm, ixb, N, yb, sIy, M4, g, inv_x, inv_y, tid, gx + (size_t)b * N * 3);
    if (gy) chamfer_bwd_side(yb, ym, iyb, M, xb, sIx, N4, g, inv_y, inv_x, tid, gy + (size_t)b * M * 3);
}

// gy[i] = sum_b gy[b * len + i] in ascending b, in place (row 0 receives the sum)
__global__ __launch_bounds__(256) void chamfer_sum_rows_kernel(float *gy, int B, int len)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    float s = gy[i];
    for (int b = 1; b < B; ++b) s += gy[(size_t)b * len + i];
    gy[i] = s;
}

}  // namespace

static int chamfer_fits(int N, int M) { return (size_t)3 * (N + M) * sizeof(float) <= 150 * 1024; }

template <bool IDX>
static int launch_chamfer_impl(const float *x, const float *y, const unsigned char *xmask, const unsigned char *ymask, int B, int N, int M,
                               int y_batched, float *out, int *idx_x, int *idx_y, hipStream_t s)
{
    const size_t smem = (size_t)3 * (((N + 1) & ~1) + ((M + 1) & ~1)) * sizeof(float);      // (planes padded to an even number of points)
    if (!chamfer_fits(N, M)) return -1;
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
    if (!chamfer_fits(N, M)) return -1;
    const size_t smem = (size_t)(((N + 3) & ~3) + ((M + 3) & ~3)) * sizeof(int);      // the two index rows, padded to a multiple of 4
    if (smem > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(chamfer_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
        return -2;
    hipLaunchKernelGGL(chamfer_bwd_kernel, dim3(B), dim3(256), smem, s, x, y, xmask, ymask, idx_x, idx_y, grad_out, N, M, y_batched, gx, gy);
    if (gy && !y_batched && B > 1)
        hipLaunchKernelGGL(chamfer_sum_rows_kernel, dim3((3 * M + 255) / 256), dim3(256), 0, s, gy, B, 3 * M);
    return 0;
}
