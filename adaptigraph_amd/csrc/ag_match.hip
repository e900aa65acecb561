// ag_match.hip — the training losses of src/dynamics/gnn/loss.py that match two clouds without particle correspondence.
//
// earth-mover distance (loss.py:25-60):  x (B,N,3), y (By,M,3), By in {1,B}
//     the reference builds dis (B,N,M), copies it to the host, runs scipy.optimize.linear_sum_assignment per sample and gathers the pairs; here
//     one wave per sample solves the same assignment problem exactly (shortest augmenting paths, Jonker-Volgenant in Crouse's rectangular form:
//     the algorithm scipy runs) with the column side in registers, the row side in LDS and the cost of a pair recomputed from the coordinates
//     at every scan step: no (N,M) matrix anywhere, no atomics, no host read, the same bits on every call.
// hausdorff (loss.py:63-82): per sample the two directed maxima of the nearest-neighbour distance, with the points that attain them.
//
// cost of a pair: c = sqrtf((dx dx + dy dy) + dz dz) in fp32 with separately rounded products (-ffp-contract=off), widened to fp64
// for the solver: duals, path lengths and the sum are fp64.
#include "ag_cloud_dev.h"

namespace {

__device__ __forceinline__ bool finite3(const float *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// The wave-wide arg-min of (value, key), lower value first, then lower key, left in every lane.  The order is total (keys are distinct except between
// lanes without a candidate, which hold the same pair), so any exchange pattern that spans the wave ends with the same pair everywhere.  Inside a row
// of 16 lanes the partner comes by a DPP move (quads crossed by 1 and 2, then the row's halves and the row mirrored): a register operation, where
// ds_bpermute is an LDS-pipe round trip; the rows are joined by two __shfl_xor stages.
template <int CTRL>
__device__ __forceinline__ int dpp_move(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false); }

__device__ __forceinline__ void take_lower(double &bv, int &bk, double ov, int ok)
{
    if (ov < bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
}

template <int CTRL>
__device__ __forceinline__ void argmin_dpp_stage(double &bv, int &bk)
{
    const double ov = __hiloint2double(dpp_move<CTRL>(__double2hiint(bv)), dpp_move<CTRL>(__double2loint(bv)));
    take_lower(bv, bk, ov, dpp_move<CTRL>(bk));
}

__device__ __forceinline__ void wave_argmin(double &bv, int &bk)
{
    argmin_dpp_stage<0xB1>(bv, bk);      // quad_perm [1,0,3,2]
    argmin_dpp_stage<0x4E>(bv, bk);      // quad_perm [2,3,0,1]
    argmin_dpp_stage<0x141>(bv, bk);     // row_half_mirror
    argmin_dpp_stage<0x140>(bv, bk);     // row_mirror
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) take_lower(bv, bk, __shfl_xor(bv, o), __shfl_xor(bk, o));
}

// valid points of one cloud in ascending order: list[0..count) = their indices; marks[0..Q) = -1; bad: a valid coordinate is NaN or +-Inf
__device__ __forceinline__ int compact_valid(const float *p, const unsigned char *mask, int Q, int lane, int *list, int *marks, bool &bad)
{
    int count = 0;
    for (int base = 0; base < Q; base += 64) {
        const int q = base + lane;
        const bool v = q < Q && (!mask || mask[q]);
        if (v && !finite3(p + 3 * q)) bad = true;
        const unsigned long long bal = __ballot(v);
        if (v) list[count + ballot_rank(bal, lane)] = q;
        count += __popcll(bal);
        if (q < Q) marks[q] = -1;
    }
    return count;
}

// One wave per sample.  CPL: columns per lane; column j of the larger valid side belongs to lane j % 64, register slot j / 64, so the clouds
// hold at most 64 CPL points a side.  The smaller valid side are the rows: K = min(Nx, My) augmentations, each a Dijkstra-like search whose
// scan step is one broadcast of the current row (coordinates, dual), one update per owned column and one wave-wide arg-min of
// (path length, assigned?, column): lower length first, then a free column, then the lower index, so the result is one fixed optimum.
// Every loop is bounded by N, M or the number of rows assigned so far; none waits for convergence.
template <int CPL>
__global__ __launch_bounds__(64) void emd_kernel(const float *x, const float *y, const unsigned char *xmask, const unsigned char *ymask, int N, int M,
                                                 int y_batched, float *out, int *col, int *row)
{
    constexpr int MAXC = 64 * CPL;
    __shared__ double sU[MAXC];                            // row duals; after the solve: the matched cost of every x point
    __shared__ float sRx[MAXC], sRy[MAXC], sRz[MAXC];      // row coordinates
    __shared__ int sXi[MAXC], sYi[MAXC];                   // valid points of x / y: compact position -> index
    __shared__ int sC4R[MAXC], sR4C[MAXC], sPred[MAXC];    // column of a row, row of a column, predecessor row of a column on the shortest path
    __shared__ int sOutX[MAXC], sOutY[MAXC];               // col / row of this sample
    const int b = blockIdx.x, lane = threadIdx.x;
    const int by = y_batched ? b : 0;
    const float *xb = x + (size_t)b * N * 3, *yb = y + (size_t)by * M * 3;
    const unsigned char *xm = xmask ? xmask + (size_t)b * N : nullptr, *ym = ymask ? ymask + (size_t)by * M : nullptr;
    int *colb = col + (size_t)b * N, *rowb = row + (size_t)b * M;

    bool bad = false;
    const int nx = compact_valid(xb, xm, N, lane, sXi, sOutX, bad);
    const int my = compact_valid(yb, ym, M, lane, sYi, sOutY, bad);
    bool fail = __any(bad) || nx == 0 || my == 0;          // non-finite input or an empty side: NaN, every index -1
    const bool rows_x = nx <= my;
    const int R = rows_x ? nx : my, C = rows_x ? my : nx;
    const int *rowIdx = rows_x ? sXi : sYi, *colIdx = rows_x ? sYi : sXi;
    const float *rp = rows_x ? xb : yb, *cp = rows_x ? yb : xb;
    __syncthreads();

    float cx[CPL], cy[CPL], cz[CPL];
    double v[CPL];
    int r4c[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int j = lane + 64 * k;
        const bool in = !fail && j < C;
        const float *p = cp + 3 * (in ? colIdx[j] : 0);
        cx[k] = in ? p[0] : 0.f; cy[k] = in ? p[1] : 0.f; cz[k] = in ? p[2] : 0.f;
        v[k] = 0.0;
        r4c[k] = -1;
        if (in) sR4C[j] = -1;
    }
    if (!fail)
        for (int i = lane; i < R; i += 64) {
            const float *p = rp + 3 * rowIdx[i];
            sRx[i] = p[0]; sRy[i] = p[1]; sRz[i] = p[2];
            sU[i] = 0.0;
            sC4R[i] = -1;
        }
    __syncthreads();

    for (int cur = 0; cur < R && !fail; ++cur) {
        double spc[CPL];                                   // shortest path length to every owned column
        int pred[CPL];
        unsigned sc = 0;                                   // bit k: owned column k is scanned (on the tree)
#pragma unroll
        for (int k = 0; k < CPL; ++k) { spc[k] = INFINITY; pred[k] = -1; }
        double minVal = 0.0;
        int i = cur, sink = -1;
        for (int step = 0; step <= cur && sink < 0; ++step) {      // at most `cur` assigned columns join the tree before a free one does
            const float ax = sRx[i], ay = sRy[i], az = sRz[i];
            const double ui = sU[i];
            double bv = INFINITY;
            int bk = 0x7fffffff;
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                const int j = lane + 64 * k;
                if (j < C && !((sc >> k) & 1u)) {
                    const double c = (double)pair_cost(ax, ay, az, cx[k], cy[k], cz[k]);
                    const double r = ((minVal + c) - ui) - v[k];
                    if (r < spc[k]) { spc[k] = r; pred[k] = i; }
                    const int key = (r4c[k] >= 0 ? (1 << 20) : 0) | j;
                    if (spc[k] < bv || (spc[k] == bv && key < bk)) { bv = spc[k]; bk = key; }
                }
            }
            wave_argmin(bv, bk);
            if (!(bv < INFINITY)) break;                  // (a cost overflowed fp32: no finite path)
            minVal = bv;
            const int j = bk & 0xfffff;
            if ((j & 63) == lane) sc |= 1u << (j >> 6);
            const int ni = sR4C[j];
            if (ni < 0) sink = j; else i = ni;
        }
        if (sink < 0) { fail = true; break; }
        // duals: v[j] -= minVal - spc[j] for every scanned column, u[i] += the same for the row it is assigned to, u[cur] += minVal
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            if ((sc >> k) & 1u) {
                const double d = minVal - spc[k];
                v[k] -= d;
                if (r4c[k] >= 0) sU[r4c[k]] += d;
            }
            const int j = lane + 64 * k;
            if (j < C) sPred[j] = pred[k];
        }
        if (lane == 0) sU[cur] += minVal;
        __syncthreads();
        // augment along the predecessors from the free column back to row `cur`: at most cur + 1 rows
        int j = sink;
        for (int t = 0; t <= cur; ++t) {
            const int i2 = sPred[j];
            if (i2 < 0) break;                             // (cannot happen: every column on the path was reached from a row)
            const int jn = sC4R[i2];
            if (lane == 0) { sR4C[j] = i2; sC4R[i2] = j; }
            j = jn;
            if (i2 == cur) break;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const int jj = lane + 64 * k;
            r4c[k] = jj < C ? sR4C[jj] : -1;
        }
    }
    __syncthreads();

    if (!fail) {
        for (int i = lane; i < R; i += 64) {
            const int pr = rowIdx[i], pc = colIdx[sC4R[i]];
            const int n = rows_x ? pr : pc, m = rows_x ? pc : pr;
            sOutX[n] = m;
            sOutY[m] = n;
            sU[n] = (double)pair_cost(xb[3 * n], xb[3 * n + 1], xb[3 * n + 2], yb[3 * m], yb[3 * m + 1], yb[3 * m + 2]);
        }
    }
    __syncthreads();
    if (lane == 0) {
        float val = NAN;
        if (!fail) {
            double S = 0.0;
            for (int n = 0; n < N; ++n)
                if (sOutX[n] >= 0) S += sU[n];
            val = (float)(S / (double)R);
        }
        out[b] = val;
    }
    for (int n = lane; n < N; n += 64) colb[n] = fail ? -1 : sOutX[n];
    for (int m = lane; m < M; m += 64) rowb[m] = fail ? -1 : sOutY[m];
}

// ---- earth-mover backward (gather form): every point reads its partner ----
//   gx[n] = g u(x_n - y_col[n]) / K,  gy[m] = g u(y_m - x_row[m]) / K,  u(v) = v / ||v||, u(0) = 0, K = the number of matched pairs; unmatched: 0
__device__ __forceinline__ void emd_bwd_side(const float *q, const float *o, const int *partner, int Q, float g, float inv_k, int tid, float *gq)
{
    for (int i = tid; i < Q; i += 256) {
        const int p = partner[i];
        float g0 = 0.f, g1 = 0.f, g2 = 0.f;
        if (p >= 0) {
            const float d0 = q[3 * i] - o[3 * p], d1 = q[3 * i + 1] - o[3 * p + 1], d2 = q[3 * i + 2] - o[3 * p + 2];
            const float r = sqrtf(pair_d2(d0, d1, d2));
            if (r > 0.f) { g0 = g * ((d0 / r) * inv_k); g1 = g * ((d1 / r) * inv_k); g2 = g * ((d2 / r) * inv_k); }
        }
        gq[3 * i] = g0; gq[3 * i + 1] = g1; gq[3 * i + 2] = g2;
    }
}

__global__ __launch_bounds__(256) void emd_bwd_kernel(const float *x, const float *y, const int *col, const int *row, const float *grad_out, int N, int M,
                                                      int y_batched, float *gx, float *gy)
{
    __shared__ int red[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int by = y_batched ? b : 0;
    const float *xb = x + (size_t)b * N * 3, *yb = y + (size_t)by * M * 3;
    const int *colb = col + (size_t)b * N, *rowb = row + (size_t)b * M;
    int cnt = 0;
    for (int n = tid; n < N; n += 256) cnt += colb[n] >= 0 ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);      // (not wave_sum: the matching kernels keep the machine code they had)
    if (lane == 0) red[wave] = cnt;
    __syncthreads();
    const int K = four_wave_total(red);
    const float inv_k = K > 0 ? 1.f / (float)K : 0.f, g = grad_out[b];
    emd_bwd_side(xb, yb, colb, N, g, inv_k, tid, gx + (size_t)b * N * 3);
    if (gy) emd_bwd_side(yb, xb, rowb, M, g, inv_k, tid, gy + (size_t)b * M * 3);
}

// ---- hausdorff: per sample max_n min_m c and max_m min_n c with the points that attain them ----
// one direction: over the valid query points q (ascending per thread) the largest nearest-neighbour distance; ties of the min go to the lowest
// other index, ties of the max to the lowest query index.  Invalid points sit at +inf: skipped as queries, never a minimum (c = +inf is not < +inf).
__device__ __forceinline__ void hausdorff_dir(const float *qx, const float *qy, const float *qz, int Q, const float *ox, const float *oy, const float *oz,
                                              int On, int tid, float &best, int &bq, int &bo)
{
    best = -1.f; bq = -1; bo = -1;
    for (int q = tid; q < Q; q += 256) {
        const float a0 = qx[q], a1 = qy[q], a2 = qz[q];
        if (a0 == INFINITY) continue;
        float mc = INFINITY;
        int mi = -1;
        for (int o = 0; o < On; ++o) {
            const float c = pair_cost(a0, a1, a2, ox[o], oy[o], oz[o]);
            if (c < mc) { mc = c; mi = o; }
        }
        if (mi >= 0 && mc > best) { best = mc; bq = q; bo = mi; }
    }
}

__global__ __launch_bounds__(256) void hausdorff_kernel(const float *x, const float *y, const unsigned char *xmask, const unsigned char *ymask, int N, int M,
                                                        int y_batched, float *out, int *arg)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ float redv[2][4];
    __shared__ int redq[2][4], redo[2][4];
    float *sx = sm, *sy = sm + 3 * N;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int by = y_batched ? b : 0;
    const float *xb = x + (size_t)b * N * 3, *yb = y + (size_t)by * M * 3;
    const unsigned char *xm = xmask ? xmask + (size_t)b * N : nullptr, *ym = ymask ? ymask + (size_t)by * M : nullptr;
    for (int i = tid; i < 3 * N; i += 256) {
        const int n = i / 3, c = i - 3 * n;
        sx[c * N + n] = (xm && !xm[n]) ? INFINITY : xb[i];
    }
    for (int i = tid; i < 3 * M; i += 256) {
        const int m = i / 3, c = i - 3 * m;
        sy[c * M + m] = (ym && !ym[m]) ? INFINITY : yb[i];
    }
    __syncthreads();
    float bv[2];
    int bq[2], bo[2];
    hausdorff_dir(sx, sx + N, sx + 2 * N, N, sy, sy + M, sy + 2 * M, M, tid, bv[0], bq[0], bo[0]);
    hausdorff_dir(sy, sy + M, sy + 2 * M, M, sx, sx + N, sx + 2 * N, N, tid, bv[1], bq[1], bo[1]);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv[d], o);
            const int oq = __shfl_xor(bq[d], o), oo = __shfl_xor(bo[d], o);
            if (oq >= 0 && (bq[d] < 0 || ov > bv[d] || (ov == bv[d] && oq < bq[d]))) { bv[d] = ov; bq[d] = oq; bo[d] = oo; }
        }
        if (lane == 0) { redv[d][wave] = bv[d]; redq[d][wave] = bq[d]; redo[d][wave] = bo[d]; }
    }
    __syncthreads();
    if (tid == 0) {
        float fv[2];
        int fq[2], fo[2];
        for (int d = 0; d < 2; ++d) {
            fv[d] = -1.f; fq[d] = -1; fo[d] = -1;
            for (int w = 0; w < 4; ++w) {
                const float ov = redv[d][w];
                const int oq = redq[d][w];
                if (oq >= 0 && (fq[d] < 0 || ov > fv[d] || (ov == fv[d] && oq < fq[d]))) { fv[d] = ov; fq[d] = oq; fo[d] = redo[d][w]; }
            }
        }
        const bool live = fq[0] >= 0 && fq[1] >= 0;      // an empty side: NaN and -1 throughout
        out[2 * b] = live ? fv[0] : NAN;
        out[2 * b + 1] = live ? fv[1] : NAN;
        arg[4 * b] = live ? fq[0] : -1; arg[4 * b + 1] = live ? fo[0] : -1;
        arg[4 * b + 2] = live ? fq[1] : -1; arg[4 * b + 3] = live ? fo[1] : -1;
    }
}

template <int CPL>
void launch_emd_cpl(const float *x, const float *y, const unsigned char *xmask, const unsigned char *ymask, int B, int N, int M, int y_batched,
                    float *out, int *col, int *row, hipStream_t s)
{
    hipLaunchKernelGGL(emd_kernel<CPL>, dim3(B), dim3(64), 0, s, x, y, xmask, ymask, N, M, y_batched, out, col, row);
}

}  // namespace

int ag_launch_emd(const float *x, const float *y, const unsigned char *xmask, const unsigned char *ymask, int B, int N, int M, int y_batched,
                  float *out, int *col, int *row, hipStream_t s)
{
    const int big = N > M ? N : M;
    if (N < 1 || M < 1 || big > kEmdMaxPoints) return -1;
    if (big <= 64) launch_emd_cpl<1>(x, y, xmask, ymask, B, N, M, y_batched, out, col, row, s);
    else if (big <= 128) launch_emd_cpl<2>(x, y, xmask, ymask, B, N, M, y_batched, out, col, row, s);
    else if (big <= 256) launch_emd_cpl<4>(x, y, xmask, ymask, B, N, M, y_batched, out, col, row, s);
    else if (big <= 512) launch_emd_cpl<8>(x, y, xmask, ymask, B, N, M, y_batched, out, col, row, s);
    else launch_emd_cpl<16>(x, y, xmask, ymask, B, N, M, y_batched, out, col, row, s);
    return 0;
}

int ag_launch_emd_backward(const float *x, const float *y, const int *col, const int *row, const float *grad_out, int B, int N, int M, int y_batched,
                           float *gx, float *gy, hipStream_t s)
{
    hipLaunchKernelGGL(emd_bwd_kernel, dim3(B), dim3(256), 0, s, x, y, col, row, grad_out, N, M, y_batched, gx, gy);
    ag_launch_sum_rows(gy, B, 3 * M, y_batched, s);
    return 0;
}

int ag_launch_hausdorff(const float *x, const float *y, const unsigned char *xmask, const unsigned char *ymask, int B, int N, int M, int y_batched,
                        float *out, int *arg, hipStream_t s)
{
    if (!ag_cloud_resident(N, M)) return -1;              // both clouds of a sample in LDS
    const size_t smem = (size_t)3 * ((size_t)N + (size_t)M) * sizeof(float);
    if (smem > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(hausdorff_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
        return -2;
    hipLaunchKernelGGL(hausdorff_kernel, dim3(B), dim3(256), smem, s, x, y, xmask, ymask, N, M, y_batched, out, arg);
    return 0;
}
