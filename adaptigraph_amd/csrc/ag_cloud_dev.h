// ag_cloud_dev.h — shared device layer of the cloud-distance kernels: chamfer with both clouds in LDS (ag_cost.hip), tiled chamfer
// (ag_cost_tiled.hip), earth-mover and Hausdorff (ag_match.hip).  No kernels here: what two of those units compute alike is written once, so
// that the bit equality the tiled chamfer promises with the resident one is one expression and not two copies.
//
// Arithmetic of a pair: d2 = (dx dx + dy dy) + dz dz in fp32 with separately rounded products (-ffp-contract=off: what torch's
// ((x - y) ** 2).sum(-1) computes), cost = sqrtf(d2), u(v) = v / ||v|| with u(0) = 0.
#pragma once
#include "ag_block_dev.h"
#include "ag_common.h"

typedef float ag_f2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int kChamQ = 4;      // query points a thread keeps in registers, forward and backward, resident and tiled

// ---- pair arithmetic ----
template <typename T>      // float, or ag_f2 for two pairs at once
__device__ __forceinline__ T pair_d2(T d0, T d1, T d2) { return (d0 * d0 + d1 * d1) + d2 * d2; }

__device__ __forceinline__ float pair_cost(float ax, float ay, float az, float bx, float by, float bz) { return sqrtf(pair_d2(ax - bx, ay - by, az - bz)); }

// s += u(a - o)
__device__ __forceinline__ void unit_add(float ax, float ay, float az, const float *o, float &sx, float &sy, float &sz)
{
    const float d0 = ax - o[0], d1 = ay - o[1], d2 = az - o[2];
    const float r = sqrtf(pair_d2(d0, d1, d2));
    if (r > 0.f) { sx += d0 / r; sy += d1 / r; sz += d2 / r; }
}

// ---- sample view: the clouds and masks of sample b; a broadcast target (y_batched = 0) is cloud 0 for every sample ----
struct CloudSample {
    const float *xb, *yb;
    const unsigned char *xm, *ym;      // nullptr: every point valid
};
__device__ __forceinline__ CloudSample cloud_sample(const float *x, const float *y, const unsigned char *xmask, const unsigned char *ymask, int N, int M,
                                                    int y_batched, int b)
{
    const int by = y_batched ? b : 0;
    return {x + (size_t)b * N * 3, y + (size_t)by * M * 3, xmask ? xmask + (size_t)b * N : nullptr, ymask ? ymask + (size_t)by * M : nullptr};
}

// ---- the four-wave reduction tail (four_wave_park / four_wave_total: ag_block_dev.h) of the chamfer kernels ----
// the chamfer value of a sample from the parked {sum_y, sum_x, n_y, n_x}: the two means; NaN when a side has no valid point
__device__ __forceinline__ float chamfer_value(const float (*red)[4])
{
    const float ny = four_wave_total(red[2]), nx = four_wave_total(red[3]);
    const float v = four_wave_total(red[0]) / ny + four_wave_total(red[1]) / nx;
    return (nx > 0.f && ny > 0.f) ? v : NAN;
}

// the chamfer backward's 1 / (valid count) of both sides from per-thread counts {x, y}: float adds of 1, exact (in any order) up to 2^24.
// An empty side: the value is NaN, the gradient zero: both come back 0.  Holds the barrier between the park and the totals.
__device__ __forceinline__ void chamfer_inv_counts(float (&c)[2], float (*red)[4], int lane, int wave, float &inv_x, float &inv_y)
{
    four_wave_park(c, red, lane, wave);
    __syncthreads();
    const float nx = four_wave_total(red[0]), my = four_wave_total(red[1]);
    const bool live = nx > 0.f && my > 0.f;
    inv_x = live ? 1.f / nx : 0.f;
    inv_y = live ? 1.f / my : 0.f;
}

// ---- chamfer backward (gather form, no atomics) ----
// For sample b with g = grad_out[b], Nx / My the valid counts:
//   gx[n] = g (u(x_n - y_{idx_x[n]}) / Nx + sum_{m: idx_y[m] = n} u(x_n - y_m) / My)
//   gy[m] = g (u(y_m - x_{idx_y[m]}) / My + sum_{n: idx_x[n] = m} u(y_m - x_n) / Nx)
// The scatter sums are gathers: a thread keeps kChamQ query points and scans the OTHER side's index row in ascending order, four entries per
// LDS read; the coordinates stay in global memory and are read only for the few matching entries.  Every sum has one fixed order.
// key: the query point's index, -2 for none (matches no index entry: entries are >= -1); a: its coordinates; s: sum of u(query - other) over its matches
struct ChamferBwdSlot { int key; float a0, a1, a2, s0, s1, s2; };
struct ChamferBwdQuery { ChamferBwdSlot p[kChamQ]; };

// slot k = point q0 + 256 k of the query side qp (Q points, mask qm or nullptr)
__device__ __forceinline__ void chamfer_bwd_load(ChamferBwdQuery &r, int q0, const float *qp, const unsigned char *qm, int Q)
{
#pragma unroll
    for (int k = 0; k < kChamQ; ++k) {
        const int q = q0 + 256 * k;
        const bool ok = q < Q && (!qm || qm[q]);
        ChamferBwdSlot &s = r.p[k];
        s.key = ok ? q : -2;
        s.a0 = ok ? qp[3 * (size_t)q] : 0.f; s.a1 = ok ? qp[3 * (size_t)q + 1] : 0.f; s.a2 = ok ? qp[3 * (size_t)q + 2] : 0.f;
        s.s0 = s.s1 = s.s2 = 0.f;
    }
}

// four entries e of the other side's index row; oj: the coordinates of the first of these four other points (read only behind a match)
__device__ __forceinline__ void chamfer_bwd_scan4(ChamferBwdQuery &r, int4 e, const float *oj)
{
#pragma unroll
    for (int k = 0; k < kChamQ; ++k) {
        ChamferBwdSlot &s = r.p[k];
        if (e.x == s.key) unit_add(s.a0, s.a1, s.a2, oj + 0, s.s0, s.s1, s.s2);
        if (e.y == s.key) unit_add(s.a0, s.a1, s.a2, oj + 3, s.s0, s.s1, s.s2);
        if (e.z == s.key) unit_add(s.a0, s.a1, s.a2, oj + 6, s.s0, s.s1, s.s2);
        if (e.w == s.key) unit_add(s.a0, s.a1, s.a2, oj + 9, s.s0, s.s1, s.s2);
    }
}

// after the whole row: the point's own nearest term (idx_q: the query side's index row; op, On: the other cloud; nn < On: never read past a cloud
// for a bad index), the scaling by inv_q / inv_o = 1 / (valid count) of the query / other side, the write to gq
__device__ __forceinline__ void chamfer_bwd_store(const ChamferBwdQuery &r, int q0, int Q, const int *idx_q, const float *op, int On, float g, float inv_q,
                                                  float inv_o, float *gq)
{
#pragma unroll
    for (int k = 0; k < kChamQ; ++k) {
        const int q = q0 + 256 * k;
        if (q >= Q) continue;
        const ChamferBwdSlot &s = r.p[k];
        float t0 = 0.f, t1 = 0.f, t2 = 0.f;
        const int nn = s.key >= 0 ? idx_q[q] : -1;
        if (nn >= 0 && nn < On) unit_add(s.a0, s.a1, s.a2, op + 3 * (size_t)nn, t0, t1, t2);
        const bool live = s.key >= 0 && inv_q > 0.f;
        gq[3 * (size_t)q + 0] = live ? g * (t0 * inv_q + s.s0 * inv_o) : 0.f;
        gq[3 * (size_t)q + 1] = live ? g * (t1 * inv_q + s.s1 * inv_o) : 0.f;
        gq[3 * (size_t)q + 2] = live ? g * (t2 * inv_q + s.s2 * inv_o) : 0.f;
    }
}

}  // namespace
