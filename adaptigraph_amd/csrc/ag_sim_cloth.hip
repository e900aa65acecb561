// ag_sim_cloth.hip — a batched mass-spring cloth simulator: one grasp-and-drag of E cloth episodes in one launch.  Like ag_sim.hip and
// ag_sim_pile.hip it stands in for the data side of the reference (src/sim/sim_env/flex_env.py:258-402 steps a closed CUDA solver); the model is
// this project's own (not FleX, no self-collision), stated operation for operation in adaptigraph_amd/sim/cloth.py (cloth_push_host, the float32 numpy
// statement) and repeated here so that both give the same bits.
//
// One 1024-thread workgroup owns an episode for the whole call, four particles per thread (particle i = t + 1024 k, n = nx nz <= 4096).  A
// particle's position at the start of the substep and its velocity stay in registers; LDS holds ONE copy of the predicted positions of all
// particles (three planes of 4096 floats, 48 KB) and their inverse masses (4096 bytes): the constraint sweep is a coloured Gauss-Seidel pass in
// place.  A sweep is twelve phases (sim/cloth.py has the order); within a phase no particle belongs to two pairs, so the threads of a phase touch
// disjoint words and its result does not depend on which thread takes which pair: that is the whole basis of the equality with the host.  A
// phase maps its pair keys q = 0 .. rows cols - 1 over the threads (q = t + 1024 m), splits q into (row a, column b) with a multiply-high by
// a precomputed reciprocal (exact for q < 4096 and divisors <= 64), and ends in a workgroup barrier: 1 + 12 iters barriers per substep.
// Segment step counts, iters, grasped or not and recording are uniform over a workgroup, and an episode outside its bounds returns as a whole
// before the first barrier, so every barrier is reached by all 1024 threads.  The pick is five rounds of a workgroup-wide minimum over the
// 64-bit keys (bits of d2) << 32 | index (block_min_u64: an integer minimum, exact in any order; equal d2 goes to the lower index).
// No atomics, no float reductions.  Every product is rounded on its own (-ffp-contract=off), division and square root are the correctly
// rounded ones.
#include "ag_sim_dev.h"
#include "ag_block_dev.h"

namespace {

constexpr int kClothThreads = 1024;
constexpr int kClothPer = AG_SIM_CLOTH_MAX_PARTICLES / kClothThreads;      // particles per thread
constexpr int kClothSide = 64;
constexpr int kPickK = AG_SIM_CLOTH_PICK_K;
constexpr unsigned long long kNoKey = ~0ull;

struct ClothPushArgs {
    const int32_t *nx, *nz, *steps;
    const float *rest, *gains, *inv, *action, *lat;
    float *x, *v, *obj, *eef;
    int32_t *n_frames, *picked;
    int n_max, F_max, n_push_max, substeps, iters, record_every, settle;
    float h, g, r, damp, lift, grasp2, finger, tool_y;
};

// q / d for 0 <= q < 4096 and 1 <= d <= 64 as a multiply-high by ceil(2^32 / d): the error q (d ceil(2^32 / d) - 2^32) < 4096 * 64 stays below 2^32
struct ClothDiv {
    int d;
    unsigned magic;
};
__device__ __forceinline__ ClothDiv cloth_div(int d) { return ClothDiv{d, d > 1 ? 0xFFFFFFFFu / (unsigned)d + 1u : 0u}; }
__device__ __forceinline__ int cloth_quot(int q, const ClothDiv &c) { return c.d > 1 ? (int)__umulhi((unsigned)q, c.magic) : q; }

// the u-th index whose bit 1 equals p, ascending: 2p, 2p + 1, 4 + 2p, 4 + 2p + 1, ...
__device__ __forceinline__ int cloth_par4(int u, int p) { return 4 * (u >> 1) + 2 * p + (u & 1); }
// how many bend pairs (c, c + 2) a line of `len` particles has whose first index has bit 1 equal to p
__device__ __forceinline__ int cloth_bend_count(int len, int p)
{
    const int starts = len - 2, rem = starts & 3;      // first indices 0 .. len - 3 (len >= 2)
    return 2 * (starts >> 2) + (p == 0 ? min(rem, 2) : max(rem - 2, 0));
}

struct ClothGrid {
    int nx, nz;
    ClothDiv by_nx, by_m[2], by_b[2];      // pairs per row: of the z families (nx), of the parity families along x, of bend x
};

// One phase of the sweep: FAM 0 stretch x, 1 stretch z, 2 diagonal (ix, iz)-(ix + 1, iz + 1), 3 diagonal (ix + 1, iz)-(ix, iz + 1), 4 bend x,
// 5 bend z; p the colour.  Every index it forms lies inside the grid: i, j < nx nz <= 4096.  Ends in a barrier.
template <int FAM>
__device__ __forceinline__ void cloth_phase(const int p, const ClothGrid &G, float *sx, float *sy, float *sz, const unsigned char *sw,
                                            const float rest, const float gain, const int t)
{
    const int nx = G.nx, nz = G.nz;
    const ClothDiv by = (FAM == 1 || FAM == 5) ? G.by_nx : FAM == 4 ? G.by_b[p] : G.by_m[p];
    const int rows = FAM == 0 || FAM == 4 ? nz : FAM == 2 || FAM == 3 ? nz - 1 : FAM == 1 ? (nz - p) / 2 : cloth_bend_count(nz, p);
    const int count = rows * by.d;
    for (int q = t; q < count; q += kClothThreads) {
        const int a = cloth_quot(q, by), b = q - a * by.d;
        int i, j;
        if (FAM == 0) { i = a * nx + 2 * b + p; j = i + 1; }
        else if (FAM == 1) { i = (2 * a + p) * nx + b; j = i + nx; }
        else if (FAM == 2) { i = a * nx + 2 * b + p; j = i + nx + 1; }
        else if (FAM == 3) { i = a * nx + 2 * b + p + 1; j = i + nx - 1; }
        else if (FAM == 4) { i = a * nx + cloth_par4(b, p); j = i + 2; }
        else { i = cloth_par4(a, p) * nx + b; j = i + 2 * nx; }
        const float xi = sx[i], yi = sy[i], zi = sz[i], xj = sx[j], yj = sy[j], zj = sz[j];
        const float dx = xj - xi, dy = yj - yi, dz = zj - zi;
        const float len = sqrtf((dx * dx + dy * dy) + dz * dz);
        const float wi = (float)sw[i], wj = (float)sw[j];
        const float ws = wi + wj;
        if (!(len == 0.f) && !(ws == 0.f)) {
            const float c = (gain * (len - rest)) / (len * ws);
            const float cx = c * dx, cy = c * dy, cz = c * dz;
            sx[i] = xi + wi * cx; sy[i] = yi + wi * cy; sz[i] = zi + wi * cz;
            sx[j] = xj - wj * cx; sy[j] = yj - wj * cy; sz[j] = zj - wj * cz;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(kClothThreads) void cloth_push_kernel(const ClothPushArgs a)
{
    __shared__ float s_x[AG_SIM_CLOTH_MAX_PARTICLES], s_y[AG_SIM_CLOTH_MAX_PARTICLES], s_z[AG_SIM_CLOTH_MAX_PARTICLES];
    __shared__ unsigned char s_w[AG_SIM_CLOTH_MAX_PARTICLES];
    const int e = blockIdx.x, t = threadIdx.x;
    const int nx = a.nx[e], nz = a.nz[e], n1 = a.steps[2 * e], n2 = a.steps[2 * e + 1];
    if (nx < 2 || nx > kClothSide || nz < 2 || nz > kClothSide || nx * nz > a.n_max || n1 < 1 || n2 < 1 || n1 > a.n_push_max ||
        n2 > a.n_push_max - n1)
        return sim_no_frame(a.n_frames, e, t);
    const int n = nx * nz, n_push = n1 + n2;
    const float l0 = a.rest[2 * e], lsh = a.rest[2 * e + 1], l2 = l0 * 2.f;
    const float ks = a.gains[4 * e], kh = a.gains[4 * e + 1], kb = a.gains[4 * e + 2], mu = a.gains[4 * e + 3];
    const float inv1 = a.inv[2 * e], inv2 = a.inv[2 * e + 1];
    const float xs = a.action[4 * e], zs = a.action[4 * e + 1], xe = a.action[4 * e + 2], ze = a.action[4 * e + 3];
    const float ux = a.lat[2 * e], uz = a.lat[2 * e + 1];
    const float h = a.h, r = a.r, damp = a.damp, lift = a.lift;
    const float gh = a.g * h, mgh = (mu * a.g) * h;
    const float fx = a.finger * ux, fz = a.finger * uz;
    const int S = a.substeps, total = n_push + a.settle;
    float *frames = a.obj + (size_t)e * a.F_max * a.n_max * 3;
    float *tool = a.eef + (size_t)e * a.F_max * 6;
    ClothGrid G;
    G.nx = nx; G.nz = nz;
    G.by_nx = cloth_div(nx);
    G.by_m[0] = cloth_div(nx / 2); G.by_m[1] = cloth_div((nx - 1) / 2);
    G.by_b[0] = cloth_div(cloth_bend_count(nx, 0)); G.by_b[1] = cloth_div(cloth_bend_count(nx, 1));

    bool live[kClothPer], pin[kClothPer];
    float x[kClothPer], y[kClothPer], z[kClothPer], vx[kClothPer], vy[kClothPer], vz[kClothPer], ox[kClothPer], oz[kClothPer];
    unsigned long long key[kClothPer];
#pragma unroll
    for (int k = 0; k < kClothPer; ++k) {
        const int i = t + kClothThreads * k;
        live[k] = i < n;
        const size_t row = ((size_t)e * a.n_max + (live[k] ? i : 0)) * 3;
        x[k] = live[k] ? a.x[row] : 0.f; y[k] = live[k] ? a.x[row + 1] : 0.f; z[k] = live[k] ? a.x[row + 2] : 0.f;
        vx[k] = live[k] ? a.v[row] : 0.f; vy[k] = live[k] ? a.v[row + 1] : 0.f; vz[k] = live[k] ? a.v[row + 2] : 0.f;
        ox[k] = x[k] - xs; oz[k] = z[k] - zs;
        const float d2 = ox[k] * ox[k] + oz[k] * oz[k];
        key[k] = live[k] ? ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)i : kNoKey;
        pin[k] = false;
    }
    // the pick: kPickK rounds of the workgroup's smallest key (block_min_u64: two barriers each, reached by every thread)
    int pk[kPickK];
    float d2min = 0.f;
#pragma unroll
    for (int rnd = 0; rnd < kPickK; ++rnd) {
        unsigned long long m = key[0];
#pragma unroll
        for (int k = 1; k < kClothPer; ++k) m = key[k] < m ? key[k] : m;
        const unsigned long long best = block_min_u64(m);
        pk[rnd] = best == kNoKey ? -1 : (int)(unsigned)(best & 0xFFFFFFFFull);
        if (rnd == 0) d2min = __uint_as_float((unsigned)(best >> 32));
#pragma unroll
        for (int k = 0; k < kClothPer; ++k)
            if (key[k] == best && best != kNoKey) { key[k] = kNoKey; pin[k] = true; }
    }
    const bool grasped = pk[0] >= 0 && d2min <= a.grasp2;      // (uniform)
    if (t < kPickK) a.picked[e * kPickK + t] = grasped ? pk[t] : -1;
#pragma unroll
    for (int k = 0; k < kClothPer; ++k) {
        pin[k] = pin[k] && grasped;
        if (live[k]) s_w[t + kClothThreads * k] = pin[k] ? 0 : 1;
    }
    float oy[kClothPer];
#pragma unroll
    for (int k = 0; k < kClothPer; ++k) oy[k] = y[k];

    float cx = xs, cy = 0.f, cz = zs;
    for (int st = 0; st < total; ++st) {
        const bool held = st < n_push;
        if (st == n_push) {      // the release: every particle is free again (read by the phases after the next barrier)
#pragma unroll
            for (int k = 0; k < kClothPer; ++k) {
                if (live[k]) s_w[t + kClothThreads * k] = 1;
                pin[k] = false;
            }
        }
        for (int s = 0; s < S; ++s) {
            // b'. the gripper's point of this substep
            if (st < n1) {
                const float tt = sim_substep_t(st, S, s, inv1);
                cx = xs + (xe - xs) * tt; cy = lift * tt; cz = zs + (ze - zs) * tt;
            } else if (held) {
                const float tt = sim_substep_t(st - n1, S, s, inv2);
                cx = xe; cy = fmaxf(lift - lift * tt, 0.f); cz = ze;
            }
            // a. predict, b. pins.  The planes were last read by their owners (below) and by the last phase, both before that phase's barrier
            // or after it by the owner alone, so the owner may overwrite its own words here.
#pragma unroll
            for (int k = 0; k < kClothPer; ++k) {
                const float wy = vy[k] - gh;
                float px = x[k] + h * (vx[k] * damp), py = y[k] + h * (wy * damp), pz = z[k] + h * (vz[k] * damp);
                if (pin[k]) { px = cx + ox[k]; py = cy + oy[k]; pz = cz + oz[k]; }
                if (live[k]) { s_x[t + kClothThreads * k] = px; s_y[t + kClothThreads * k] = py; s_z[t + kClothThreads * k] = pz; }
            }
            __syncthreads();
            // c. sweeps
            for (int it = 0; it < a.iters; ++it) {
                cloth_phase<0>(0, G, s_x, s_y, s_z, s_w, l0, ks, t); cloth_phase<0>(1, G, s_x, s_y, s_z, s_w, l0, ks, t);
                cloth_phase<1>(0, G, s_x, s_y, s_z, s_w, l0, ks, t); cloth_phase<1>(1, G, s_x, s_y, s_z, s_w, l0, ks, t);
                cloth_phase<2>(0, G, s_x, s_y, s_z, s_w, lsh, kh, t); cloth_phase<2>(1, G, s_x, s_y, s_z, s_w, lsh, kh, t);
                cloth_phase<3>(0, G, s_x, s_y, s_z, s_w, lsh, kh, t); cloth_phase<3>(1, G, s_x, s_y, s_z, s_w, lsh, kh, t);
                cloth_phase<4>(0, G, s_x, s_y, s_z, s_w, l2, kb, t); cloth_phase<4>(1, G, s_x, s_y, s_z, s_w, l2, kb, t);
                cloth_phase<5>(0, G, s_x, s_y, s_z, s_w, l2, kb, t); cloth_phase<5>(1, G, s_x, s_y, s_z, s_w, l2, kb, t);
            }
            // d. ground, e. velocity and friction
#pragma unroll
            for (int k = 0; k < kClothPer; ++k) {
                if (!live[k]) continue;
                const float px = s_x[t + kClothThreads * k], pz = s_z[t + kClothThreads * k];
                float py = s_y[t + kClothThreads * k];
                const bool on = py <= r;
                py = py < r ? r : py;      // (a NaN stays, as in numpy's maximum)
                float wx = (px - x[k]) / h, wz = (pz - z[k]) / h;
                const float wy = (py - y[k]) / h;
                if (on && !pin[k]) {
                    const float f = sim_coulomb(wx, wz, mgh);
                    wx = wx * f; wz = wz * f;
                }
                vx[k] = wx; vy[k] = wy; vz[k] = wz;
                x[k] = px; y[k] = py; z[k] = pz;
            }
        }
        if (held && st % a.record_every == 0) {
            const int f = sim_recorded_frame(st, a.record_every);
#pragma unroll
            for (int k = 0; k < kClothPer; ++k)
                if (live[k]) sim_store3(frames + ((size_t)f * a.n_max + t + kClothThreads * k) * 3, x[k], y[k], z[k]);
            if (t < 2) {
                float *o = tool + (f * 2 + t) * 3;
                o[0] = t == 0 ? cx + fx : cx - fx; o[1] = a.tool_y + cy; o[2] = t == 0 ? cz + fz : cz - fz;
            }
        }
    }
    const int f = sim_final_frame(n_push, a.record_every);
#pragma unroll
    for (int k = 0; k < kClothPer; ++k)
        if (live[k]) {
            const int i = t + kClothThreads * k;
            sim_store3(frames + ((size_t)f * a.n_max + i) * 3, x[k], y[k], z[k]);
            const size_t row = ((size_t)e * a.n_max + i) * 3;
            sim_store3(a.x + row, x[k], y[k], z[k]);
            sim_store3(a.v + row, vx[k], vy[k], vz[k]);
        }
    if (t < 2) {
        float *o = tool + (f * 2 + t) * 3;
        o[0] = t == 0 ? xe + fx : xe - fx; o[1] = a.tool_y + lift; o[2] = t == 0 ? ze + fz : ze - fz;
    }
    if (t == 0) a.n_frames[e] = f + 1;
}

}  // namespace

extern "C" {

int ag_sim_cloth_push(const int32_t *nx, const int32_t *nz, const float *rest, const float *gains, const int32_t *steps, const float *inv,
                      const float *action, const float *lat, float *x, float *v, float *obj, float *eef, int32_t *n_frames, int32_t *picked,
                      int E, int n_max, int F_max, int n_push_max, int substeps, int iters, int record_every, int settle, float h, float g,
                      float r, float damp, float lift, float grasp2, float finger, float tool_y, ag_stream_t stream)
{
    if (!nx || !nz || !rest || !gains || !steps || !inv || !action || !lat || !x || !v || !obj || !eef || !n_frames || !picked)
        return ag_fail(AG_ERR_ARG, "ag_sim_cloth_push: null argument");
    if (int err = sim_check_schedule("ag_sim_cloth_push", E, n_max, 4, AG_SIM_CLOTH_MAX_PARTICLES, "AG_SIM_CLOTH_MAX_PARTICLES", F_max, n_push_max, 2,
                                     substeps, true, iters, record_every, settle, h, "drag"))
        return err;
    ClothPushArgs a{nx, nz, steps, rest, gains, inv, action, lat, x, v, obj, eef, n_frames, picked, n_max, F_max, n_push_max, substeps, iters,
                    record_every, settle, h, g, r, damp, lift, grasp2, finger, tool_y};
    hipLaunchKernelGGL(cloth_push_kernel, dim3(E), dim3(kClothThreads), 0, static_cast<hipStream_t>(stream), a);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

}  // extern "C"
