// ag_mppi.hip — the MPPI update of every chunk of a planning step in one launch: optimize_action_mppi and clip_actions of
// src/planning/plan_utils.py:31-39 and 80-101 and the arg-max that keeps a chunk's best sample (src/planning/real_world/planner.py:259-265).
//
// mppi_update_kernel: one workgroup of kMppiThreads per chunk of S samples.  A thread owns the samples tid, tid + kMppiThreads, ...  Its first
// kMppiU of them are loaded up front — the rewards and the action rows of look-ahead index 0 in flight together — and stay in registers for the
// whole kernel: a chunk of up to kMppiThreads * kMppiU samples (the reference's 500) reads every reward once and, with L = 1, every input word
// once.  The samples beyond are re-read (a strided re-read out of L2) in each of the three passes: maximum and arg-max, the softmax denominator,
// the weighted sums per look-ahead index.
//
// Arithmetic, fp32, every product and sum rounded separately: t = reward * reward_weight; e = exp(t - max t); w = e / sum e; per look-ahead index the
// sums of w x, w z, w (x - (len * push_length) cos theta), w (z - (len * push_length) sin theta); theta' = atan2 of the start minus the end,
// len' = sqrt(dx dx + dz dz) / push_length; theta' wrapped by ((theta + pi) mod 2 pi) - pi with the divisor's sign, every field clamped.
// Every reduction has one fixed order (per thread ascending, butterfly, waves ascending): the same bits on every call.
//
// NaN: a NaN reward is the chunk's arg-max (the first one, as torch.argmax and np.argmax have it) and makes max t, so every weight and the chunk's
// new sequence NaN (the clamp is two compares that keep one).  No other chunk reads it.
#include "../../include/adaptigraph_hip.h"
#include "ag_block_dev.h"
#include "ag_common.h"

#include <climits>

namespace {

constexpr int kMppiThreads = 256;
constexpr int kMppiWaves = kMppiThreads / 64;
constexpr int kMppiU = 4;      // samples per thread held in registers, and loads in flight per thread in a later trip

__device__ __forceinline__ float clamp_keep(float v, float lo, float hi)                              // min(v, hi) then max(., lo): NaN stays
{
    v = v > hi ? hi : v;
    return v < lo ? lo : v;
}

struct Best {
    float v;
    int i;
};
// the larger reward; NaN is the largest and the first NaN wins; equal rewards (+0 and -0 are equal): the lower index
__device__ __forceinline__ Best better(Best p, Best q)
{
    const bool pn = p.v != p.v, qn = q.v != q.v;
    const bool take_q = (pn || qn) ? (qn && (!pn || q.i < p.i)) : (q.v > p.v || (q.v == p.v && q.i < p.i));
    return take_q ? q : p;
}

// one action row (x, z, theta, length); the compiler makes the four words one 16-byte load
__device__ __forceinline__ float4 load_row(const float *p) { return make_float4(p[0], p[1], p[2], p[3]); }

struct Sums {
    float xs = 0.f, zs = 0.f, xe = 0.f, ze = 0.f;
};
// one sample's share of the weighted means of the push's start and end point (plan_utils.py:86-93)
__device__ __forceinline__ void add_sample(Sums &m, float w, float4 r, float push_length)
{
    const float reach = r.w * push_length;
    m.xs += w * r.x;
    m.zs += w * r.y;
    m.xe += w * (r.x - reach * cosf(r.z));
    m.ze += w * (r.y - reach * sinf(r.z));
}

__global__ __launch_bounds__(kMppiThreads) void mppi_update_kernel(const AgMppiArgs a)
{
    __shared__ float red_max[kMppiWaves], red_val[kMppiWaves], red_den[kMppiWaves], red_sum[4][kMppiWaves];
    __shared__ int red_idx[kMppiWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.S, L = a.L;
    const size_t chunk = blockIdx.x, row = (size_t)L * 4;
    const float *rew = a.reward + chunk * S;
    const float *act = a.actions + chunk * S * row;

    // the thread's first kMppiU samples: rewards and the rows of look-ahead index 0, all loads in flight together.  A slot past the end re-reads the
    // last sample and is kept out of every reduction by ok0[].
    float r0[kMppiU], e0[kMppiU];
    float4 v0[kMppiU];
    bool ok0[kMppiU];
#pragma unroll
    for (int k = 0; k < kMppiU; ++k) {
        const int s = tid + kMppiThreads * k;
        ok0[k] = s < S;
        const int sc = ok0[k] ? s : S - 1;
        r0[k] = rew[sc];
        v0[k] = load_row(act + (size_t)sc * row);
    }

    // pass 1: max of t = reward * reward_weight, and the arg-max of the reward
    float tmax = -INFINITY;
    Best best{-INFINITY, INT_MAX};      // (an index no sample has: a real -inf reward wins the tie against it)
#pragma unroll
    for (int k = 0; k < kMppiU; ++k) {
        if (ok0[k]) {
            tmax = nan_max(tmax, r0[k] * a.reward_weight);
            best = better(best, Best{r0[k], tid + kMppiThreads * k});
        }
    }
    for (int base = kMppiThreads * kMppiU; base < S; base += kMppiThreads * kMppiU) {
        float r[kMppiU];
#pragma unroll
        for (int k = 0; k < kMppiU; ++k) {
            const int s = base + kMppiThreads * k + tid;
            r[k] = rew[s < S ? s : S - 1];
        }
#pragma unroll
        for (int k = 0; k < kMppiU; ++k) {
            const int s = base + kMppiThreads * k + tid;
            if (s < S) {
                tmax = nan_max(tmax, r[k] * a.reward_weight);
                best = better(best, Best{r[k], s});
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        tmax = nan_max(tmax, __shfl_xor(tmax, o));
        best = better(best, Best{__shfl_xor(best.v, o), __shfl_xor(best.i, o)});
    }
    if (lane == 0) { red_max[wave] = tmax; red_val[wave] = best.v; red_idx[wave] = best.i; }
    __syncthreads();
    tmax = red_max[0];
    best = Best{red_val[0], red_idx[0]};
#pragma unroll
    for (int w = 1; w < kMppiWaves; ++w) {
        tmax = nan_max(tmax, red_max[w]);
        best = better(best, Best{red_val[w], red_idx[w]});
    }
    if (tid == 0) {
        if (a.best_idx) a.best_idx[chunk] = best.i;
        if (a.best_reward) a.best_reward[chunk] = best.v;
    }
    if (a.best_seq) {
        const float *src = act + (size_t)best.i * row;
        for (int i = tid; i < (int)row; i += kMppiThreads) a.best_seq[chunk * row + i] = src[i];
    }
    if (!a.new_seq) return;      // (uniform over the workgroup)

    // pass 2: e = exp(t - max t) and its sum
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < kMppiU; ++k) {
        e0[k] = ok0[k] ? expf(r0[k] * a.reward_weight - tmax) : 0.f;
        den += e0[k];
    }
    for (int base = kMppiThreads * kMppiU; base < S; base += kMppiThreads * kMppiU) {
        float r[kMppiU];
#pragma unroll
        for (int k = 0; k < kMppiU; ++k) {
            const int s = base + kMppiThreads * k + tid;
            r[k] = rew[s < S ? s : S - 1];
        }
#pragma unroll
        for (int k = 0; k < kMppiU; ++k) {
            const int s = base + kMppiThreads * k + tid;
            den += s < S ? expf(r[k] * a.reward_weight - tmax) : 0.f;
        }
    }
    den = wave_sum(den);
    if (lane == 0) red_den[wave] = den;
    __syncthreads();
    den = red_den[0];
#pragma unroll
    for (int w = 1; w < kMppiWaves; ++w) den += red_den[w];

    // pass 3, per look-ahead index: the weighted means of the push's ends, re-encoded and clipped
    for (int l = 0; l < L; ++l) {
        Sums m;
        if (l > 0) {
#pragma unroll
            for (int k = 0; k < kMppiU; ++k) {
                const int s = tid + kMppiThreads * k;
                v0[k] = load_row(act + (size_t)(ok0[k] ? s : S - 1) * row + 4 * l);
            }
        }
#pragma unroll
        for (int k = 0; k < kMppiU; ++k)
            if (ok0[k]) add_sample(m, e0[k] / den, v0[k], a.push_length);
        for (int base = kMppiThreads * kMppiU; base < S; base += kMppiThreads * kMppiU) {
            float r[kMppiU];
            float4 v[kMppiU];
#pragma unroll
            for (int k = 0; k < kMppiU; ++k) {
                const int s = base + kMppiThreads * k + tid, sc = s < S ? s : S - 1;
                r[k] = rew[sc];
                v[k] = load_row(act + (size_t)sc * row + 4 * l);
            }
#pragma unroll
            for (int k = 0; k < kMppiU; ++k) {
                const int s = base + kMppiThreads * k + tid;
                if (s < S) add_sample(m, expf(r[k] * a.reward_weight - tmax) / den, v[k], a.push_length);
            }
        }
        m.xs = wave_sum(m.xs); m.zs = wave_sum(m.zs); m.xe = wave_sum(m.xe); m.ze = wave_sum(m.ze);
        if (l > 0) __syncthreads();      // (thread 0 has read the sums of l - 1)
        if (lane == 0) { red_sum[0][wave] = m.xs; red_sum[1][wave] = m.zs; red_sum[2][wave] = m.xe; red_sum[3][wave] = m.ze; }
        __syncthreads();
        if (tid == 0) {
            float xs = red_sum[0][0], zs = red_sum[1][0], xe = red_sum[2][0], ze = red_sum[3][0];
#pragma unroll
            for (int w = 1; w < kMppiWaves; ++w) { xs += red_sum[0][w]; zs += red_sum[1][w]; xe += red_sum[2][w]; ze += red_sum[3][w]; }
            const float dx = xe - xs, dz = ze - zs;
            float theta = atan2f(zs - ze, xs - xe);
            const float len = sqrtf(dx * dx + dz * dz) / a.push_length;
            // angle_normalize (plan_utils.py:27-28) on float32 with pi rounded to float32, the remainder taking the divisor's sign
            const float pi = 3.14159265358979323846f, two_pi = 6.28318530717958647692f;
            float rem = fmodf(theta + pi, two_pi);
            if (rem != 0.f && rem < 0.f) rem += two_pi;
            theta = rem - pi;
            float *out = a.new_seq + chunk * row + 4 * l;
            out[0] = clamp_keep(xs, a.lo[0], a.hi[0]);
            out[1] = clamp_keep(zs, a.lo[1], a.hi[1]);
            out[2] = clamp_keep(theta, a.lo[2], a.hi[2]);
            out[3] = clamp_keep(len, a.lo[3], a.hi[3]);
        }
    }
}

}  // namespace

void ag_launch_mppi_update(const AgMppiArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(mppi_update_kernel, dim3(a.n_chunk), dim3(kMppiThreads), 0, s, a);
}
