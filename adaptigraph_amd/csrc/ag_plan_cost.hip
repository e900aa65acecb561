// ag_plan_cost.hip — everything of the planner's running_cost (src/planning/plan.py:27-59) but the error term's own kernel: the penalties and
// box_loss of src/planning/losses.py:26-92, the workspace-bounds term and the reward, with every predicted cloud read once.
//
// plan_terms_kernel: one 64-lane wave per (b, l) cloud of state_seqs (B, L, n, 3), four waves per workgroup, no LDS, no atomics.  The lanes stride
// over the particles (x and z only: nothing in the cost reads y), kPlanU trips of loads in flight per lane, and while a particle is in registers it
// feeds the cloud's extents, box_loss (when selected) and the squared distance to the pusher of the NEXT push, l + 1 — the cloud "before push l + 1"
// of losses.py:42-43 is this one.  The wave of l = 0 also sweeps state_init (n, 3; shared by all samples, so it stays in cache) against push 0, and
// for cloth every wave sweeps state_init against its own push (losses.py:50-64 reads nothing else).  sqrt is monotone: the square root of the
// smallest squared distance is the smallest distance, bit for bit (the argument of ag_cost.hip).  Every word of the term table has one writer.
//
// plan_reward_kernel: one workgroup; max(error) and (cloth) max(dmax) over all (b, l), then the reward per sample exactly as plan.py:37 and 53 write
// it.  Every sum and every reduction has one fixed order: the same bits on every call.
//
// plan_reward_chunk_kernel (ag_plan_cost_chunked): the same device function, one workgroup per chunk of S samples over that chunk's rows of the
// table — each thread meets the rows it would meet in a call on the chunk alone, in the same order, so the chunk's rewards are that call's bits.
//
// NaN: torch's min / max / mean / clamp carry a NaN, fminf / fmaxf drop it.  The reductions below are written as compares that keep one
// (nan_min / nan_max of ag_block_dev.h, keep_pos, cap_at), so that a diverged sample gets a NaN reward as in the reference, never a good one.
#include "../../include/adaptigraph_hip.h"
#include "ag_block_dev.h"
#include "ag_common.h"

namespace {

constexpr int kPlanWaves = 4;      // clouds per workgroup
constexpr int kPlanU = 4;          // particles per lane in flight
constexpr int kRewardThreads = 1024;

__device__ __forceinline__ float keep_pos(float v) { return v < 0.f ? 0.f : v; }                      // clamp_min(0): NaN stays
__device__ __forceinline__ float cap_at(float v, float c) { return v > c ? c : v; }                   // clamp_max(c): NaN stays

struct Sweep {
    float xlo = INFINITY, xhi = -INFINITY, zlo = INFINITY, zhi = -INFINITY;
    float box_sum = 0.f;
    float near = INFINITY, far = -INFINITY;      // squared
};

// the pusher points of one action (x_start, z_start, theta, length): its start (rope, cloth), or nine points along the flat pusher (granular)
template <int NP>
__device__ __forceinline__ void pusher_points(const float *act, float rad, float (&px)[NP], float (&pz)[NP])
{
    if constexpr (NP == 1) {
        px[0] = act[0];
        pz[0] = act[1];
    } else {
        const float dx = rad * sinf(act[2]), dz = -rad * cosf(act[2]);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const float off = -1.f + 0.25f * (float)k;
            px[k] = act[0] + off * dx;
            pz[k] = act[1] + off * dz;
        }
    }
}

// one pass of a wave over a cloud of n particles.  EXT: extents; BOX: the box_loss sum; NP > 0: nearest (FAR: and farthest) squared distance to the
// points.  A lane past the end re-reads the last particle (min and max do not mind; the sum skips it), so that the loads of a trip are unconditional.
template <int NP, bool EXT, bool BOX, bool FAR>
__device__ __forceinline__ void sweep(const float *cloud, int n, int lane, const float *px, const float *pz, const float *box, Sweep &s)
{
    for (int base = 0; base < n; base += 64 * kPlanU) {
        float x[kPlanU], z[kPlanU];
        bool ok[kPlanU];
#pragma unroll
        for (int k = 0; k < kPlanU; ++k) {
            const int i = base + 64 * k + lane;
            ok[k] = i < n;
            const float *p = cloud + (size_t)3 * (ok[k] ? i : n - 1);
            x[k] = p[0];
            z[k] = p[2];
        }
#pragma unroll
        for (int k = 0; k < kPlanU; ++k) {
            if constexpr (EXT) {
                s.xlo = nan_min(s.xlo, x[k]); s.xhi = nan_max(s.xhi, x[k]);
                s.zlo = nan_min(s.zlo, z[k]); s.zhi = nan_max(s.zhi, z[k]);
            }
            if constexpr (BOX) {
                const float dx = keep_pos(box[0] - x[k]) + keep_pos(x[k] - box[1]);
                const float dz = keep_pos(box[2] - z[k]) + keep_pos(z[k] - box[3]);
                const float d = sqrtf(dx * dx + dz * dz);
                s.box_sum += ok[k] ? d : 0.f;
            }
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const float dx = px[q] - x[k], dz = pz[q] - z[k];
                const float d2 = dx * dx + dz * dz;
                s.near = nan_min(s.near, d2);
                if constexpr (FAR) s.far = nan_max(s.far, d2);
            }
        }
    }
}

__device__ __forceinline__ float touch_term(float d, float touch) { return expf(-keep_pos(d - touch) * 100.0f); }

template <int PEN, bool BOX>
__global__ __launch_bounds__(64 * kPlanWaves) void plan_terms_kernel(const AgPlanCostArgs a)
{
    constexpr int NP = PEN == AG_PENALTY_GRANULAR ? 9 : 1;
    constexpr bool kPush = PEN == AG_PENALTY_ROPE || PEN == AG_PENALTY_GRANULAR;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long c = (long long)blockIdx.x * kPlanWaves + wave;
    if (c >= (long long)a.B * a.L) return;      // (no barrier in this kernel)
    const int b = (int)(c / a.L), l = (int)(c - (long long)b * a.L);
    const float *cloud = a.state_seqs + (size_t)c * a.n * 3;
    const float *act = a.action + (size_t)c * 4;
    float px[NP], pz[NP];
    Sweep own, init;
    const bool has_next = kPush && l + 1 < a.L;
    if (has_next) {
        pusher_points<NP>(act + 4, a.rad, px, pz);
        sweep<NP, true, BOX, false>(cloud, a.n, lane, px, pz, a.box, own);
    } else {
        sweep<0, true, BOX, false>(cloud, a.n, lane, px, pz, a.box, own);
    }
    if constexpr (kPush) {
        if (l == 0) {
            pusher_points<NP>(act, a.rad, px, pz);
            sweep<NP, false, false, false>(a.state_init, a.n, lane, px, pz, a.box, init);
        }
    }
    if constexpr (PEN == AG_PENALTY_CLOTH) {
        pusher_points<1>(act, a.rad, px, pz);
        sweep<1, false, false, true>(a.state_init, a.n, lane, px, pz, a.box, init);
    }
    const float xlo = wave_nan_min(own.xlo), xhi = wave_nan_max(own.xhi), zlo = wave_nan_min(own.zlo), zhi = wave_nan_max(own.zhi);
    const float box_sum = BOX ? wave_sum(own.box_sum) : 0.f;
    const float near_next = kPush ? wave_nan_min(own.near) : 0.f;
    const float near_init = PEN != AG_PENALTY_NONE ? wave_nan_min(init.near) : 0.f;
    const float far_init = PEN == AG_PENALTY_CLOTH ? wave_nan_max(init.far) : 0.f;
    if (lane != 0) return;
    float *t = a.terms + (size_t)c * AG_PLAN_TERMS;
    t[0] = BOX ? box_sum / (float)a.n : a.error_in[c];
    const float m0 = xlo - a.bbox[0], m1 = a.bbox[1] - xhi, m2 = zlo - a.bbox[2], m3 = a.bbox[3] - zhi;
    t[2] = nan_max(nan_max(expf(-keep_pos(m0) * 100.0f), expf(-keep_pos(m1) * 100.0f)),
                   nan_max(expf(-keep_pos(m2) * 100.0f), expf(-keep_pos(m3) * 100.0f)));
    t[5] = xlo; t[6] = xhi; t[7] = zlo; t[8] = zhi;
    if constexpr (PEN == AG_PENALTY_NONE) { t[1] = 0.f; t[3] = 0.f; t[4] = 0.f; }
    if constexpr (kPush) {
        t[4] = 0.f;
        if (has_next) {                          // this cloud is the one before push l + 1
            const float d = sqrtf(near_next);
            t[AG_PLAN_TERMS + 3] = d;
            t[AG_PLAN_TERMS + 1] = touch_term(d, a.touch);
        }
        if (l == 0) {
            const float d = sqrtf(near_init);
            t[3] = d;
            t[1] = touch_term(d, a.touch);
        }
    }
    if constexpr (PEN == AG_PENALTY_CLOTH) {      // (the collision term needs max(dmax) over the whole call: plan_reward_kernel)
        t[3] = sqrtf(near_init);
        t[4] = sqrtf(far_init);
    }
}

// the rewards of the nb samples from b0 on, by one workgroup: both maxima are taken over these samples' rows of the table and over no others
template <bool CLOTH>
__device__ __forceinline__ void plan_reward_rows(const AgPlanCostArgs &a, int b0, int nb)
{
    __shared__ float red[2][kRewardThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long c0 = (long long)b0 * a.L, BL = (long long)nb * a.L;
    float emax = -INFINITY, fmax_ = -INFINITY;
    for (long long c = tid; c < BL; c += kRewardThreads) {
        const float *t = a.terms + (size_t)(c0 + c) * AG_PLAN_TERMS;
        emax = nan_max(emax, t[0]);
        if constexpr (CLOTH) fmax_ = nan_max(fmax_, cap_at(t[4], a.far_cap));
    }
    emax = wave_nan_max(emax);
    if constexpr (CLOTH) fmax_ = wave_nan_max(fmax_);
    if (lane == 0) { red[0][wave] = emax; red[1][wave] = fmax_; }
    __syncthreads();
    emax = red[0][0];
    fmax_ = red[1][0];
#pragma unroll
    for (int w = 1; w < kRewardThreads / 64; ++w) { emax = nan_max(emax, red[0][w]); fmax_ = nan_max(fmax_, red[1][w]); }
    const float weight = 2.0f / (emax + 1e-6f);
    const float count = (float)a.L;
    for (int b = b0 + tid; b < b0 + nb; b += kRewardThreads) {
        float *t = a.terms + (size_t)b * a.L * AG_PLAN_TERMS;
        float csum = 0.f, bsum = 0.f, err = 0.f;
        for (int l = 0; l < a.L; ++l, t += AG_PLAN_TERMS) {
            float col;
            if constexpr (CLOTH) {      // (this is the term's one writer: nothing has been stored there yet)
                const float dmin = keep_pos(t[3] - a.grasp), dmax = cap_at(t[4], a.far_cap) / fmax_;
                col = (1.0f - expf(-dmin * 100.0f)) - dmax * 0.2f;
                t[1] = col;
            } else {
                col = t[1];
            }
            csum += col;
            bsum += t[2];
            err = t[0];      // (the last step's is the one the reward reads)
        }
        a.reward[b] = (-weight * err - 5.0f * (csum / count)) - 5.0f * (bsum / count);
    }
}

template <bool CLOTH>
__global__ __launch_bounds__(kRewardThreads) void plan_reward_kernel(const AgPlanCostArgs a)
{
    plan_reward_rows<CLOTH>(a, 0, a.B);
}

// the planner's chunks (plan.py:241-247: one trajectory_optimization each): workgroup c scores the S samples of chunk c as a call of their own
template <bool CLOTH>
__global__ __launch_bounds__(kRewardThreads) void plan_reward_chunk_kernel(const AgPlanCostArgs a, int S)
{
    plan_reward_rows<CLOTH>(a, blockIdx.x * S, S);
}

template <int PEN>
void launch_terms(const AgPlanCostArgs &a, dim3 grid, hipStream_t s)
{
    if (a.box_criterion) hipLaunchKernelGGL((plan_terms_kernel<PEN, true>), grid, dim3(64 * kPlanWaves), 0, s, a);
    else hipLaunchKernelGGL((plan_terms_kernel<PEN, false>), grid, dim3(64 * kPlanWaves), 0, s, a);
}

}  // namespace

void ag_launch_plan_cost(const AgPlanCostArgs &a, int n_chunk, hipStream_t s)
{
    const long long BL = (long long)a.B * a.L;
    const dim3 grid((unsigned)((BL + kPlanWaves - 1) / kPlanWaves));
    switch (a.penalty) {
    case AG_PENALTY_ROPE: launch_terms<AG_PENALTY_ROPE>(a, grid, s); break;
    case AG_PENALTY_CLOTH: launch_terms<AG_PENALTY_CLOTH>(a, grid, s); break;
    case AG_PENALTY_GRANULAR: launch_terms<AG_PENALTY_GRANULAR>(a, grid, s); break;
    default: launch_terms<AG_PENALTY_NONE>(a, grid, s); break;
    }
    const bool cloth = a.penalty == AG_PENALTY_CLOTH;
    if (n_chunk > 1) {
        const int S = a.B / n_chunk;
        if (cloth) hipLaunchKernelGGL(plan_reward_chunk_kernel<true>, dim3(n_chunk), dim3(kRewardThreads), 0, s, a, S);
        else hipLaunchKernelGGL(plan_reward_chunk_kernel<false>, dim3(n_chunk), dim3(kRewardThreads), 0, s, a, S);
    } else if (cloth) {
        hipLaunchKernelGGL(plan_reward_kernel<true>, dim3(1), dim3(kRewardThreads), 0, s, a);
    } else {
        hipLaunchKernelGGL(plan_reward_kernel<false>, dim3(1), dim3(kRewardThreads), 0, s, a);
    }
}
