// ag_rollout.hip — per-step state update of the batched rollout, entirely on device.
//
// Replaces the tail of the inner loop of dynamics() / dynamics_masked()
// (src/planning/forward_dynamics.py:160-176 / :356-372):
//     pred_state_seq[repeat == ai] = pred_state                       record-on-repeat
//     y_cur   = min_i pred_y            (dynamics, :163)   |  masked mean (dynamics_masked, :359)
//     eef_cur = state[-1, tools] + action[tools]; eef_cur.y = y_cur (+ gripper raise)   (:164-168)
//     state   = cat([state[1:], cat([pred_state, eef_cur])])           history shift     (:170,176)
// A sample is updated by ceil(3N / 2048) workgroups (grid.y), each of which re-derives the sample's tool height from the predicted
// positions itself (a 4-16 KB L2-resident read: cheaper than a second launch or a grid-wide hand-off; with ONE workgroup per sample the
// 64-sample cloth-4k launch used a quarter of the CUs: 0.077 ms); no host synchronisation (the reference syncs via .item() every step).
#include "ag_block_dev.h"
#include "ag_common.h"

namespace {

constexpr int kStepChunk = 2048;     // plane elements per workgroup

// SHARED (compile time: the plain rollout keeps its direct indexing — the map costs it 25 % of this launch): the shared-state rollout of ag_shared.hip
template <bool SHARED>
__global__ __launch_bounds__(256) void rollout_step_kernel(AgStepArgs a)
{
    __shared__ float red[2][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // prediction of particle i, component c: by (sample, particle), or — shared-state rollout — by compact row through cmap (a private row or the base's)
    const float *pred = a.pred_pos + (SHARED ? (size_t)0 : (size_t)b * a.n_p * 3);
    const int32_t *cm = SHARED ? a.cmap + (size_t)b * a.N : nullptr;
    auto at = [&](int i, int c) { return SHARED ? pred[(size_t)cm[i] * 3 + c] : pred[i * 3 + c]; };

    float y;
    if (a.height_mode == 0) {
        float m = INFINITY;
        for (int i = tid; i < a.n_p; i += 256) m = fminf(m, at(i, 1));
        m = wave_fmin(m);
        if (lane == 0) red[0][wave] = m;
        __syncthreads();
        y = four_wave_min(red[0]);
    } else {
        const uint8_t *mk = a.obj_mask + (size_t)b * a.n_p;
        float sc[2] = {0.f, 0.f};      // masked sum of the heights, mask count
        for (int i = tid; i < a.n_p; i += 256) {
            const float w = mk[i] ? 1.f : 0.f;
            sc[0] += at(i, 1) * w;
            sc[1] += w;
        }
        four_wave_park(sc, red, lane, wave);
        __syncthreads();
        y = four_wave_total(red[0]) / four_wave_total(red[1]);
    }
    y += a.raise;

    const int plane = a.N * 3;
    const int k0 = blockIdx.y * kStepChunk, k1 = min(k0 + kStepChunk, plane);
    if (a.repeat[b] == a.step && !(SHARED && b == 0)) {
        int row = SHARED ? b - 1 : b;      // (shared-state rollout: internal sample b is the caller's b - 1; the base records nothing)
        bool ok = true;
        if (a.out_index) {                 // ragged rollout: the caller's row of this sample (uniform over the workgroup)
            row = a.out_index[row];
            ok = (unsigned)row < (unsigned)a.out_rows;
            if (!ok && tid == 0 && blockIdx.y == 0) atomicOr(a.status, AG_STATUS_ORDER_BIT);
        }
        float *o = a.out_seq + (size_t)row * a.n_p * 3;
        if (ok)
            for (int k = k0 + tid; k < min(k1, a.n_p * 3); k += 256) o[k] = SHARED ? at(k / 3, k % 3) : pred[k];
    }
    float *st = a.state + (size_t)b * a.H * a.N * 3;
    const float *dl = a.delta + (size_t)b * a.N * 3;
    // shared-state rollout: a private prediction that differs from the base's in any bit makes the particle dirty from the next step on
    auto mark = [&](int n, int c, float v) {
        if constexpr (SHARED)
            if (b > 0 && cm[n] != n && __float_as_uint(v) != __float_as_uint(pred[(size_t)n * 3 + c])) { a.dirty[(size_t)b * a.N + n] = 1; a.sample_dirty[b] = 1; }
    };
    if (a.H == AG_NHIS) {
        // all of this thread's loads first, then its stores: `st` is read and written, so a plain loop orders every iteration's loads behind the
        // previous iteration's stores — eight dependent memory round trips per thread (17 us per launch at C2; 8 us this way)
        constexpr int kPer = kStepChunk / 256;
        float v[kPer][AG_NHIS], nv[kPer];
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int k = k0 + tid + 256 * i;
            if (k < k1) {
#pragma unroll
                for (int h = 1; h < AG_NHIS; ++h) v[i][h] = st[(size_t)h * plane + k];
                const int n = k / 3, c = k - n * 3;
                nv[i] = n < a.n_p ? (SHARED ? at(n, c) : pred[k]) : (c == 1 ? y : v[i][AG_NHIS - 1] + dl[k]);
                if (n < a.n_p) mark(n, c, nv[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int k = k0 + tid + 256 * i;
            if (k < k1) {
#pragma unroll
                for (int h = 0; h + 1 < AG_NHIS; ++h) st[(size_t)h * plane + k] = v[i][h + 1];
                st[(size_t)(AG_NHIS - 1) * plane + k] = nv[i];
            }
        }
        return;
    }
    for (int k = k0 + tid; k < k1; k += 256) {
        const int n = k / 3, c = k - n * 3;
        const float last = st[(size_t)(a.H - 1) * plane + k];
        for (int h = 0; h + 1 < a.H; ++h) st[(size_t)h * plane + k] = st[(size_t)(h + 1) * plane + k];
        float nv;
        if (n < a.n_p) { nv = SHARED ? at(n, c) : pred[k]; mark(n, c, nv); }
        else nv = (c == 1) ? y : last + dl[k];
        st[(size_t)(a.H - 1) * plane + k] = nv;
    }
}

// Ragged rollout, behind the last step (ag_common.h: ag_launch_ragged_finish).  grid (B, chunks of a sample's H N 3 floats)
__global__ __launch_bounds__(256) void ragged_finish_kernel(const float *state, const int32_t *repeat, const int32_t *out_index, float *state_final,
                                                           int B, int per, int *status)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const int row = out_index ? out_index[b] : b;
    const bool ok = (unsigned)row < (unsigned)B;
    if (tid == 0 && blockIdx.y == 0) {
        const int r = max(repeat[b], 0), before = b > 0 ? max(repeat[b - 1], 0) : r;
        if (!ok || before < r) atomicOr(status, AG_STATUS_ORDER_BIT);
    }
    if (!ok || !state_final) return;
    const float *src = state + (size_t)b * per;
    float *dst = state_final + (size_t)row * per;
    constexpr int kPer = kStepChunk / 256;
    const int k0 = blockIdx.y * kStepChunk + tid;
    float v[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) v[i] = k0 + 256 * i < per ? src[k0 + 256 * i] : 0.f;
#pragma unroll
    for (int i = 0; i < kPer; ++i)
        if (k0 + 256 * i < per) dst[k0 + 256 * i] = v[i];
}

}  // namespace

void ag_launch_ragged_finish(const float *state, const int32_t *repeat, const int32_t *out_index, float *state_final, int B, int H, int N, int *status,
                             hipStream_t s)
{
    const int per = H * N * 3;
    hipLaunchKernelGGL(ragged_finish_kernel, dim3(B, (per + kStepChunk - 1) / kStepChunk), dim3(256), 0, s, state, repeat, out_index, state_final, B, per,
                       status);
}

// Zero a few device words with a KERNEL instead of hipMemsetAsync: inside a captured HIP graph the memset NODES of the shared-state rollout were not
// reliably replayed (second replay of tests' graph: garbage; eager calls and the first replay fine), kernel nodes are.
__global__ void zero_words_kernel(int32_t *p, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0;
}
void ag_launch_zero_words(int32_t *p, int n, hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(zero_words_kernel, dim3((n + 255) / 256), dim3(256), 0, s, p, n);
}

void ag_launch_rollout_step(const AgStepArgs &a, hipStream_t s)
{
    const dim3 grid(a.B, (a.N * 3 + kStepChunk - 1) / kStepChunk);
    if (a.cmap) hipLaunchKernelGGL(rollout_step_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(rollout_step_kernel<false>, grid, dim3(256), 0, s, a);
}
