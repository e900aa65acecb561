// ag_step_update.hip — the tail of a model step of the DIFFERENTIABLE rollouts (ag_step_update_forward / ag_step_update_backward): what
// rollout_step_kernel (ag_rollout.hip) does in place for the no-grad drivers, out of place for autograd, and its adjoint.  One launch each way.
//
//     rec_out = repeat == step ? pred : rec                                   record-on-repeat        (forward_dynamics.py:160-161 / :356-357)
//     y       = min_i pred_y | masked mean of pred_y ; + raise                tool height             (:163 / :359, :167-168)
//     tool    = state[-1, tools] + delta[tools]; tool.y = y                                           (:164-168 / :360-364)
//     state_out = cat([state[1:], cat([pred, tool])])                         history shift           (:170,176 / :366,372)
//
// grid (B, chunks of kStepChunk plane elements), as rollout_step_kernel: every workgroup of a sample re-derives the sample's height (forward) or
// the height's adjoint (backward: the sum G of the tool rows' y gradients, and the arg-min or the mask count) from L2-resident rows.  Sums run in
// the order of rollout_step_kernel — thread-strided partials, the xor butterfly, (w0 + w1) + (w2 + w3) — so the masked mean has the engine's bits;
// every output element has one writer and one fixed order of additions: no atomics.
#include "ag_block_dev.h"
#include "ag_common.h"

namespace {

constexpr int kStepChunk = 2048;     // plane elements per workgroup

__device__ __forceinline__ int min2i(int a, int b) { return a < b ? a : b; }

// min_i pred[i].y over a sample (fminf: a NaN is dropped), in every thread.  One barrier; red is free again after the caller's next barrier.
__device__ __forceinline__ float sample_min_y(const float *pred, int n_p, float *red, int tid)
{
    float m = INFINITY;
    for (int i = tid; i < n_p; i += 256) m = fminf(m, pred[i * 3 + 1]);
    m = wave_fmin(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    return four_wave_min(red);
}

__global__ __launch_bounds__(256) void step_update_fwd_kernel(AgStepUpdateArgs a)
{
    __shared__ float red[2][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *pred = a.pred + (size_t)b * a.n_p * 3;
    float y;
    if (a.height_mode == 0) {
        y = sample_min_y(pred, a.n_p, red[0], tid);
    } else {
        const uint8_t *mk = a.obj_mask + (size_t)b * a.n_p;
        float sc[2] = {0.f, 0.f};      // masked sum of the heights, mask count
        for (int i = tid; i < a.n_p; i += 256) {
            const float w = mk[i] ? 1.f : 0.f;
            sc[0] += pred[i * 3 + 1] * w;
            sc[1] += w;
        }
        four_wave_park(sc, red, lane, wave);
        __syncthreads();
        y = four_wave_total(red[0]) / four_wave_total(red[1]);
    }
    y += a.raise;

    const int plane = a.N * 3, np3 = a.n_p * 3;
    const int k0 = blockIdx.y * kStepChunk, k1 = min(k0 + kStepChunk, plane);
    const bool record = a.repeat[b] == a.step;
    const float *rec = a.rec ? a.rec + (size_t)b * np3 : nullptr;
    float *rec_out = a.rec_out + (size_t)b * np3;
    const float *st = a.state + (size_t)b * a.H * plane;
    const float *dl = a.delta + (size_t)b * plane;
    float *so = a.state_out + (size_t)b * a.H * plane;
    for (int k = k0 + tid; k < k1; k += 256) {
        const int n = k / 3, c = k - n * 3;
        float nv;
        if (k < np3) {
            nv = pred[k];
            rec_out[k] = record ? nv : (rec ? rec[k] : 0.f);
        } else {
            nv = c == 1 ? y : st[(size_t)(a.H - 1) * plane + k] + dl[k];
        }
        for (int h = 0; h + 1 < a.H; ++h) so[(size_t)h * plane + k] = st[(size_t)(h + 1) * plane + k];
        so[(size_t)(a.H - 1) * plane + k] = nv;
    }
}

__global__ __launch_bounds__(256) void step_update_bwd_kernel(AgStepUpdateArgs a)
{
    __shared__ float red[2][4];
    __shared__ int redi[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int plane = a.N * 3, np3 = a.n_p * 3;
    const float *pred = a.pred + (size_t)b * np3;
    const float *go = a.g_state_out + (size_t)b * a.H * plane;
    const float *g_new = go + (size_t)(a.H - 1) * plane;        // gradient of the newest frame
    const uint8_t *mk = a.height_mode == 0 ? nullptr : a.obj_mask + (size_t)b * a.n_p;

    // G = sum over the tool rows of the newest frame's y gradient; the mask count rides along
    float sc[2] = {0.f, 0.f};
    for (int n = a.n_p + tid; n < a.N; n += 256) sc[0] += g_new[n * 3 + 1];
    if (mk)
        for (int i = tid; i < a.n_p; i += 256) sc[1] += mk[i] ? 1.f : 0.f;
    four_wave_park(sc, red, lane, wave);
    __syncthreads();
    const float G = four_wave_total(red[0]);
    const float share = mk ? G / four_wave_total(red[1]) : G;   // d y / d pred_y of a masked-in particle is 1 / count
    int first = -1;                                             // AG_HEIGHT_MIN: the first particle at the minimum takes G
    if (!mk) {
        __syncthreads();                                        // red is read above and written below
        const float m = sample_min_y(pred, a.n_p, red[0], tid);
        int f = 0x7fffffff;
        for (int i = tid; i < a.n_p; i += 256)
            if (pred[i * 3 + 1] == m) f = min2i(f, i);
        f = wave_reduce<int, min2i>(f);
        if (lane == 0) redi[wave] = f;
        __syncthreads();
        first = min2i(min2i(redi[0], redi[1]), min2i(redi[2], redi[3]));
    }

    const int k0 = blockIdx.y * kStepChunk, k1 = min(k0 + kStepChunk, plane);
    const bool record = a.repeat[b] == a.step;
    const float *g_rec_out = a.g_rec_out ? a.g_rec_out + (size_t)b * np3 : nullptr;
    float *g_pred = a.g_pred + (size_t)b * np3;
    float *g_rec = a.g_rec ? a.g_rec + (size_t)b * np3 : nullptr;
    float *gs = a.g_state + (size_t)b * a.H * plane;
    float *gd = a.g_delta + (size_t)b * plane;
    for (int k = k0 + tid; k < k1; k += 256) {
        const int n = k / 3, c = k - n * 3;
        const float gn = g_new[k];
        float through = 0.f;                                    // the tool rows' x and z pass through to state[-1] and delta
        if (k < np3) {
            const float gr = g_rec_out ? g_rec_out[k] : 0.f;
            float g = gn + (record ? gr : 0.f);
            if (c == 1) g += mk ? (mk[n] ? share : 0.f) : (n == first ? G : 0.f);
            g_pred[k] = g;
            if (g_rec) g_rec[k] = record ? 0.f : gr;
        } else if (c != 1) {
            through = gn;
        }
        gd[k] = through;
        gs[k] = a.H > 1 ? 0.f : through;                        // the oldest frame's gradient is dropped by the shift
        for (int h = 1; h + 1 < a.H; ++h) gs[(size_t)h * plane + k] = go[(size_t)(h - 1) * plane + k];
        if (a.H > 1) gs[(size_t)(a.H - 1) * plane + k] = go[(size_t)(a.H - 2) * plane + k] + through;
    }
}

}  // namespace

void ag_launch_step_update(const AgStepUpdateArgs &a, int backward, hipStream_t s)
{
    const dim3 grid(a.B, (a.N * 3 + kStepChunk - 1) / kStepChunk);
    if (backward) hipLaunchKernelGGL(step_update_bwd_kernel, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(step_update_fwd_kernel, grid, dim3(256), 0, s, a);
}
