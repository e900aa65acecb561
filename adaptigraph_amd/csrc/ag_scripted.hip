// ag_scripted.hip — per-step state update of the SCRIPTED rollout (ag_rollout_scripted), entirely on device.
//
// Replaces the tail of the step loop of the reference's evaluation rollout (src/dynamics/rollout/rollout.py:62-93 with the frame walk of
// src/dynamics/rollout/graph.py:373-399 resolved up front):
//     pred_seq[:, t] = pred                                                      every step recorded
//     err[:, t]      = sum_i obj_mask * ||pred - gt[:, t]|| / max(sum obj_mask, 1) mean key-point error
//     state          = cat([state[1:], cat([pred, tool_pos[:, t + 1]])])         history shift, tool placed absolutely from the script
//     action         = [0 (objects) | tool_delta[:, t + 1]]                      next step's node input
// Unlike rollout_step_kernel (ag_rollout.hip) the tool is not advanced by last + delta and has no height rule; the last step reads no script
// entry and leaves state and action as its forward saw them.  A sample is updated by ceil(3N / 2048) workgroups (grid.y); the error sum is
// taken by the first of them alone, in one fixed order: no atomics, no memset, no second launch, the same bits every call.
#include "ag_block_dev.h"
#include "ag_common.h"

namespace {

constexpr int kStepChunk = 2048;     // plane elements per workgroup

__global__ __launch_bounds__(256) void scripted_step_kernel(AgScriptArgs a)
{
    __shared__ float red[2][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *pred = a.pred_pos + (size_t)b * a.n_p * 3;
    const size_t bt = (size_t)b * a.T + a.t;

    if (a.gt && blockIdx.y == 0) {
        // thread: its points in ascending order; wave and workgroup: the fixed order of ag_block_dev.h
        const float *g = a.gt + bt * a.n_p * 3;
        const uint8_t *mk = a.obj_mask ? a.obj_mask + (size_t)b * a.n_p : nullptr;
        float sc[2] = {0.f, 0.f};      // sum of the errors, count of the points
        for (int i = tid; i < a.n_p; i += 256) {
            if (mk && !mk[i]) continue;
            const float dx = pred[i * 3] - g[i * 3], dy = pred[i * 3 + 1] - g[i * 3 + 1], dz = pred[i * 3 + 2] - g[i * 3 + 2];
            sc[0] += sqrtf((dx * dx + dy * dy) + dz * dz);
            sc[1] += 1.f;
        }
        four_wave_park(sc, red, lane, wave);
        __syncthreads();
        if (tid == 0) a.err[bt] = four_wave_total(red[0]) / fmaxf(four_wave_total(red[1]), 1.f);
    }

    const int plane = a.N * 3, obj = a.n_p * 3;
    const int k0 = blockIdx.y * kStepChunk, k1 = min(k0 + kStepChunk, plane);
    if (a.pred_seq) {
        float *o = a.pred_seq + bt * obj;
        for (int k = k0 + tid; k < min(k1, obj); k += 256) o[k] = pred[k];
    }
    if (a.t + 1 >= a.T) return;

    const int tool = plane - obj;
    const size_t script = (bt + 1) * tool;      // entry t + 1 of sample b
    float *st = a.state + (size_t)b * AG_NHIS * plane;
    float *act = a.action + (size_t)b * plane;
    // all of this thread's loads first, then its stores: `st` is read and written (rollout_step_kernel)
    constexpr int kPer = kStepChunk / 256;
    float v[kPer][AG_NHIS], nv[kPer], na[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int k = k0 + tid + 256 * i;
        if (k < k1) {
#pragma unroll
            for (int h = 1; h < AG_NHIS; ++h) v[i][h] = st[(size_t)h * plane + k];
            nv[i] = k < obj ? pred[k] : a.tool_pos[script + (k - obj)];
            na[i] = k < obj ? 0.f : a.tool_delta[script + (k - obj)];
        }
    }
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int k = k0 + tid + 256 * i;
        if (k < k1) {
#pragma unroll
            for (int h = 0; h + 1 < AG_NHIS; ++h) st[(size_t)h * plane + k] = v[i][h + 1];
            st[(size_t)(AG_NHIS - 1) * plane + k] = nv[i];
            act[k] = na[i];
        }
    }
}

}  // namespace

void ag_launch_scripted_step(const AgScriptArgs &a, hipStream_t s)
{
    const dim3 grid(a.B, (a.N * 3 + kStepChunk - 1) / kStepChunk);
    hipLaunchKernelGGL(scripted_step_kernel, grid, dim3(256), 0, s, a);
}
