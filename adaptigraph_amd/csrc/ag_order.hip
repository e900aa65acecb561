// ag_order.hip — the ordering of a ragged rollout (ag_rollout_order): the samples of a batch by non-increasing action_repeat, ties by ascending index,
// and per model step the number of samples still running.  ONE launch, no scratch, no host synchronisation: it stands in front of dynamics()'s one
// host read (forward_dynamics.py:156: n_steps = max(action_repeat)), so what counts is its latency, not its throughput.
//
// A counting sort over the keys 0 .. AG_ORDER_STEPS + 1 (negative repeats count as 0; everything above AG_ORDER_STEPS shares the last key).  Every
// workgroup owns 256 consecutive samples and builds, in LDS, the histogram of the WHOLE batch and the histogram of the samples in front of its own —
// B four-byte loads per workgroup, 80 KB at the planner's 20 000 samples, all L2 hits — so that no workgroup waits for another:
//   rank[b] = #{j : key[j] > key[b]}  +  #{j < b : key[j] == key[b]}
//           = suffix[key[b] + 1]      +  before[key[b]] + (equal keys among the workgroup's own samples in front of b)
// and active[s] = suffix[s + 1], written by workgroup 0.  Histograms are integer LDS atomics: the sums do not depend on their order, two calls give the
// same words.  Samples of the last key (repeat > AG_ORDER_STEPS: a batch the ragged rollout hands back to the plain call) are ranked among themselves
// by their value with a scan of the batch through LDS tiles, which only the workgroups that own such a sample run.
#include "ag_common.h"

namespace {

constexpr int kOrderKeys = AG_ORDER_STEPS + 2;      // 0 .. AG_ORDER_STEPS, and "above"
constexpr int kOrderBins = 1280;                    // >= kOrderKeys, five bins per thread of the suffix scan
static_assert(kOrderBins > kOrderKeys && kOrderBins == 5 * 256, "suffix[key + 1] is a bin for every key; 256 threads scan five bins each");
constexpr int kOrderLoads = 8;                     // loads a thread keeps in flight in the histogram pass

__device__ __forceinline__ int order_key(int r) { return r < 0 ? 0 : (r > AG_ORDER_STEPS ? AG_ORDER_STEPS + 1 : r); }

__global__ __launch_bounds__(256) void rollout_order_kernel(const int32_t *repeat, int B, int32_t *order, int32_t *active)
{
    __shared__ int all[kOrderBins], before[kOrderBins], part[256], own_key[256], tile[256];
    const int tid = threadIdx.x, b0 = blockIdx.x * 256, b = b0 + tid;
    for (int k = tid; k < kOrderBins; k += 256) { all[k] = 0; before[k] = 0; }
    const int mine = b < B ? repeat[b] : 0;
    const int key = order_key(mine);
    own_key[tid] = b < B ? key : -1;
    __syncthreads();
    // the two histograms: a thread's kOrderLoads loads are issued together, then counted
    for (int j0 = tid; j0 < B; j0 += 256 * kOrderLoads) {
        int r[kOrderLoads];
#pragma unroll
        for (int u = 0; u < kOrderLoads; ++u) r[u] = j0 + 256 * u < B ? repeat[j0 + 256 * u] : 0;
#pragma unroll
        for (int u = 0; u < kOrderLoads; ++u) {
            const int j = j0 + 256 * u;
            if (j < B) {
                const int k = order_key(r[u]);
                atomicAdd(&all[k], 1);
                if (j < b0) atomicAdd(&before[k], 1);
            }
        }
    }
    __syncthreads();
    // suffix[k] = #{j : key[j] >= k}, in place over `all`: five bins per thread, the threads' sums scanned from the back
    int loc[5], sum = 0;
#pragma unroll
    for (int i = 4; i >= 0; --i) { sum += all[tid * 5 + i]; loc[i] = sum; }
    part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int add = tid + o < 256 ? part[tid + o] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    const int behind = part[tid] - sum;      // the bins of the threads behind this one
#pragma unroll
    for (int i = 0; i < 5; ++i) all[tid * 5 + i] = loc[i] + behind;
    __syncthreads();
    if (blockIdx.x == 0)
        for (int s = tid; s <= AG_ORDER_STEPS; s += 256) active[s] = all[s + 1];
    // equal keys among the workgroup's own samples in front of this one
    int eq = 0;
    for (int j = 0; j < tid; ++j) eq += own_key[j] == key ? 1 : 0;
    int rank = all[key + 1] + before[key] + eq;
    // the last key: its samples are ordered by value.  rank = #{j : repeat[j] > mine} + #{j < b : repeat[j] == mine} over the whole batch
    const bool above = b < B && key == AG_ORDER_STEPS + 1;
    if (__syncthreads_or(above ? 1 : 0)) {
        int cnt = 0;
        for (int j0 = 0; j0 < B; j0 += 256) {
            __syncthreads();
            tile[tid] = j0 + tid < B ? repeat[j0 + tid] : 0;
            __syncthreads();
            const int n = B - j0 < 256 ? B - j0 : 256;
            if (above)
                for (int j = 0; j < n; ++j) cnt += (tile[j] > mine || (tile[j] == mine && j0 + j < b)) ? 1 : 0;
        }
        if (above) rank = cnt;
    }
    if (b < B && (unsigned)rank < (unsigned)B) order[rank] = b;      // (rank counts samples other than b: below B unless `repeat` changes under the kernel)
}

}  // namespace

void ag_launch_rollout_order(const int32_t *repeat, int B, int32_t *order, int32_t *active, hipStream_t s)
{
    hipLaunchKernelGGL(rollout_order_kernel, dim3((B + 255) / 256), dim3(256), 0, s, repeat, B, order, active);
}
