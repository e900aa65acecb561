// ag_block_dev.h — the wave (64 lanes) and workgroup (256 threads = four waves; block_min_u64: up to sixteen waves) collectives of the
// kernels, written once.  No kernels here and nothing of the engine.  What each primitive guarantees, and every caller relies on:
//   integers  — ranks, counts, scans, offsets: exact, whatever the order of the additions.
//   floats    — ONE fixed order, so a result is the same bits on every call and in a replayed graph: a thread's own accumulation is the
//               caller's; a wave is the xor butterfly with offsets 32, 16, .. 1; the four wave values of a workgroup are (w0 + w1) + (w2 + w3),
//               or the same nesting of fminf.  min and max are exact in any order; the NaN-keeping and the plain forms differ in what a NaN does.
//   barriers  — part of each primitive's contract, stated with it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// ---- wave reductions: the result in every lane ----
template <typename T, T (*F)(T, T)>      // F: the combining operation
__device__ __forceinline__ T wave_reduce(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = F(v, __shfl_xor(v, o));
    return v;
}
template <typename T>
__device__ __forceinline__ T add2(T a, T b) { return a + b; }
template <typename T>
__device__ __forceinline__ T wave_sum(T v) { return wave_reduce<T, add2<T>>(v); }

// torch's min / max carry a NaN: once NaN, NaN
__device__ __forceinline__ float nan_min(float a, float b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ float nan_max(float a, float b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ float wave_nan_min(float v) { return wave_reduce<float, nan_min>(v); }
__device__ __forceinline__ float wave_nan_max(float v) { return wave_reduce<float, nan_max>(v); }
// fminf / fmaxf drop a NaN: the result is NaN only if every lane's value is
__device__ __forceinline__ float wave_fmin(float v) { return wave_reduce<float, fminf>(v); }
__device__ __forceinline__ float wave_fmax(float v) { return wave_reduce<float, fmaxf>(v); }

// ---- four-wave tail of a 256-thread workgroup ----
// K per-thread partial sums (or counts): the butterfly of every wave, lane 0 parks wave w's sums in red[k][w].  No barrier inside: after the
// caller's, four_wave_total(red[k]) is the workgroup's sum and four_wave_min(red[k]) the minimum of four parked minima.
template <int K>
__device__ __forceinline__ void four_wave_park(float (&v)[K], float (*red)[4], int lane, int wave)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += __shfl_xor(v[k], o);
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[k][wave] = v[k];
}
template <typename T>
__device__ __forceinline__ T four_wave_total(const T *r) { return (r[0] + r[1]) + (r[2] + r[3]); }
__device__ __forceinline__ float four_wave_min(const float *r) { return fminf(fminf(r[0], r[1]), fminf(r[2], r[3])); }
__device__ __forceinline__ float four_wave_max(const float *r) { return fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3])); }

// ---- rank among the set lanes of a wave-wide flag ----
// bal = __ballot(flag): how many set lanes lie below `lane`.  With a running count in front it is the slot of an ordered compaction without
// atomics; the wave's count is __popcll(bal).
__device__ __forceinline__ int ballot_rank(unsigned long long bal, int lane) { return __popcll(bal & ((1ull << lane) - 1ull)); }

// ---- exclusive scan over the 256 threads of a workgroup: int, or int2 for two scans at once ----
__device__ __forceinline__ int lanes_up(int v, int o) { return __shfl_up(v, o); }
__device__ __forceinline__ int2 lanes_up(int2 v, int o) { return make_int2(__shfl_up(v.x, o), __shfl_up(v.y, o)); }

// returns the sum of v over the threads in front of this one; *total: the workgroup's sum, in every thread.  Two barriers, the second behind the
// last read of the function's LDS words: it may be called again at once.
template <typename T>
__device__ T block_exclusive_scan(T v, T *total)
{
    __shared__ T wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = lanes_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    T base = T();
    for (int w = 0; w < wave; ++w) base += wsum[w];
    *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    return base + x - v;
}

// ---- minimum of a 64-bit key over a workgroup of ANY whole number of waves up to sixteen (1024 threads) ----
// returns the smallest v of all threads, in every thread: an integer minimum, exact in any order, so a key (value bits) << 32 | index picks
// the smallest value and, among equal values, the lowest index.  Every thread of the workgroup must call it.  Two barriers, the second behind
// the last read of the function's LDS words: it may be called again at once.
__device__ __forceinline__ unsigned long long min_u64(unsigned long long a, unsigned long long b) { return b < a ? b : a; }
__device__ __forceinline__ unsigned long long lanes_xor(unsigned long long v, int o)
{
    const unsigned lo = __shfl_xor((unsigned)v, o), hi = __shfl_xor((unsigned)(v >> 32), o);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ unsigned long long block_min_u64(unsigned long long v)
{
    __shared__ unsigned long long wmin[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = (int)(blockDim.x >> 6);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min_u64(v, lanes_xor(v, o));
    if (lane == 0) wmin[wave] = v;
    __syncthreads();
    unsigned long long m = wmin[0];
    for (int w = 1; w < waves; ++w) m = min_u64(m, wmin[w]);
    __syncthreads();
    return m;
}

// ---- two-pass scan over a grid: kScanRows items per workgroup ----
// Pass one leaves every workgroup's sum in blk_sum[blockIdx.x]; in pass two a workgroup's offset is the sum of blk_sum[0 .. blockIdx.x), which
// every workgroup adds up itself (a strided sum, then the scan above: its two barriers) and every thread gets.  The second form: two arrays at once.
constexpr int kScanRows = 256;
inline size_t ag_scan_blocks(size_t rows) { return rows / kScanRows + 2; }      // words of a blk_sum buffer for `rows` items (host)

__device__ __forceinline__ int block_offset(const int32_t *blk_sum)
{
    int part = 0, base;
    for (int i = threadIdx.x; i < (int)blockIdx.x; i += kScanRows) part += blk_sum[i];
    block_exclusive_scan(part, &base);
    return base;
}
__device__ __forceinline__ int2 block_offset(const int32_t *blk_x, const int32_t *blk_y)
{
    int2 part = make_int2(0, 0), base;
    for (int i = threadIdx.x; i < (int)blockIdx.x; i += kScanRows) { part.x += blk_x[i]; part.y += blk_y[i]; }
    block_exclusive_scan(part, &base);
    return base;
}

}  // namespace
