// ag_fps.hip — farthest-point key-point sampling (src/dynamics/dataset/graph.py:8-36, src/dynamics/utils.py:10-24, src/planning/perception.py:266-279).
//
// Per cloud: pick `start`; keep for every point the distance to its nearest pick; the next pick is the arg-max of the kept distances, LOWEST INDEX on
// ties; stop after K picks, after `count` picks, or (radius given) once the largest kept distance is <= radius.  The picks are strictly sequential and
// every pick touches every point, so ONE workgroup owns a cloud for the whole call (B clouds = B workgroups; a single cloud uses one CU — splitting a
// cloud over workgroups would put a grid-wide exchange of ~10 us into a pick that costs well under 1 us).
//
// Resident form (N <= AG_FPS_RESIDENT_POINTS): thread t of T holds points t, t + T, t + 2T ... (at most kPPT of them) with their coordinates and kept
// distances in registers from the first pick to the last.  Per pick: update + local arg-max in registers (ascending index, strict >: the lowest index of
// a thread's maxima), a wave reduction on the packed key (distance bits << 32 | ~index: ONE unsigned max gives the largest distance and, among equals,
// the lowest index; kept distances are >= +0 and finite, so their bit patterns order like the values), then one LDS exchange: the winning lane of every
// wave writes its key and ITS coordinates to the wave's slot, one barrier, every thread reads the 16 slots, takes the max and reads the winner's
// coordinates from its slot.  The slots are double-buffered by pick parity, so a pick costs ONE workgroup barrier (the slot written for pick k + 2 was
// last read before barrier k + 1).  The stop tests depend on the reduced key only: workgroup-uniform.
// Streaming form (any N): the same loop with the points read from global memory and the kept distances in the caller's workspace (each thread reads and
// writes only its own entries: no further synchronisation).
//
// The arithmetic is the host code's (adaptigraph_amd/sampling.py), operation for operation: d = p - pick per axis, (d0 d0 + d1 d1) + d2 d2 with every
// product and sum rounded to fp32 (the library is built with -ffp-contract=off), AG_FPS_NORM then takes the correctly rounded square root of EVERY
// distance before the min (the root maps neighbouring floats to one value: ties the squared form does not have).
#include "ag_common.h"
#include "../../include/adaptigraph_hip.h"

namespace {

constexpr int kPPT = 8;                 // resident points per thread: kPPT * 1024 = AG_FPS_RESIDENT_POINTS
constexpr int kMaxWaves = 16;           // 1024 threads
static_assert(kPPT * 64 * kMaxWaves == AG_FPS_RESIDENT_POINTS, "header constant");

typedef unsigned long long u64;

template <int CTRL> __device__ __forceinline__ u64 key_max_dpp(u64 k)
{
    const int lo = (int)(unsigned)k, hi = (int)(unsigned)(k >> 32);
    const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
    const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
    const u64 o = ((u64)ohi << 32) | olo;
    return o > k ? o : k;
}

// max of the key over the 64 lanes, wave-uniform: quads and 16-lane rows by DPP, the four rows through scalar registers
__device__ __forceinline__ u64 key_max_wave(u64 k)
{
    k = key_max_dpp<0xB1>(k);       // quad_perm [1, 0, 3, 2]
    k = key_max_dpp<0x4E>(k);       // quad_perm [2, 3, 0, 1]
    k = key_max_dpp<0x124>(k);      // row_ror 4
    k = key_max_dpp<0x128>(k);      // row_ror 8: every lane holds its row's max
    const int lo = (int)(unsigned)k, hi = (int)(unsigned)(k >> 32);
    u64 m = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const u64 v = ((u64)(unsigned)__builtin_amdgcn_readlane(hi, 16 * r) << 32) | (unsigned)__builtin_amdgcn_readlane(lo, 16 * r);
        m = v > m ? v : m;
    }
    return m;
}

template <int METRIC> __device__ __forceinline__ float fps_dist(float x, float y, float z, float cx, float cy, float cz)
{
    const float d0 = x - cx, d1 = y - cy, d2 = z - cz;
    const float s = (d0 * d0 + d1 * d1) + d2 * d2;
    // sqrtf, not __fsqrt_rn: hipcc expands sqrtf to v_sqrt_f32 plus the FMA-residual test of its two neighbours (correctly rounded); __fsqrt_rn is the bare
    // 1-ulp v_sqrt_f32 here
    if constexpr (METRIC == AG_FPS_NORM) return sqrtf(s);
    else return s;
}

template <bool RESIDENT, int METRIC>
__global__ __launch_bounds__(1024) void fps_kernel(const float *__restrict__ pts, const int32_t *__restrict__ count, const int32_t *__restrict__ start,
                                                   int N, int K, const double *__restrict__ radius, int32_t *__restrict__ idx,
                                                   int32_t *__restrict__ n_out, float *__restrict__ near_ws)
{
    __shared__ uint2 s_key[2][kMaxWaves];
    __shared__ float4 s_xyz[2][kMaxWaves];
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const float *p = pts + (size_t)b * N * 3;
    int32_t *out = idx + (size_t)b * K;
    const int cnt = min(count ? count[b] : N, N);
    int cur = start[b];
    if (tid < 2 * kMaxWaves) s_key[tid >> 4][tid & 15] = make_uint2(0u, 0u);      // slots of waves that do not exist never win
    int n = 0;
    if (cnt >= 1 && cur >= 0 && cur < cnt) {      // (anything else: no pick, n_out = 0)
        const int klim = min(K, cnt);
        const bool has_r = METRIC == AG_FPS_NORM && radius != nullptr;
        const double r = has_r ? radius[b] : 0.0;
        float px[kPPT], py[kPPT], pz[kPPT], nr[kPPT];
        const int used = RESIDENT ? (cnt + T - 1) / T : 0;      // points per thread in use (uniform)
        if constexpr (RESIDENT) {
#pragma unroll
            for (int j = 0; j < kPPT; ++j) {
                const int i = j * T + tid;
                const bool ok = i < cnt;
                px[j] = ok ? p[3 * (size_t)i] : 0.f; py[j] = ok ? p[3 * (size_t)i + 1] : 0.f; pz[j] = ok ? p[3 * (size_t)i + 2] : 0.f;
                nr[j] = ok ? INFINITY : -INFINITY;      // min(-inf, d) stays -inf and never exceeds the running maximum
            }
        }
        float *ws = RESIDENT ? nullptr : near_ws + (size_t)b * N;
        float cx = p[3 * (size_t)cur], cy = p[3 * (size_t)cur + 1], cz = p[3 * (size_t)cur + 2];
        __syncthreads();
        for (int k = 0;; ++k) {
            if (tid == 0) out[k] = cur;
            float bd = -INFINITY, bx = 0.f, by = 0.f, bz = 0.f;
            int bi = 0;
            if constexpr (RESIDENT) {
#pragma unroll
                for (int j = 0; j < kPPT; ++j)
                    if (j < used) {
                        nr[j] = fminf(nr[j], fps_dist<METRIC>(px[j], py[j], pz[j], cx, cy, cz));
                        if (nr[j] > bd) { bd = nr[j]; bi = j * T + tid; bx = px[j]; by = py[j]; bz = pz[j]; }
                    }
            } else {
                for (int i = tid; i < cnt; i += T) {
                    const float x = p[3 * (size_t)i], y = p[3 * (size_t)i + 1], z = p[3 * (size_t)i + 2];
                    const float v = fminf(k ? ws[i] : INFINITY, fps_dist<METRIC>(x, y, z, cx, cy, cz));
                    ws[i] = v;
                    if (v > bd) { bd = v; bi = i; bx = x; by = y; bz = z; }
                }
            }
            const u64 key = tid < cnt ? ((u64)__float_as_uint(bd) << 32) | (unsigned)~bi : 0ull;      // a thread with a point has a key > 0
            const u64 wmax = key_max_wave(key);
            const int buf = k & 1;
            if (key == wmax && (key != 0ull || lane == 0)) {      // exactly one lane per wave (indices are unique)
                s_key[buf][wave] = make_uint2((unsigned)wmax, (unsigned)(wmax >> 32));
                s_xyz[buf][wave] = make_float4(bx, by, bz, 0.f);
            }
            __syncthreads();
            u64 g = 0;
            int gw = 0;
#pragma unroll
            for (int w = 0; w < kMaxWaves; ++w) {
                const uint2 e = s_key[buf][w];
                const u64 v = ((u64)e.y << 32) | e.x;
                if (v > g) { g = v; gw = w; }
            }
            n = k + 1;
            if (n >= klim) break;
            if (has_r && !((double)__uint_as_float((unsigned)(g >> 32)) > r)) break;      // the host's `while near.max() > radius`
            const float4 c = s_xyz[buf][gw];
            cur = (int)~(unsigned)g;
            cx = c.x; cy = c.y; cz = c.z;
        }
    }
    for (int i = n + tid; i < K; i += T) out[i] = -1;
    if (tid == 0) n_out[b] = n;
}

template <bool RESIDENT, int METRIC>
void launch(int T, const float *pts, const int32_t *count, const int32_t *start, int B, int N, int K, const double *radius, int32_t *idx,
            int32_t *n_out, float *ws, hipStream_t s)
{
    hipLaunchKernelGGL((fps_kernel<RESIDENT, METRIC>), dim3(B), dim3(T), 0, s, pts, count, start, N, K, radius, idx, n_out, ws);
}

}  // namespace

void ag_launch_fps(const float *pts, const int32_t *count, const int32_t *start, int B, int N, int K, int metric, const double *radius,
                   int32_t *idx, int32_t *n_out, float *near_ws, hipStream_t s)
{
    const bool norm = metric == AG_FPS_NORM;
    if (N <= AG_FPS_RESIDENT_POINTS) {
        // about four points per thread: the update is a dependent chain per point, the barrier grows with the number of waves
        int T = 64;
        while (T < 1024 && 4 * T < N) T *= 2;
        if (norm) launch<true, AG_FPS_NORM>(T, pts, count, start, B, N, K, radius, idx, n_out, nullptr, s);
        else launch<true, AG_FPS_SQUARED>(T, pts, count, start, B, N, K, nullptr, idx, n_out, nullptr, s);
    } else {
        if (norm) launch<false, AG_FPS_NORM>(1024, pts, count, start, B, N, K, radius, idx, n_out, near_ws, s);
        else launch<false, AG_FPS_SQUARED>(1024, pts, count, start, B, N, K, nullptr, idx, n_out, near_ws, s);
    }
}
