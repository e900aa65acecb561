// ag_batch.hip — training batches assembled on the device (src/dynamics/dataset/dataset.py:10-252): DynDataset.__getitem__ of B samples and
// their collation, from position stores that stay in HBM.
//
// Two kernels, both pure data movement of a few megabytes per batch (launch latency, not bandwidth, is their cost):
//   gather_clouds   one thread per float of the padded (B, Nmax, 3) cloud buffer: a linear, coalesced copy of one frame per sample.
//   assemble        one thread per (sample b, frame slot f, node j): it loads the node's position at that slot — a picked object point, a tool
//                   point, or zero padding — and writes every tensor that position belongs to; the threads of slot 0 also write the per-node
//                   tensors that do not depend on the slot (attrs, masks, p_instance, material_index).  Consecutive threads are consecutive
//                   nodes: stores are contiguous 12-byte pieces, loads follow the picks.
//
// The arithmetic is the host code's (adaptigraph_amd/dataset.py), which the tests compare bit for bit:
//   noise     fp32(double(v) + noise): numpy adds a float64 array into a float32 one in float64 and rounds once
//   actions   tool[f + 1] - tool[f] in the tool store's own type, rounded to fp32 afterwards
//   rotation  a @ rot: out_j = fmaf(a2, r2j, fmaf(a1, r1j, a0 * r0j)) — the first product rounded, then two fused steps (the library is built
//             with -ffp-contract=off, so nothing else is fused)
// Every index read from device memory (episode, frame, pick, pick count) is range-checked; a bad one yields zeros.
#include "ag_common.h"
#include "../../include/adaptigraph_hip.h"

namespace {

constexpr int kThreads = 128;

struct Episode {
    long long obj_off, tool_off, T, N;
    bool ok;
};

__device__ __forceinline__ Episode load_episode(const int64_t *__restrict__ episodes, int n_episodes, int e)
{
    Episode r = {0, 0, 0, 0, false};
    if (e >= 0 && e < n_episodes) {
        const int64_t *row = episodes + 4 * (size_t)e;
        r.obj_off = row[0]; r.tool_off = row[1]; r.T = row[2]; r.N = row[3];
        r.ok = r.obj_off >= 0 && r.tool_off >= 0 && r.T > 0 && r.N > 0;
    }
    return r;
}

__global__ __launch_bounds__(kThreads) void gather_clouds_kernel(const float *__restrict__ store, const int64_t *__restrict__ episodes, int n_episodes,
                                                                 const int32_t *__restrict__ epi, const int32_t *__restrict__ frame, int Nmax,
                                                                 float *__restrict__ pts, int32_t *__restrict__ count)
{
    const int b = blockIdx.y;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;      // float of row b
    const Episode ep = load_episode(episodes, n_episodes, epi[b]);
    const long long f = frame[b];
    const bool ok = ep.ok && f >= 0 && f < ep.T;
    const long long n = ok ? (ep.N < Nmax ? ep.N : (long long)Nmax) : 0;
    if (i == 0) count[b] = (int32_t)n;
    if (i < 3ll * Nmax) pts[(size_t)b * 3 * Nmax + i] = i < 3 * n ? store[(ep.obj_off + f * ep.N) * 3 + i] : 0.f;
}

struct AssembleArgs {
    ag_batch_dims d;
    const float *obj;
    const void *tool;
    const int64_t *episodes;
    const int32_t *epi, *frames, *picks;
    const double *noise;
    const float *rot;
    ag_batch_out o;
};

struct Vec3 {
    float x, y, z;
};

__device__ __forceinline__ Vec3 rotate(Vec3 a, const float *__restrict__ r)
{
    if (!r) return a;
    Vec3 o;
    o.x = fmaf(a.z, r[6], fmaf(a.y, r[3], a.x * r[0]));
    o.y = fmaf(a.z, r[7], fmaf(a.y, r[4], a.x * r[1]));
    o.z = fmaf(a.z, r[8], fmaf(a.y, r[5], a.x * r[2]));
    return o;
}

__device__ __forceinline__ void store3(float *__restrict__ p, Vec3 v)
{
    p[0] = v.x; p[1] = v.y; p[2] = v.z;
}

template <typename TOOL> __global__ __launch_bounds__(kThreads) void assemble_kernel(const AssembleArgs a)
{
    const int H = a.d.H, Fu = a.d.Fu, no = a.d.no, K = a.d.K, ns = a.d.no + a.d.n_eef;
    const int j = blockIdx.x * kThreads + threadIdx.x, f = blockIdx.y, b = blockIdx.z;
    if (j >= ns) return;
    const Episode ep = load_episode(a.episodes, a.d.n_episodes, a.epi[b]);
    const int32_t *fr = a.frames + (size_t)b * (H + Fu);
    const int32_t *pk = a.picks + (size_t)b * (K + 1);
    const int n_kp = max(0, min(pk[K], min(K, no)));
    const bool tool_row = j >= no;
    const long long frame = fr[f];
    const bool frame_ok = ep.ok && frame >= 0 && frame < ep.T;
    const float *rot = a.rot ? a.rot + 9 * (size_t)b : nullptr;

    // the node's position at this slot, and for a tool point the step to the next slot
    Vec3 v = {0.f, 0.f, 0.f}, step = {0.f, 0.f, 0.f};
    const bool wants_step = f >= H - 1 && f < H + Fu - 1;
    if (tool_row) {
        if (frame_ok) {
            const TOOL *p = static_cast<const TOOL *>(a.tool) + (ep.tool_off + frame * a.d.n_eef + (j - no)) * 3;
            const TOOL px = p[0], py = p[1], pz = p[2];
            v.x = (float)px; v.y = (float)py; v.z = (float)pz;
            if (wants_step) {
                const long long next = fr[f + 1];
                if (next >= 0 && next < ep.T) {
                    const TOOL *q = static_cast<const TOOL *>(a.tool) + (ep.tool_off + next * a.d.n_eef + (j - no)) * 3;
                    step.x = (float)(q[0] - px); step.y = (float)(q[1] - py); step.z = (float)(q[2] - pz);
                }
            }
        }
    } else if (j < n_kp && frame_ok) {
        const long long src = pk[j];
        if (src >= 0 && src < ep.N) {
            const float *p = a.obj + (ep.obj_off + frame * ep.N + src) * 3;
            v.x = p[0]; v.y = p[1]; v.z = p[2];
        }
    }

    if (f < H) {
        Vec3 s = v;
        if (a.noise) {
            const double *nz = a.noise + (((size_t)b * H + f) * ns + j) * 3;
            s.x = (float)((double)s.x + nz[0]); s.y = (float)((double)s.y + nz[1]); s.z = (float)((double)s.z + nz[2]);
        }
        store3(a.o.state + (((size_t)b * H + f) * ns + j) * 3, rotate(s, rot));
    } else {
        if (!tool_row) store3(a.o.state_future + (((size_t)b * Fu + (f - H)) * no + j) * 3, rotate(v, rot));
        if (f < H + Fu - 1) {
            const Vec3 zero = {0.f, 0.f, 0.f};
            store3(a.o.eef_future + (((size_t)b * (Fu - 1) + (f - H)) * ns + j) * 3, tool_row ? rotate(v, rot) : zero);
        }
    }
    if (wants_step) {
        float *dst = f == H - 1 ? a.o.action + ((size_t)b * ns + j) * 3 : a.o.action_future + (((size_t)b * (Fu - 1) + (f - H)) * ns + j) * 3;
        store3(dst, rotate(step, rot));
    }
    if (f == 0) {
        const bool kept = j < n_kp;
        const size_t node = (size_t)b * ns + j;
        a.o.attrs[2 * node] = kept ? 1.f : 0.f;
        a.o.attrs[2 * node + 1] = tool_row ? 1.f : 0.f;
        a.o.state_mask[node] = kept || tool_row;
        a.o.eef_mask[node] = tool_row;
        if (!tool_row) {
            const size_t obj = (size_t)b * no + j;
            a.o.p_instance[obj] = kept ? 1.f : 0.f;
            a.o.obj_mask[obj] = kept;
            for (int m = 0; m < a.d.n_mat; ++m) a.o.material_index[obj * a.d.n_mat + m] = kept && m == a.d.mat_col;
        }
    }
}

}  // namespace

void ag_launch_gather_clouds(const float *store, const int64_t *episodes, int n_episodes, const int32_t *epi, const int32_t *frame, int B, int Nmax,
                             float *pts, int32_t *count, hipStream_t s)
{
    const unsigned gx = (unsigned)((3ll * Nmax + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(gather_clouds_kernel, dim3(gx, B), dim3(kThreads), 0, s, store, episodes, n_episodes, epi, frame, Nmax, pts, count);
}

void ag_launch_assemble_batch(const ag_batch_dims &d, const float *obj, const void *tool, const int64_t *episodes, const int32_t *epi,
                              const int32_t *frames, const int32_t *picks, const double *noise, const float *rot, const ag_batch_out &o, hipStream_t s)
{
    const AssembleArgs a = {d, obj, tool, episodes, epi, frames, picks, noise, rot, o};
    const dim3 grid((d.no + d.n_eef + kThreads - 1) / kThreads, d.H + d.Fu, d.B);
    if (d.tool_f64) hipLaunchKernelGGL(assemble_kernel<double>, grid, dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL(assemble_kernel<float>, grid, dim3(kThreads), 0, s, a);
}
