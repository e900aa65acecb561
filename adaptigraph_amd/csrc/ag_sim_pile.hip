// ag_sim_pile.hip — a batched disc-pile-on-table simulator: one board push of E granular episodes in one launch.  Like ag_sim.hip it stands in
// for the data side of the reference (src/sim/sim_env/flex_env.py:258-402 steps a closed CUDA solver); the model is this project's own, stated
// operation for operation in adaptigraph_amd/sim/pile.py (pile_push_host, the float32 numpy statement) and repeated here so that both give the same bits.
//
// One 256-thread workgroup owns an episode for the whole push, four grains per thread (grain i = t + 256 k, n <= 1024).  A grain's position at
// the start of the substep and its velocity stay in registers; LDS holds the predicted positions of all grains twice
// (Jacobi: an iteration reads one copy and writes the other; 2 x 2 planes of 1024 floats = 16 KB) and the neighbour grid: 64 x 64 cells of side
// 2 rho 17/16 centred on the workspace's origin (4096 words = 16 KB) and the grains' indices sorted by cell (1024 words = 4 KB).  A grain's cell
// is trunc(min(max((p - origin) inv_cell, 0), 63)) per axis: a monotone map, under which two grains nearer than 2 rho lie in the same or in
// neighbouring cells (DESIGN.md §8.12 has the argument), also where the clamp folds everything outside the grid into its border cells.
// The grid is rebuilt before EVERY contact iteration, since an iteration moves grains:
//   clear    s_cell[c] = 0                                                          | barrier 1
//   count    atomicAdd(&s_cell[cell of grain], 1)            integer LDS atomics    | barrier 2
//   scan     thread t owns cells 16 t .. 16 t + 15: s_cell[c] = grains in the cells before c (block_exclusive_scan: two barriers) | barrier 5
//   place    slot = atomicAdd(&s_cell[cell], 1); s_slot[slot] = grain: s_cell[c] is now the END of cell c and the start of cell c + 1 | barrier 6
//   walk     the three rows of cells around a grain are three contiguous slot ranges; every j in them with 0 < d < 2 rho adds its two rounded
//            integers and one count; the grain's new position goes to the other copy   | barrier 7
// The order of the slots within a cell is the order of arrival at the atomic, which differs from call to call; nothing depends on it: the sums
// are integers.  No global atomics, no float atomics.  Whether an episode pushes or records, its n and its iteration count are uniform over its
// workgroup, so every barrier is reached by all 256 threads.  Every product is rounded on its own (-ffp-contract=off), division and square root
// are the correctly rounded ones.
#include "ag_sim_dev.h"
#include "ag_block_dev.h"

namespace {

constexpr int kPileThreads = 256;
constexpr int kPilePer = AG_SIM_PILE_MAX_PARTICLES / kPileThreads;      // grains per thread
constexpr int kPileGrid = 64, kPileCells = kPileGrid * kPileGrid, kPileCellsPer = kPileCells / kPileThreads;

struct PilePushArgs {
    const int32_t *n, *n_push;
    const float *rho, *inv, *push, *lat;
    float *x, *v, *obj, *eef;
    int32_t *n_frames;
    int n_max, F_max, n_push_max, substeps, iters, record_every, settle;
    float h, g, mu, W, T, slack, tool_y, lift, rho_max;
};

// the cell coordinate of p along one axis: 0 .. 63 for every p, NaN included (fmaxf drops it)
__device__ __forceinline__ int pile_cell(float p, float org, float inv_cell)
{
    return (int)fminf(fmaxf((p - org) * inv_cell, 0.f), (float)(kPileGrid - 1));
}

__device__ __forceinline__ int pile_cell2(float px, float pz, float org, float inv_cell)
{
    return pile_cell(pz, org, inv_cell) * kPileGrid + pile_cell(px, org, inv_cell);
}

__global__ __launch_bounds__(kPileThreads) void pile_push_kernel(const PilePushArgs a)
{
    __shared__ float s_px[2][AG_SIM_PILE_MAX_PARTICLES], s_pz[2][AG_SIM_PILE_MAX_PARTICLES];
    __shared__ __attribute__((aligned(16))) int s_cell[kPileCells];
    __shared__ int s_slot[AG_SIM_PILE_MAX_PARTICLES];
    const int e = blockIdx.x, t = threadIdx.x;
    const int n = a.n[e], n_push = a.n_push[e];
    const float rho = a.rho[e];
    if (n < 1 || n > a.n_max || n_push < 1 || n_push > a.n_push_max || !(rho > 0.f) || rho > a.rho_max) return sim_no_frame(a.n_frames, e, t);
    const float inv = a.inv[e];
    const float sx = a.push[4 * e], sz = a.push[4 * e + 1], ex = a.push[4 * e + 2], ez = a.push[4 * e + 3];
    const float ux = a.lat[2 * e], uz = a.lat[2 * e + 1];
    const float h = a.h, W = a.W, mW = -a.W;
    const float mgh = (a.mu * a.g) * h, two_rho = rho * 2.f, reach = rho + a.T, out = reach + a.slack;
    const float cell = two_rho * 1.0625f, inv_cell = 1.f / cell, org = -32.f * cell;
    const int S = a.substeps, total = n_push + a.settle;
    float *frames = a.obj + (size_t)e * a.F_max * a.n_max * 3;
    float *tool = a.eef + (size_t)e * a.F_max * 15;
    const float off = (t == 0 ? 1.f : t == 1 ? -1.f : t == 2 ? 0.f : t == 3 ? 0.5f : -0.5f) * W;      // key point t of threads 0 .. 4

    bool live[kPilePer];
    float x[kPilePer], y[kPilePer], z[kPilePer], vx[kPilePer], vz[kPilePer], px[kPilePer], pz[kPilePer];
#pragma unroll
    for (int k = 0; k < kPilePer; ++k) {
        const int i = t + kPileThreads * k;
        live[k] = i < n;
        const size_t row = ((size_t)e * a.n_max + (live[k] ? i : 0)) * 3;
        x[k] = live[k] ? a.x[row] : 0.f; y[k] = live[k] ? a.x[row + 1] : 0.f; z[k] = live[k] ? a.x[row + 2] : 0.f;
        vx[k] = live[k] ? a.v[row] : 0.f; vz[k] = live[k] ? a.v[row + 2] : 0.f;
        px[k] = x[k]; pz[k] = z[k];
    }
    float cx = sx, cz = sz;
    for (int st = 0; st < total; ++st) {
        const bool pushing = st < n_push;
        for (int s = 0; s < S; ++s) {
            // a. predict
#pragma unroll
            for (int k = 0; k < kPilePer; ++k) {
                px[k] = x[k] + h * vx[k]; pz[k] = z[k] + h * vz[k];
                if (live[k]) { s_px[0][t + kPileThreads * k] = px[k]; s_pz[0][t + kPileThreads * k] = pz[k]; }
            }
            // b. contacts: iteration `it` reads copy it & 1 and writes the other.  The copies and s_cell were last read before the barrier that
            // ends the iteration before (barrier 7), so the predict above and the clear below overwrite nothing that is still in use.
            for (int it = 0; it < a.iters; ++it) {
                const float *rx = s_px[it & 1], *rz = s_pz[it & 1];
                float *wx = s_px[(it & 1) ^ 1], *wz = s_pz[(it & 1) ^ 1];
#pragma unroll
                for (int c = 0; c < kPileCellsPer; ++c) s_cell[t + kPileThreads * c] = 0;
                __syncthreads();
                for (int i = t; i < n; i += kPileThreads) atomicAdd(&s_cell[pile_cell2(rx[i], rz[i], org, inv_cell)], 1);
                __syncthreads();
                int mine[kPileCellsPer], sum = 0, all;
#pragma unroll
                for (int c = 0; c < kPileCellsPer; ++c) { mine[c] = s_cell[t * kPileCellsPer + c]; sum += mine[c]; }
                int run = block_exclusive_scan(sum, &all);
#pragma unroll
                for (int c = 0; c < kPileCellsPer; ++c) { s_cell[t * kPileCellsPer + c] = run; run += mine[c]; }
                __syncthreads();
                for (int i = t; i < n; i += kPileThreads) s_slot[atomicAdd(&s_cell[pile_cell2(rx[i], rz[i], org, inv_cell)], 1)] = i;      // slot < all == n
                __syncthreads();
                for (int i = t; i < n; i += kPileThreads) {
                    const float xi = rx[i], zi = rz[i];
                    const int gx = pile_cell(xi, org, inv_cell), gz = pile_cell(zi, org, inv_cell);
                    const int x0 = max(gx - 1, 0), x1 = min(gx + 1, kPileGrid - 1), z1 = min(gz + 1, kPileGrid - 1);
                    int sum_x = 0, sum_z = 0, cnt = 0;
                    for (int r = max(gz - 1, 0); r <= z1; ++r) {
                        const int c0 = r * kPileGrid + x0;
                        const int hi = s_cell[r * kPileGrid + x1];
#pragma unroll 1      // a handful of slots per row; unrolled, the divisions and roots of eight of them cost 224 VGPRs instead of 109
                        for (int sl = c0 ? s_cell[c0 - 1] : 0; sl < hi; ++sl) {      // cells x0 .. x1 of row r: one contiguous range of slots
                            const int j = s_slot[sl];
                            const float dx = xi - rx[j], dz = zi - rz[j];
                            const float d = sqrtf(dx * dx + dz * dz);
                            if (j != i && d > 0.f && d < two_rho) {
                                const float c = (two_rho - d) / (d * 2.f);
                                sum_x += (int)rintf((c * dx) * 4194304.f);
                                sum_z += (int)rintf((c * dz) * 4194304.f);
                                ++cnt;
                            }
                        }
                    }
                    wx[i] = cnt ? xi + ((float)sum_x * (1.f / 4194304.f)) / (float)cnt : xi;
                    wz[i] = cnt ? zi + ((float)sum_z * (1.f / 4194304.f)) / (float)cnt : zi;
                }
                __syncthreads();
            }
#pragma unroll
            for (int k = 0; k < kPilePer; ++k)
                if (live[k]) { px[k] = s_px[a.iters & 1][t + kPileThreads * k]; pz[k] = s_pz[a.iters & 1][t + kPileThreads * k]; }
            // c. board
            if (pushing) {
                sim_tool_centre(cx, cz, sx, sz, ex, ez, sim_substep_t(st, S, s, inv));
#pragma unroll
                for (int k = 0; k < kPilePer; ++k) {
                    const float ax = px[k] - cx, az = pz[k] - cz;
                    float al = ax * ux + az * uz;
                    al = al < mW ? mW : al;      // (a NaN stays, as in numpy's maximum and minimum)
                    al = al > W ? W : al;
                    const float qx = cx + al * ux, qz = cz + al * uz;
                    const float fx = px[k] - qx, fz = pz[k] - qz;
                    const float d = sqrtf(fx * fx + fz * fz);
                    if (d > 0.f && d < reach) {
                        const float kk = out / d;
                        px[k] = qx + fx * kk; pz[k] = qz + fz * kk;
                    }
                }
            }
            // d. velocity and friction
#pragma unroll
            for (int k = 0; k < kPilePer; ++k) {
                const float wx_ = (px[k] - x[k]) / h, wz_ = (pz[k] - z[k]) / h;
                const float f = sim_coulomb(wx_, wz_, mgh);
                vx[k] = wx_ * f; vz[k] = wz_ * f;
                x[k] = px[k]; z[k] = pz[k];
            }
        }
        if (pushing && st % a.record_every == 0) {
            const int f = sim_recorded_frame(st, a.record_every);
#pragma unroll
            for (int k = 0; k < kPilePer; ++k)
                if (live[k]) sim_store3(frames + ((size_t)f * a.n_max + t + kPileThreads * k) * 3, x[k], y[k], z[k]);
            if (t < 5) { tool[(f * 5 + t) * 3] = cx + off * ux; tool[(f * 5 + t) * 3 + 1] = a.tool_y; tool[(f * 5 + t) * 3 + 2] = cz + off * uz; }
        }
    }
    const int f = sim_final_frame(n_push, a.record_every);
#pragma unroll
    for (int k = 0; k < kPilePer; ++k)
        if (live[k]) {
            const int i = t + kPileThreads * k;
            sim_store3(frames + ((size_t)f * a.n_max + i) * 3, x[k], y[k], z[k]);
            const size_t row = ((size_t)e * a.n_max + i) * 3;
            a.x[row] = x[k]; a.x[row + 2] = z[k];
            a.v[row] = vx[k]; a.v[row + 2] = vz[k];
        }
    if (t < 5) { tool[(f * 5 + t) * 3] = ex + off * ux; tool[(f * 5 + t) * 3 + 1] = a.tool_y + a.lift; tool[(f * 5 + t) * 3 + 2] = ez + off * uz; }
    if (t == 0) a.n_frames[e] = f + 1;
}

}  // namespace

extern "C" {

int ag_sim_pile_push(const int32_t *n, const float *rho, const float *inv, const int32_t *n_push, const float *push, const float *lat, float *x,
                     float *v, float *obj, float *eef, int32_t *n_frames, int E, int n_max, int F_max, int n_push_max, int substeps, int iters,
                     int record_every, int settle, float h, float g, float mu, float W, float T, float slack, float tool_y, float lift,
                     float rho_max, ag_stream_t stream)
{
    if (!n || !rho || !inv || !n_push || !push || !lat || !x || !v || !obj || !eef || !n_frames)
        return ag_fail(AG_ERR_ARG, "ag_sim_pile_push: null argument");
    if (int err = sim_check_schedule("ag_sim_pile_push", E, n_max, 1, AG_SIM_PILE_MAX_PARTICLES, "AG_SIM_PILE_MAX_PARTICLES", F_max, n_push_max, 1,
                                     substeps, true, iters, record_every, settle, h, "push"))
        return err;
    if (!(rho_max > 0.f) || rho_max > 0.25f)      // 1023 contact terms of at most rho 2^22 each must fit int32
        return ag_fail(AG_ERR_ARG, "ag_sim_pile_push: rho_max = %g outside (0, 0.25]", (double)rho_max);
    PilePushArgs a{n, n_push, rho, inv, push, lat, x, v, obj, eef, n_frames, n_max, F_max, n_push_max, substeps, iters, record_every, settle,
                   h, g, mu, W, T, slack, tool_y, lift, rho_max};
    hipLaunchKernelGGL(pile_push_kernel, dim3(E), dim3(kPileThreads), 0, static_cast<hipStream_t>(stream), a);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

}  // extern "C"
