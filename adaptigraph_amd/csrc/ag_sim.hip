// ag_sim.hip — a batched rope-on-table particle simulator: one push of E episodes in one launch.  It stands in for the data side of the
// reference (src/sim/sim_env/flex_env.py:258-402 steps a closed CUDA solver); the model is this project's own, stated operation for operation in
// adaptigraph_amd/sim/rope.py (rope_push_host, the float32 numpy restatement) and repeated here so that both give the same bits.
//
// One 256-thread workgroup owns an episode for the whole push, one particle per thread (n <= 256).  Positions and the cluster fits live in LDS (seven
// planes of 256 floats = 7 KB), the particle's own position, start-of-substep position and velocity in registers.  A substep:
//   a  predict      v.y -= g h; p = x + h v                                        write own p           | barrier 1
//   b  stretch      pairs (i, i + 1), even i                                       thread i writes i, i+1| barrier 2
//                   pairs (i, i + 1), odd i                                        thread i writes i, i+1| barrier 3
//   c  fits         cluster j = particles j .. j + w - 1: centroid, direction      thread j reads p, writes its fit | barrier 4 (only with clusters)
//      goals        particle i: mean goal over its clusters, ascending j           thread i reads fits, own p to registers
//   d-f pusher, ground, velocity and friction                                      registers only
// The next substep's write of p[i] comes after barrier 3 (no clusters) or 4 (clusters), behind every other thread's last read of it; the fits are
// rewritten behind barriers 1-3 of the next substep.  Whether an episode has clusters, pushes or records is uniform over its workgroup, so every
// barrier is reached by all 256 threads.  No atomics; every float sum runs in the stated order (no butterfly reductions), every product is rounded
// on its own (-ffp-contract=off), division and square root are the correctly rounded ones.
#include "ag_sim_dev.h"

namespace {

constexpr int kRopeThreads = AG_SIM_ROPE_MAX_PARTICLES;

struct RopePushArgs {
    const int32_t *n, *w, *n_push;
    const float *l0, *kappa, *inv, *push;
    float *x, *v, *obj, *eef;
    int32_t *n_frames;
    int n_max, F_max, n_push_max, substeps, record_every, settle;
    float h, g, r, R, mu, lift;
};

__device__ __forceinline__ void stretch_pair(float *px, float *py, float *pz, int i, float l0)
{
    const float xi = px[i], yi = py[i], zi = pz[i], xj = px[i + 1], yj = py[i + 1], zj = pz[i + 1];
    const float dx = xj - xi, dy = yj - yi, dz = zj - zi;
    const float len = sqrtf((dx * dx + dy * dy) + dz * dz);
    if (len > 0.f) {
        const float c = (len - l0) / (len * 2.f);
        px[i] = xi + c * dx; py[i] = yi + c * dy; pz[i] = zi + c * dz;
        px[i + 1] = xj - c * dx; py[i + 1] = yj - c * dy; pz[i + 1] = zj - c * dz;
    }
}

__global__ __launch_bounds__(kRopeThreads) void rope_push_kernel(const RopePushArgs a)
{
    __shared__ float s_px[kRopeThreads], s_py[kRopeThreads], s_pz[kRopeThreads];
    __shared__ float s_cx[kRopeThreads], s_cz[kRopeThreads], s_ux[kRopeThreads], s_uz[kRopeThreads];
    const int e = blockIdx.x, i = threadIdx.x;
    const int n = a.n[e], n_push = a.n_push[e];
    if (n < 2 || n > a.n_max || n_push < 1 || n_push > a.n_push_max) return sim_no_frame(a.n_frames, e, i);
    const bool live = i < n;
    const size_t row = ((size_t)e * a.n_max + (live ? i : 0)) * 3;
    float x = live ? a.x[row] : 0.f, y = live ? a.x[row + 1] : 0.f, z = live ? a.x[row + 2] : 0.f;
    float vx = live ? a.v[row] : 0.f, vy = live ? a.v[row + 1] : 0.f, vz = live ? a.v[row + 2] : 0.f;
    const float l0 = a.l0[e], kappa = a.kappa[e], inv = a.inv[e];
    const float sx = a.push[4 * e], sz = a.push[4 * e + 1], ex = a.push[4 * e + 2], ez = a.push[4 * e + 3];
    const int w = a.w[e];
    const bool clusters = w >= 3 && w <= n;
    const int n_cl = n - w + 1;                                            // clusters 0 .. n - w
    const float h = a.h, r = a.r;
    const float gh = a.g * h, reach = a.R + r, mgh = (a.mu * a.g) * h, fw = (float)w;
    const int S = a.substeps, total = n_push + a.settle;
    float *frames = a.obj + (size_t)e * a.F_max * a.n_max * 3;
    float *tool = a.eef + (size_t)e * a.F_max * 3;
    float px = x, py = y, pz = z, cx = sx, cz = sz;
    for (int st = 0; st < total; ++st) {
        const bool pushing = st < n_push;
        for (int s = 0; s < S; ++s) {
            // a. predict
            vy = vy - gh;
            px = x + h * vx; py = y + h * vy; pz = z + h * vz;
            if (live) { s_px[i] = px; s_py[i] = py; s_pz[i] = pz; }
            __syncthreads();
            // b. stretch: even pairs, then odd pairs
            if (!(i & 1) && i + 1 < n) stretch_pair(s_px, s_py, s_pz, i, l0);
            __syncthreads();
            if ((i & 1) && i + 1 < n) stretch_pair(s_px, s_py, s_pz, i, l0);
            __syncthreads();
            if (live) { px = s_px[i]; py = s_py[i]; pz = s_pz[i]; }
            // c. straight-segment shape matching (Jacobi: every fit reads the p of barrier 3)
            if (clusters) {
                if (i < n_cl) {
                    float mx = s_px[i], mz = s_pz[i];
                    for (int k = 1; k < w; ++k) { mx = mx + s_px[i + k]; mz = mz + s_pz[i + k]; }
                    mx = mx / fw; mz = mz / fw;
                    float fa = 0.f, fb = 0.f;
                    for (int k = 0; k < w; ++k) {
                        const float q = ((float)(2 * k - (w - 1)) * 0.5f) * l0;
                        const float ta = q * (s_px[i + k] - mx), tb = q * (s_pz[i + k] - mz);
                        fa = k ? fa + ta : ta; fb = k ? fb + tb : tb;
                    }
                    const float nn = sqrtf(fa * fa + fb * fb);
                    const bool zero = nn == 0.f;                           // (a NaN keeps the division and spreads, as on the host)
                    s_cx[i] = mx; s_cz[i] = mz;
                    s_ux[i] = zero ? 1.f : fa / nn; s_uz[i] = zero ? 0.f : fb / nn;
                }
                __syncthreads();
                if (live) {
                    const int j0 = max(0, i - w + 1), j1 = min(i, n_cl - 1);
                    float gx = 0.f, gz = 0.f;
                    for (int j = j0; j <= j1; ++j) {
                        const float q = ((float)(2 * (i - j) - (w - 1)) * 0.5f) * l0;
                        const float tx = s_cx[j] + q * s_ux[j], tz = s_cz[j] + q * s_uz[j];
                        gx = j > j0 ? gx + tx : tx; gz = j > j0 ? gz + tz : tz;      // the first term starts the sum, as in the fits
                    }
                    const float cnt = (float)(j1 - j0 + 1);
                    px = px + kappa * (gx / cnt - px); pz = pz + kappa * (gz / cnt - pz);
                }
            }
            // d. pusher
            if (pushing) {
                sim_tool_centre(cx, cz, sx, sz, ex, ez, sim_substep_t(st, S, s, inv));
                const float dx = px - cx, dz = pz - cz;
                const float d = sqrtf(dx * dx + dz * dz);
                if (d > 0.f && d < reach) {
                    const float k = reach / d;
                    px = cx + dx * k; pz = cz + dz * k;
                }
            }
            // e. ground
            const bool on = py <= r;
            py = fmaxf(py, r);
            // f. velocity and friction
            vx = (px - x) / h; vy = (py - y) / h; vz = (pz - z) / h;
            if (on) {
                const float f = sim_coulomb(vx, vz, mgh);
                vx = vx * f; vz = vz * f;
            }
            x = px; y = py; z = pz;
        }
        if (pushing && st % a.record_every == 0) {
            const int f = sim_recorded_frame(st, a.record_every);
            if (live) sim_store3(frames + ((size_t)f * a.n_max + i) * 3, x, y, z);
            if (i == 0) sim_store3(tool + 3 * f, cx, r, cz);
        }
    }
    const int f = sim_final_frame(n_push, a.record_every);
    if (live) {
        sim_store3(frames + ((size_t)f * a.n_max + i) * 3, x, y, z);
        sim_store3(a.x + row, x, y, z);
        sim_store3(a.v + row, vx, vy, vz);
    }
    if (i == 0) {
        sim_store3(tool + 3 * f, ex, r + a.lift, ez);
        a.n_frames[e] = f + 1;
    }
}

}  // namespace

extern "C" {

int ag_sim_rope_push(const int32_t *n, const float *l0, const int32_t *w, const float *kappa, const float *inv, const int32_t *n_push,
                     const float *push, float *x, float *v, float *obj, float *eef, int32_t *n_frames, int E, int n_max, int F_max,
                     int n_push_max, int substeps, int record_every, int settle, float h, float g, float r, float R, float mu, float lift,
                     ag_stream_t stream)
{
    if (!n || !l0 || !w || !kappa || !inv || !n_push || !push || !x || !v || !obj || !eef || !n_frames)
        return ag_fail(AG_ERR_ARG, "ag_sim_rope_push: null argument");
    if (int err = sim_check_schedule("ag_sim_rope_push", E, n_max, 2, AG_SIM_ROPE_MAX_PARTICLES, "AG_SIM_ROPE_MAX_PARTICLES", F_max, n_push_max, 1,
                                     substeps, false, 0, record_every, settle, h, "push"))
        return err;
    RopePushArgs a{n, w, n_push, l0, kappa, inv, push, x, v, obj, eef, n_frames, n_max, F_max, n_push_max, substeps, record_every, settle,
                   h, g, r, R, mu, lift};
    hipLaunchKernelGGL(rope_push_kernel, dim3(E), dim3(kRopeThreads), 0, static_cast<hipStream_t>(stream), a);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

}  // extern "C"
