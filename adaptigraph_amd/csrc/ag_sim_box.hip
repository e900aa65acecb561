// ag_sim_box.hip — a batched rigid-box-on-table simulator: one push of E box episodes in one launch.  It stands in for the data side of the
// reference's fourth material (src/sim/data_gen/data_gen_box.py over src/sim/sim_env/pymunk_env.py, a 2-D rigid-body engine that does not
// exist here); the model is this project's own (not pymunk, not fitted to it), stated operation for operation in adaptigraph_amd/sim/box.py
// (box_push_host, the float32 numpy statement) and repeated here so that both give the same bits.
//
// One 256-thread workgroup owns an episode for the whole call.  The body's state -- pose (X, Z, co, si), velocity (VX, VZ, Omega) -- is seven
// floats, and every thread carries all of it and repeats the scalar steps (predict, pusher, velocity, the 3 x 3 solve): the same operations on
// the same values give the same bits in every thread, so nothing is broadcast.  The particles exist for step d only, the friction of the
// support: up to four per thread (particle i = t + 256 k, n <= 1024), rest coordinate and mass in registers for the whole call.  Each forms its
// four terms k, k rx, k rz, k |rho|^2, rounds each times 2^22 to a 64-bit integer, and the workgroup adds them up: a thread's own four, the
// butterfly of its wave (wave_sum), the four wave sums through LDS.  Integer additions are exact in any order, which is the whole basis of the
// equality with the host.  |term| <= BOX_K_MAX BOX_RHO_MAX^2 = 2^13 2^6, so a scaled term stays under 2^41 and 1024 of them under 2^51: inside
// int64, and inside float64's 53 bits on the way back to float32.  The parked sums alternate between two LDS buffers, so a substep has ONE
// barrier: a thread that writes buffer p again has passed the barrier of the substep between, which every thread reaches only after its reads
// of buffer p.  n, the step counts, pushing and recording are uniform over a workgroup, and an episode outside its bounds returns as a whole
// before the first barrier.  No atomics, no float reductions.  Every product is rounded on its own (-ffp-contract=off), division and square
// root are the correctly rounded ones.
#include "ag_sim_dev.h"
#include "ag_block_dev.h"

namespace {

constexpr int kBoxThreads = 256;
constexpr int kBoxPer = AG_SIM_BOX_MAX_PARTICLES / kBoxThreads;      // particles per thread
constexpr float kBoxRhoMax = 8.f, kBoxKMax = 8192.f;                 // sim/box.py: BOX_RHO_MAX, BOX_K_MAX
constexpr float kQ22 = 4194304.f;

struct BoxPushArgs {
    const int32_t *n, *n_push;
    const float *q, *m, *body, *inv, *push;
    float *pose, *vel, *obj, *eef, *pose_frames;
    int32_t *n_frames;
    int n_max, F_max, n_push_max, substeps, iters, record_every, settle;
    float h, g, mu, r, R, eps, v_rest, cap, lift;
};

// (co, si) turned by the rotation of Cayley parameter t and renormalised; left as it is when t == 0
__device__ __forceinline__ void box_turn(float &co, float &si, const float t)
{
    if (t == 0.f) return;
    const float tt = t * t, den = 1.f + tt;
    const float cr = (1.f - tt) / den, sr = (t + t) / den;
    const float c2 = co * cr - si * sr, s2 = si * cr + co * sr;
    const float nn = sqrtf(c2 * c2 + s2 * s2);
    co = c2 / nn; si = s2 / nn;
}

__device__ __forceinline__ float box_sum_to_float(long long total) { return (float)(double)total * (1.f / kQ22); }

__global__ __launch_bounds__(kBoxThreads) void box_push_kernel(const BoxPushArgs a)
{
    __shared__ long long s_red[2][4][4];      // [buffer][sum][wave]
    const int e = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = a.n[e], n_push = a.n_push[e];
    const float *body = a.body + 6 * e;
    const float xlo = body[0], xhi = body[1], zlo = body[2], zhi = body[3], I = body[4], rho_max = body[5];
    if (n < 4 || n > a.n_max || n_push < 1 || n_push > a.n_push_max || !(I > 0.f) || !(rho_max > 0.f) || rho_max > kBoxRhoMax)
        return sim_no_frame(a.n_frames, e, t);
    const float inv = a.inv[e];
    const float xs = a.push[4 * e], zs = a.push[4 * e + 1], xe = a.push[4 * e + 2], ze = a.push[4 * e + 3];
    const float h = a.h, r = a.r, R = a.R, eps = a.eps, cap = a.cap, mug = a.mu * a.g;
    const int S = a.substeps, total = n_push + a.settle;
    float *frames = a.obj + (size_t)e * a.F_max * a.n_max * 3;
    float *tool = a.eef + (size_t)e * a.F_max * 3;
    float *poses = a.pose_frames + (size_t)e * a.F_max * 4;

    bool live[kBoxPer];
    float qx[kBoxPer], qz[kBoxPer], m[kBoxPer];
#pragma unroll
    for (int k = 0; k < kBoxPer; ++k) {
        const int i = t + kBoxThreads * k;
        live[k] = i < n;
        const size_t row = (size_t)e * a.n_max + (live[k] ? i : 0);
        qx[k] = live[k] ? a.q[2 * row] : 0.f; qz[k] = live[k] ? a.q[2 * row + 1] : 0.f; m[k] = live[k] ? a.m[row] : 0.f;
    }
    float X = a.pose[4 * e], Z = a.pose[4 * e + 1], co = a.pose[4 * e + 2], si = a.pose[4 * e + 3];
    float VX = a.vel[3 * e], VZ = a.vel[3 * e + 1], Om = a.vel[3 * e + 2];
    float cx = xs, cz = zs;
    int buf = 0;
    for (int st = 0; st < total; ++st) {
        const bool pushing = st < n_push;
        for (int s = 0; s < S; ++s) {
            float X0 = X, Z0 = Z, co0 = co, si0 = si;
            // a. predict
            X = X + h * VX; Z = Z + h * VZ;
            box_turn(co, si, (Om * h) * 0.5f);
            // b. pusher
            if (pushing) {
                sim_tool_centre(cx, cz, xs, zs, xe, ze, sim_substep_t(st, S, s, inv));
                for (int it = 0; it < a.iters; ++it) {
                    const float dx = cx - X, dz = cz - Z;
                    const float lx = co * dx + si * dz, lz = co * dz - si * dx;
                    const float kx = nan_min(nan_max(lx, xlo), xhi), kz = nan_min(nan_max(lz, zlo), zhi);
                    const float gx = lx - kx, gz = lz - kz;
                    const float dist = sqrtf(gx * gx + gz * gz);
                    float nbx, nbz, pcx, pcz, pen;
                    if (dist == 0.f) {      // inside: out through the nearest face, the first of x_lo, x_hi, z_lo, z_hi
                        const float d0 = lx - xlo, d1 = xhi - lx, d2 = lz - zlo, d3 = zhi - lz;
                        const float dmin = nan_min(nan_min(d0, d1), nan_min(d2, d3));
                        if (d0 == dmin) { nbx = 1.f; nbz = 0.f; pcx = xlo; pcz = lz; }
                        else if (d1 == dmin) { nbx = -1.f; nbz = 0.f; pcx = xhi; pcz = lz; }
                        else if (d2 == dmin) { nbx = 0.f; nbz = 1.f; pcx = lx; pcz = zlo; }
                        else { nbx = 0.f; nbz = -1.f; pcx = lx; pcz = zhi; }
                        pen = dmin + R;
                    } else if (dist < R) {
                        nbx = -(gx / dist); nbz = -(gz / dist); pcx = kx; pcz = kz; pen = R - dist;
                    } else {
                        continue;
                    }
                    const float cr = pcx * nbz - pcz * nbx;
                    const float w = 1.f + (cr * cr) / I;
                    const float nwx = co * nbx - si * nbz, nwz = si * nbx + co * nbz;
                    if (pen > cap) {      // beyond cap: the box and the substep's start alike, so no velocity comes of it
                        const float lam1 = (pen - cap) / w;
                        const float t1 = ((cr * lam1) / I) * 0.5f;
                        X = X + lam1 * nwx; Z = Z + lam1 * nwz; X0 = X0 + lam1 * nwx; Z0 = Z0 + lam1 * nwz;
                        box_turn(co, si, t1); box_turn(co0, si0, t1);
                    }
                    const float lam = nan_min(pen, cap) / w;
                    X = X + lam * nwx; Z = Z + lam * nwz;
                    box_turn(co, si, ((cr * lam) / I) * 0.5f);
                }
            }
            // c. velocity
            float wx = (X - X0) / h, wz = (Z - Z0) / h;
            const float crel = co * co0 + si * si0, srel = si * co0 - co * si0;
            const float trel = srel / (1.f + crel);
            float wo = (trel + trel) / h;
            // d. support friction: the four integer sums
            long long t0 = 0, tx = 0, tz = 0, t2 = 0;
#pragma unroll
            for (int k = 0; k < kBoxPer; ++k) {
                if (!live[k]) continue;
                const float rx = co * qx[k] - si * qz[k], rz = si * qx[k] + co * qz[k];
                const float ux = wx - wo * rz, uz = wz + wo * rx;
                const float kk = (m[k] * mug) / nan_max(sqrtf(ux * ux + uz * uz), eps);
                t0 += (long long)rintf(kk * kQ22);
                tx += (long long)rintf((kk * rx) * kQ22);
                tz += (long long)rintf((kk * rz) * kQ22);
                t2 += (long long)rintf((kk * (rx * rx + rz * rz)) * kQ22);
            }
            t0 = wave_sum(t0); tx = wave_sum(tx); tz = wave_sum(tz); t2 = wave_sum(t2);
            if (lane == 0) { s_red[buf][0][wave] = t0; s_red[buf][1][wave] = tx; s_red[buf][2][wave] = tz; s_red[buf][3][wave] = t2; }
            __syncthreads();
            const float S0 = box_sum_to_float(four_wave_total(s_red[buf][0])), Sx = box_sum_to_float(four_wave_total(s_red[buf][1]));
            const float Sz = box_sum_to_float(four_wave_total(s_red[buf][2])), S2 = box_sum_to_float(four_wave_total(s_red[buf][3]));
            buf ^= 1;
            const float ma = 1.f + h * S0, mb = -(h * Sz), mc = h * Sx, md = I + h * S2;
            const float r3 = I * wo;
            wo = (r3 - (mb * wx + mc * wz) / ma) / (md - (mb * mb + mc * mc) / ma);
            wx = (wx - mb * wo) / ma; wz = (wz - mc * wo) / ma;
            if (sqrtf(wx * wx + wz * wz) + nan_max(wo, -wo) * rho_max < a.v_rest) { wx = 0.f; wz = 0.f; wo = 0.f; }
            VX = wx; VZ = wz; Om = wo;
        }
        if (pushing && st % a.record_every == 0) {
            const int f = sim_recorded_frame(st, a.record_every);
#pragma unroll
            for (int k = 0; k < kBoxPer; ++k)
                if (live[k])
                    sim_store3(frames + ((size_t)f * a.n_max + t + kBoxThreads * k) * 3, X + (co * qx[k] - si * qz[k]), r, Z + (si * qx[k] + co * qz[k]));
            if (t == 0) {
                sim_store3(tool + f * 3, cx, r, cz);
                poses[f * 4] = X; poses[f * 4 + 1] = Z; poses[f * 4 + 2] = co; poses[f * 4 + 3] = si;
            }
        }
    }
    const int f = sim_final_frame(n_push, a.record_every);
#pragma unroll
    for (int k = 0; k < kBoxPer; ++k)
        if (live[k])
            sim_store3(frames + ((size_t)f * a.n_max + t + kBoxThreads * k) * 3, X + (co * qx[k] - si * qz[k]), r, Z + (si * qx[k] + co * qz[k]));
    if (t == 0) {
        sim_store3(tool + f * 3, xe, r + a.lift, ze);
        poses[f * 4] = X; poses[f * 4 + 1] = Z; poses[f * 4 + 2] = co; poses[f * 4 + 3] = si;
        a.pose[4 * e] = X; a.pose[4 * e + 1] = Z; a.pose[4 * e + 2] = co; a.pose[4 * e + 3] = si;
        a.vel[3 * e] = VX; a.vel[3 * e + 1] = VZ; a.vel[3 * e + 2] = Om;
        a.n_frames[e] = f + 1;
    }
}

}  // namespace

extern "C" {

int ag_sim_box_push(const int32_t *n, const float *q, const float *m, const float *body, const float *inv, const int32_t *n_push,
                    const float *push, float *pose, float *vel, float *obj, float *eef, float *pose_frames, int32_t *n_frames, int E, int n_max,
                    int F_max, int n_push_max, int substeps, int iters, int record_every, int settle, float h, float g, float mu, float r, float R,
                    float eps, float v_rest, float cap, float lift, ag_stream_t stream)
{
    if (!n || !q || !m || !body || !inv || !n_push || !push || !pose || !vel || !obj || !eef || !pose_frames || !n_frames)
        return ag_fail(AG_ERR_ARG, "ag_sim_box_push: null argument");
    if (int err = sim_check_schedule("ag_sim_box_push", E, n_max, 4, AG_SIM_BOX_MAX_PARTICLES, "AG_SIM_BOX_MAX_PARTICLES", F_max, n_push_max, 1,
                                     substeps, true, iters, record_every, settle, h, "push"))
        return err;
    if (!(eps > 0.f) || !((mu * g) / eps <= kBoxKMax))      // with |rho| <= 8 this keeps 1024 scaled terms inside 2^51
        return ag_fail(AG_ERR_ARG, "ag_sim_box_push: (mu g) / eps = %g outside (0, %g]", (double)((mu * g) / eps), (double)kBoxKMax);
    BoxPushArgs a{n, n_push, q, m, body, inv, push, pose, vel, obj, eef, pose_frames, n_frames, n_max, F_max, n_push_max, substeps, iters,
                  record_every, settle, h, g, mu, r, R, eps, v_rest, cap, lift};
    hipLaunchKernelGGL(box_push_kernel, dim3(E), dim3(kBoxThreads), 0, static_cast<hipStream_t>(stream), a);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

}  // extern "C"
