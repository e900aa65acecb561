// ag_render.hip — depth images of a particle scene from calibrated pinhole cameras: every particle a sphere, the table a plane.  It stands in for
// what the reference asks of its simulator's renderer (src/sim/sim_env/flex_env.py:151-189, :404-409); the arithmetic is the host statement's
// (adaptigraph_amd/render.py:render_depth_host), operation for operation: float64 on float32 inputs, every product and sum rounded separately
// (the library is built with -ffp-contract=off), only + - * / sqrt.
//
// A tiled gather rasteriser, one launch: one workgroup of 256 threads per (episode, camera, tile of kTile x kTile pixels), every thread the pixels
// (u, v + 8 j), j = 0 .. 3 of its tile.  The episode's particles pass through LDS in chunks of kChunk: thread t of a chunk moves particle
// base + t into the camera frame once and bounds its image by a pixel box; the spheres whose box meets the tile are compacted into an LDS list
// by ballot rank, so the list is in ASCENDING particle index (an atomic counter would lose that order, and with it the tie rule).  Every thread
// then walks the list for its own pixels with the best (d, id) in registers and writes each pixel once.  No atomics, no traffic between
// workgroups; every barrier is reached by all threads (the trip count of the chunk loop depends on the episode alone).
//
// The box is no part of the statement, only a superset of the pixels a sphere can hit: the sphere lies inside the box [c_0 +- r] x [c_1 +- r] x
// [c_2 +- r] of the camera frame, whose z is positive after the cull (near >= 0), so x / z over it is extreme at the corners; one pixel of
// margin on every side covers the roundings.  A box that cannot be trusted (z not positive, a NaN) counts as meeting every tile.
#include "ag_block_dev.h"
#include "ag_host.h"

namespace {

constexpr int kTile = AG_RENDER_TILE;
constexpr int kChunk = AG_RENDER_CHUNK;
constexpr int kBlock = 256;
constexpr int kPix = kTile * kTile / kBlock;      // pixels per thread
constexpr int kRowStep = kBlock / kTile;          // rows between a thread's pixels
static_assert(kChunk == kBlock, "one particle of a chunk per thread");
static_assert(kTile * kTile % kBlock == 0 && kBlock % kTile == 0, "a thread's pixels share a column");

__global__ __launch_bounds__(kBlock) void render_depth_kernel(const float *__restrict__ pts, const int32_t *__restrict__ n,
                                                              const float *__restrict__ radius, const double *__restrict__ cams,
                                                              const double *__restrict__ plane, const double *__restrict__ limits, int n_max, int C,
                                                              int H, int W, int tiles_x, int tiles_y, float *__restrict__ depth,
                                                              int32_t *__restrict__ id)
{
    __shared__ double s_c0[kChunk], s_c1[kChunk], s_c2[kChunk], s_cc[kChunk];
    __shared__ int s_i[kChunk];
    __shared__ int s_cnt[kBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles = tiles_x * tiles_y, tile = (int)(blockIdx.x % (unsigned)tiles), ec = (int)(blockIdx.x / (unsigned)tiles);
    const int c = ec % C, e = ec / C;
    const int u0 = (tile % tiles_x) * kTile, v0 = (tile / tiles_x) * kTile;
    const double *k = cams + 25 * (size_t)c, *R = k + 9, *t = k + 18;
    const double fx = k[21], fy = k[22], cx = k[23], cy = k[24];
    const double near = limits[0], far = limits[1];
    int ne = n[e];
    if (ne < 0 || ne > n_max) ne = 0;
    const double rr = (double)radius[e];

    const int u = u0 + tid % kTile, vb = v0 + tid / kTile;
    double qx[kPix], qy[kPix], A[kPix], best[kPix];
    int bid[kPix];
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        const double ud = (double)u, vd = (double)(vb + kRowStep * j);
        qx[j] = (k[0] * ud + k[1] * vd) + k[2];
        qy[j] = (k[3] * ud + k[4] * vd) + k[5];
        A[j] = (qx[j] * qx[j] + qy[j] * qy[j]) + 1.0;
        best[j] = INFINITY;
        bid[j] = -2;
    }
    const double tu0 = (double)u0, tu1 = (double)(u0 + kTile - 1), tv0 = (double)v0, tv1 = (double)(v0 + kTile - 1);

    for (int base = 0; base < ne; base += kChunk) {
        const int i = base + tid;
        bool take = false;
        double c0 = 0.0, c1 = 0.0, c2 = 0.0, cc = 0.0;
        if (i < ne) {
            const float *p = pts + ((size_t)e * n_max + i) * 3;
            const double d0 = (double)p[0] - t[0], d1 = (double)p[1] - t[1], d2 = (double)p[2] - t[2];
            c0 = (R[0] * d0 + R[3] * d1) + R[6] * d2;      // R^T (p - t)
            c1 = (R[1] * d0 + R[4] * d1) + R[7] * d2;
            c2 = (R[2] * d0 + R[5] * d1) + R[8] * d2;
            const double z1 = c2 - rr;
            if (z1 > near) {      // the cull rule of the statement
                cc = ((c0 * c0 + c1 * c1) + c2 * c2) - rr * rr;
                const double i1 = 1.0 / z1, i2 = 1.0 / (c2 + rr);
                const double xl = c0 - rr, xh = c0 + rr, yl = c1 - rr, yh = c1 + rr;
                const double ulo = floor(fx * fmin(xl * i1, xl * i2) + cx) - 1.0, uhi = ceil(fx * fmax(xh * i1, xh * i2) + cx) + 1.0;
                const double vlo = floor(fy * fmin(yl * i1, yl * i2) + cy) - 1.0, vhi = ceil(fy * fmax(yh * i1, yh * i2) + cy) + 1.0;
                take = !(z1 > 0.0) || !(ulo > tu1 || uhi < tu0 || vlo > tv1 || vhi < tv0);      // (a NaN bound fails every comparison: taken)
            }
        }
        const unsigned long long bal = __ballot(take);
        if (lane == 0) s_cnt[wave] = __popcll(bal);
        __syncthreads();      // the counts are in; every thread has left the list of the chunk before
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) {
            before += w < wave ? s_cnt[w] : 0;
            total += s_cnt[w];
        }
        if (take) {
            const int at = before + ballot_rank(bal, lane);      // < kChunk: at most one entry per thread
            s_c0[at] = c0; s_c1[at] = c1; s_c2[at] = c2; s_cc[at] = cc; s_i[at] = i;
        }
        __syncthreads();      // the list is in; s_cnt is free for the next chunk
        for (int s = 0; s < total; ++s) {
            const double a0 = s_c0[s], a1 = s_c1[s], a2 = s_c2[s], ac = s_cc[s];
            const int si = s_i[s];
#pragma unroll
            for (int j = 0; j < kPix; ++j) {
                const double B = (qx[j] * a0 + qy[j] * a1) + a2;
                const double disc = B * B - A[j] * ac;
                if (disc >= 0.0) {
                    const double d = (B - sqrt(disc)) / A[j];
                    if (d > near && d < far && d < best[j]) { best[j] = d; bid[j] = si; }      // strict: the lower index keeps a tie
                }
            }
        }
    }

    double pn[4] = {0.0, 0.0, 0.0, 0.0}, num = 0.0;
    if (plane) {
#pragma unroll
        for (int a = 0; a < 4; ++a) pn[a] = plane[a];
        num = pn[3] - ((pn[0] * t[0] + pn[1] * t[1]) + pn[2] * t[2]);
    }
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        const int v = vb + kRowStep * j;
        if (u >= W || v >= H) continue;
        if (plane) {
            const double w0 = (R[0] * qx[j] + R[1] * qy[j]) + R[2], w1 = (R[3] * qx[j] + R[4] * qy[j]) + R[5],
                         w2 = (R[6] * qx[j] + R[7] * qy[j]) + R[8];
            const double den = (pn[0] * w0 + pn[1] * w1) + pn[2] * w2;
            if (den != 0.0) {
                const double dp = num / den;
                if (dp > near && dp < far && dp < best[j]) { best[j] = dp; bid[j] = -1; }
            }
        }
        const size_t at = (((size_t)e * C + c) * H + v) * W + u;
        depth[at] = bid[j] == -2 ? 0.0f : (float)best[j];
        id[at] = bid[j];
    }
}

}  // namespace

extern "C" {

int ag_render_depth(const float *pts, const int32_t *n, const float *radius, const double *cams, const double *plane, const double *limits, int E,
                    int n_max, int C, int H, int W, float *depth, int32_t *id, ag_stream_t stream)
{
    if (!pts || !n || !radius || !cams || !limits || !depth || !id) return ag_fail(AG_ERR_ARG, "ag_render_depth: null argument");
    if (E < 1 || C < 1) return ag_fail(AG_ERR_ARG, "ag_render_depth: E = %d, C = %d, both must be >= 1", E, C);
    if (H < 1 || H > AG_RENDER_MAX_SIDE || W < 1 || W > AG_RENDER_MAX_SIDE)
        return ag_fail(AG_ERR_ARG, "ag_render_depth: H = %d, W = %d outside 1 .. %d (AG_RENDER_MAX_SIDE)", H, W, AG_RENDER_MAX_SIDE);
    if (n_max < 1 || n_max > AG_RENDER_MAX_PARTICLES)
        return ag_fail(AG_ERR_ARG, "ag_render_depth: n_max = %d outside 1 .. %d (AG_RENDER_MAX_PARTICLES)", n_max, AG_RENDER_MAX_PARTICLES);
    const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
    const long long blocks = (long long)tiles_x * tiles_y * E * C;
    if (blocks > 0x7fffffffLL) return ag_fail(AG_ERR_ARG, "ag_render_depth: %lld tiles (E C tiles per image) exceed one launch", blocks);
    hipLaunchKernelGGL(render_depth_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), pts, n, radius, cams, plane,
                       limits, n_max, C, H, W, tiles_x, tiles_y, depth, id);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

}  // extern "C"
