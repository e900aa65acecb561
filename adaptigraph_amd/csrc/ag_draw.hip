// ag_draw.hip — rollout and planning records drawn as RGBA images: discs and thick segments between projected points, in paint order over a
// background.  It stands in for the drawing the reference does with cv2 (src/dynamics/rollout/graph.py:44-230 `visualize_graph`,
// src/planning/plan_utils.py:104-300 `visualize_img`); the arithmetic is the host statement's (adaptigraph_amd/viz.py:draw_host), operation for
// operation: the projection float64 on float32 inputs with every product and sum rounded separately (the library is built with
// -ffp-contract=off), everything after it integers.  Our coverage rule, NOT cv2's Bresenham lines or its anti-aliasing.
//
// Two launches on the caller's stream.  (1) project_kernel: point i in camera c -> the pixel pair scratch[(c n_pts + i) 2 ..], or kInvalid in
// x.  (2) draw_kernel, in the shape of render_depth_kernel: one workgroup of 256 threads per (frame, tile of kTile x kTile pixels), every
// thread the pixels (u, v + 8 j), j = 0 .. 3 of its tile.  The frame's primitives pass through LDS in chunks of kChunk: thread t of a chunk
// loads primitive base + t, its endpoints and its style and bounds it by a pixel box (endpoints +- size); the primitives whose box meets the
// tile are compacted into an LDS list by ballot rank, so the list is in ASCENDING primitive index -- the paint order (an atomic counter would
// lose it).  Every thread then walks the list for its own pixels with `base` and `top` in registers and writes each pixel once, as one
// 32-bit store.  No atomics, no traffic between workgroups; every barrier is reached by all threads (the trip count of the chunk loop
// depends on the frame alone).
//
// Range of the coverage test, all int64.  A valid coordinate is at most 16 383 in magnitude, a pixel lies in 0 .. 4 095 and a size is at most
// 64, so every component of q = p - a (or p - b) is at most 16 383 + 4 095 = 20 478 and of d = b - a at most 32 766 in magnitude:
//   |s|, |X| <= 2 * 20 478 * 32 766 < 1.35e9;  4 X^2 < 4 * (1.35e9)^2 = 7.3e18 < 2^63 = 9.22e18  (the corners reach 1.81e18);
//   L2 <= 2 * 32 766^2 < 2.15e9;  w^2 L2 <= 4 096 * 2.15e9 < 8.9e12;  4 |q|^2 <= 8 * 20 478^2 < 3.4e9.
#include "ag_block_dev.h"
#include "ag_host.h"

namespace {

constexpr int kTile = AG_RENDER_TILE;
constexpr int kChunk = AG_RENDER_CHUNK;
constexpr int kBlock = 256;
constexpr int kPix = kTile * kTile / kBlock;      // pixels per thread
constexpr int kRowStep = kBlock / kTile;          // rows between a thread's pixels
constexpr int kInvalid = INT32_MIN;               // x of a point that does not project
constexpr int kMaxCoord = AG_DRAW_MAX_COORD;
constexpr int kMaxSize = AG_DRAW_MAX_SIZE;
static_assert(kChunk == kBlock, "one primitive of a chunk per thread");
static_assert(kTile * kTile % kBlock == 0 && kBlock % kTile == 0, "a thread's pixels share a column");

__global__ __launch_bounds__(kBlock) void project_kernel(const float *__restrict__ pts, int n_pts, const double *__restrict__ cams, int C,
                                                         double near, int32_t *__restrict__ scratch)
{
    const long long at = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (at >= (long long)n_pts * C) return;
    const int c = (int)(at / n_pts), i = (int)(at % n_pts);
    const double *k = cams + 25 * (size_t)c, *R = k + 9, *t = k + 18;
    const double fx = k[21], fy = k[22], cx = k[23], cy = k[24];
    const float *p = pts + (size_t)i * 3;
    const double d0 = (double)p[0] - t[0], d1 = (double)p[1] - t[1], d2 = (double)p[2] - t[2];
    const double c0 = (R[0] * d0 + R[3] * d1) + R[6] * d2;      // R^T (p - t)
    const double c1 = (R[1] * d0 + R[4] * d1) + R[7] * d2;
    const double c2 = (R[2] * d0 + R[5] * d1) + R[8] * d2;
    int x = kInvalid, y = 0;
    if (c2 > near) {
        const double xt = trunc(fx * (c0 / c2) + cx), yt = trunc(fy * (c1 / c2) + cy);
        if (fabs(xt) <= (double)kMaxCoord && fabs(yt) <= (double)kMaxCoord) {      // (a NaN or an infinity fails the comparison)
            x = (int)xt;
            y = (int)yt;
        }
    }
    scratch[2 * at] = x;
    scratch[2 * at + 1] = y;
}

__device__ __forceinline__ int blend_channel(int top, int base, int alpha) { return (top * alpha + base * (256 - alpha) + 128) >> 8; }

__global__ __launch_bounds__(kBlock) void draw_kernel(const int32_t *__restrict__ scratch, int n_pts, const int32_t *__restrict__ prims, int n_prim,
                                                      const int32_t *__restrict__ styles, int n_style, const int32_t *__restrict__ frames, int C,
                                                      int H, int W, int tiles_x, int tiles_y, int alpha, int bg_mode, const void *__restrict__ bg,
                                                      int n_bg, const int32_t *__restrict__ palette, int n_pal, int color0, int color1,
                                                      uint32_t *__restrict__ out)
{
    __shared__ int s_ax[kChunk], s_ay[kChunk], s_dx[kChunk], s_dy[kChunk], s_ww[kChunk], s_meta[kChunk], s_col[kChunk];
    __shared__ int s_cnt[kBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles = tiles_x * tiles_y, tile = (int)(blockIdx.x % (unsigned)tiles), f = (int)(blockIdx.x / (unsigned)tiles);
    const int u0 = (tile % tiles_x) * kTile, v0 = (tile / tiles_x) * kTile;
    const int cam = frames[4 * f], first = frames[4 * f + 1], count = frames[4 * f + 2], bgi = frames[4 * f + 3];
    // the frame's primitives lo .. hi - 1, clipped to 0 .. n_prim; none for a camera that does not exist
    long long lo64 = first < 0 ? 0 : first, hi64 = (long long)first + (long long)count;
    if (hi64 > n_prim) hi64 = n_prim;
    if (cam < 0 || cam >= C || count < 0 || hi64 < lo64) hi64 = lo64;
    const int lo = (int)lo64, hi = (int)hi64;
    const int32_t *proj = scratch + 2 * (size_t)(cam < 0 || cam >= C ? 0 : cam) * n_pts;

    const int u = u0 + tid % kTile, vb = v0 + tid / kTile;
    int base[kPix], top[kPix];
    bool over[kPix];
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        const int v = vb + kRowStep * j;
        int col = color0;
        if (u < W && v < H && bg_mode != 0 && bgi >= 0 && bgi < n_bg) {
            const size_t at = ((size_t)bgi * H + v) * W + u;
            if (bg_mode == 1) {
                const uint32_t px = static_cast<const uint32_t *>(bg)[at];      // bytes R, G, B, A
                col = (int)(((px & 0xffu) << 16) | (px & 0xff00u) | ((px >> 16) & 0xffu));
            } else {
                const int id = static_cast<const int32_t *>(bg)[at];
                col = id >= 0 ? palette[id % n_pal] : id == -1 ? color0 : color1;
            }
        }
        base[j] = col & 0xffffff;
        top[j] = 0;
        over[j] = false;
    }

    for (int start = lo; start < hi; start += kChunk) {
        const int i = start + tid;
        bool take = false;
        int ax = 0, ay = 0, dx = 0, dy = 0, ww = 0, meta = 0, col = 0;
        if (i < hi) {
            const int pa = prims[4 * (size_t)i], pb = prims[4 * (size_t)i + 1], st = prims[4 * (size_t)i + 2];
            if (pa >= 0 && pa < n_pts && pb >= 0 && pb < n_pts && st >= 0 && st < n_style) {
                const int kind = styles[4 * st], size = styles[4 * st + 1], layer = styles[4 * st + 2];
                ax = proj[2 * pa];
                ay = proj[2 * pa + 1];
                const int bx = kind == 0 ? ax : proj[2 * pb], by = kind == 0 ? ay : proj[2 * pb + 1];
                const bool valid = (kind == 0 || kind == 1) && size >= 0 && size <= kMaxSize && (layer == 0 || layer == 1) &&
                                   ax != kInvalid && bx != kInvalid;
                if (valid) {
                    dx = bx - ax;
                    dy = by - ay;
                    ww = size * size;
                    meta = kind | (layer << 1);
                    col = styles[4 * st + 3] & 0xffffff;
                    const int xl = min(ax, bx) - size, xh = max(ax, bx) + size, yl = min(ay, by) - size, yh = max(ay, by) + size;
                    take = !(xl > u0 + kTile - 1 || xh < u0 || yl > v0 + kTile - 1 || yh < v0);
                }
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
            s_ax[at] = ax; s_ay[at] = ay; s_dx[at] = dx; s_dy[at] = dy; s_ww[at] = ww; s_meta[at] = meta; s_col[at] = col;
        }
        __syncthreads();      // the list is in; s_cnt is free for the next chunk
        for (int s = 0; s < total; ++s) {
            const long long pax = s_ax[s], pay = s_ay[s], pdx = s_dx[s], pdy = s_dy[s], pww = s_ww[s];
            const int pmeta = s_meta[s], pcol = s_col[s];
            const long long L2 = pdx * pdx + pdy * pdy;
#pragma unroll
            for (int j = 0; j < kPix; ++j) {
                const long long qx = (long long)u - pax, qy = (long long)(vb + kRowStep * j) - pay;
                bool hit;
                if ((pmeta & 1) == 0) {
                    hit = qx * qx + qy * qy <= pww;
                } else {
                    const long long sp = qx * pdx + qy * pdy;
                    if (L2 == 0 || sp < 0) {
                        hit = 4 * (qx * qx + qy * qy) <= pww;
                    } else if (sp > L2) {
                        const long long rx = qx - pdx, ry = qy - pdy;
                        hit = 4 * (rx * rx + ry * ry) <= pww;
                    } else {
                        const long long X = qx * pdy - qy * pdx;
                        hit = 4 * (X * X) <= pww * L2;
                    }
                }
                if (hit) {
                    if (pmeta & 2) { top[j] = pcol; over[j] = true; }
                    else base[j] = pcol;
                }
            }
        }
    }

#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        const int v = vb + kRowStep * j;
        if (u >= W || v >= H) continue;
        const int b = base[j], t = over[j] ? top[j] : b;
        const int r = blend_channel((t >> 16) & 0xff, (b >> 16) & 0xff, alpha), g = blend_channel((t >> 8) & 0xff, (b >> 8) & 0xff, alpha),
                  bl = blend_channel(t & 0xff, b & 0xff, alpha);
        out[((size_t)f * H + v) * W + u] = (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)bl << 16) | 0xff000000u;
    }
}

}  // namespace

extern "C" {

size_t ag_draw_scratch_bytes(int n_pts, int C)
{
    if (n_pts < 0 || C < 1) return 0;
    return (size_t)(n_pts > 0 ? n_pts : 1) * (size_t)C * 2 * sizeof(int32_t);
}

int ag_draw(const float *pts, int n_pts, const int32_t *prims, int n_prim, const int32_t *styles, int n_style, const int32_t *frames, int F,
            const double *cams, int C, const double *near, int H, int W, int alpha, int bg_mode, const void *bg, int n_bg, const int32_t *palette,
            int n_pal, int color0, int color1, void *scratch, size_t scratch_bytes, uint8_t *out, ag_stream_t stream)
{
    if (!pts || !prims || !styles || !frames || !cams || !near || !scratch || !out) return ag_fail(AG_ERR_ARG, "ag_draw: null argument");
    if (F < 1 || C < 1) return ag_fail(AG_ERR_ARG, "ag_draw: F = %d, C = %d, both must be >= 1", F, C);
    if (n_pts < 0 || n_prim < 0 || n_style < 0)
        return ag_fail(AG_ERR_ARG, "ag_draw: n_pts = %d, n_prim = %d, n_style = %d, none may be negative", n_pts, n_prim, n_style);
    if (H < 1 || H > AG_RENDER_MAX_SIDE || W < 1 || W > AG_RENDER_MAX_SIDE)
        return ag_fail(AG_ERR_ARG, "ag_draw: H = %d, W = %d outside 1 .. %d (AG_RENDER_MAX_SIDE)", H, W, AG_RENDER_MAX_SIDE);
    if (alpha < 0 || alpha > 256) return ag_fail(AG_ERR_ARG, "ag_draw: alpha = %d outside 0 .. 256", alpha);
    if (bg_mode < 0 || bg_mode > 2) return ag_fail(AG_ERR_ARG, "ag_draw: background mode %d outside 0 .. 2", bg_mode);
    if (bg_mode != 0 && (!bg || n_bg < 1)) return ag_fail(AG_ERR_ARG, "ag_draw: background mode %d needs n_bg >= 1 images", bg_mode);
    if (bg_mode == 2 && (!palette || n_pal < 1)) return ag_fail(AG_ERR_ARG, "ag_draw: background mode 2 needs a palette of n_pal >= 1 colours");
    if (scratch_bytes < ag_draw_scratch_bytes(n_pts, C))
        return ag_fail(AG_ERR_ARG, "ag_draw: scratch of %zu bytes, %zu needed (ag_draw_scratch_bytes)", scratch_bytes, ag_draw_scratch_bytes(n_pts, C));
    const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
    const long long blocks = (long long)tiles_x * tiles_y * F;
    const long long proj_blocks = ((long long)n_pts * C + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffLL || proj_blocks > 0x7fffffffLL)
        return ag_fail(AG_ERR_ARG, "ag_draw: %lld tiles (F tiles per image) or %lld projection blocks exceed one launch", blocks, proj_blocks);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (proj_blocks > 0) {
        hipLaunchKernelGGL(project_kernel, dim3((unsigned)proj_blocks), dim3(kBlock), 0, st, pts, n_pts, cams, C, *near,
                           static_cast<int32_t *>(scratch));
        AG_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(draw_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, static_cast<const int32_t *>(scratch), n_pts, prims, n_prim, styles,
                       n_style, frames, C, H, W, tiles_x, tiles_y, alpha, bg_mode, bg, n_bg, palette, n_pal, color0, color1,
                       reinterpret_cast<uint32_t *>(out));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

}  // extern "C"
