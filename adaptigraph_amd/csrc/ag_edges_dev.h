// ag_edges_dev.h — the edge builder's device layer: what ag_edges_select.hip (which senders does each receiver keep), ag_edges.hip (the lists the model
// reads) and ag_shared.hip (can a tool touch a particle at all) must state the SAME way, written once.  No kernels here.
//
// Exactness contract (bit-for-bit edge sets; a single flipped edge moves the outputs by O(1e-2)):
//   d_ij  = ((dx*dx + dy*dy) + dz*dz) in fp32 with separately rounded products (the sources are compiled with -ffp-contract=off) —
//           bit-identical to torch.sum(s_diff ** 2, -1) on the reference's CPU path
//   masks : d = 1e10 unless mask[i] && mask[j]; d = 1e10 for tool-tool pairs            (graph.py:114,118)
//   in radius  <=>  (d - thr) < 0                                                         (graph.py:125)
//   row top-k : the k = min(N, topk) smallest d of the row; restricted to in-radius candidates this is the
//           k nearest in-radius senders (every in-radius entry is smaller than every other entry);
//           exact-distance ties go to the lower sender index (torch.topk leaves them unspecified)
//   connect_tools_all : the two variants' override rules, including the batch variant's per-sample
//           batch_mask and the tool->tool edges it keeps (graph.py:77-80 vs :134-144)
//   order : (receiver, sender) ascending == adj_matrix.nonzero() row-major order (graph.py:151)
#pragma once
#include "ag_block_dev.h"
#include "ag_common.h"

namespace {

// ---- the pair test ----
__device__ __forceinline__ float pair_dist(float xi, float yi, float zi, float xj, float yj, float zj)
{
    const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
    return (dx * dx + dy * dy) + dz * dz;
}
constexpr float kMaskedDist = 1e10f;      // the distance of a masked pair: never in radius
__device__ __forceinline__ bool in_radius(float d, float thr) { return (d - thr) < 0.0f; }

// ---- the sender word of `sorted` (.w of a binned particle): its index in the sample, and whether it is a tool ----
constexpr int kSenderIndexMask = 0x3fffffff, kSenderToolBit = 0x40000000;
__device__ __forceinline__ int sender_word(int j, bool tool) { return j | (tool ? kSenderToolBit : 0); }
__device__ __forceinline__ int sender_index(int w) { return w & kSenderIndexMask; }
__device__ __forceinline__ int sender_is_tool(int w) { return w & kSenderToolBit; }      // (non-zero: a tool)

// A thread caches up to this many of a sample's particles (or their flags) in registers, all their loads in flight together:
// N <= 256 * kThreadSlots = 4 352; beyond that the kernels read them in their loops.
constexpr int kThreadSlots = 17;

// ---- one sample of a call: where its inputs, its threshold and its grid (EdgeGrid of ag_common.h, written by bin_kernel) are, and what a row
// may keep.  Pointers, so that a kernel loads the grid and the threshold where its own schedule wants them. ----
struct EdgeSample {
    const float *pos;
    const uint8_t *mk, *tl;
    EdgeGrid *grid;
    int32_t *cstart;            // (ncell + 1) first slot of every cell in `sorted`
    float4 *sorted;             // x, y, z, sender word: the valid particles in cell order
    const float *thr;           // (B) -> this sample's squared radius
    int k;                      // min(N, topk)
};
__device__ __forceinline__ EdgeSample edge_sample(const AgEdgeArgs &a, int b)
{
    EdgeSample s;
    s.pos = a.pos + (size_t)b * a.pos_stride;
    s.mk = a.mask + (size_t)b * a.N;
    s.tl = a.tool + (size_t)b * a.N;
    s.thr = a.thr_sq + b;
    s.grid = a.grid + b;
    s.cstart = a.cell_start + (size_t)b * (kCellMax + 1);
    s.sorted = a.sorted + (size_t)b * a.N;
    s.k = a.N < a.topk ? a.N : a.topk;
    return s;
}

// ---- the grid: x fastest, so the 3 x-neighbour cells of a (z, y) row are one contiguous range of `sorted` ----
__device__ __forceinline__ int cell_coord(float x, float x0, float inv, int n)
{
    const int c = (int)((x - x0) * inv);
    return c < 0 ? 0 : (c >= n ? n - 1 : c);
}
__device__ __forceinline__ int cell_id(const EdgeGrid &g, float x, float y, float z)
{
    return (cell_coord(z, g.z0, g.inv, g.nz) * g.ny + cell_coord(y, g.y0, g.inv, g.ny)) * g.nx + cell_coord(x, g.x0, g.inv, g.nx);
}
// The neighbourhood of a receiver's cell: rows r = 0..8, (dz, dy) = (r / 3 - 1, r % 3 - 1); a row that lies inside the grid is the range
// [p0, p1) of `sorted` that covers its cells x_lo..x_hi.
struct CellRows { int x_lo, x_hi, iy, iz; };
struct SortedRange { bool in_grid; int p0, p1; };
__device__ __forceinline__ CellRows cell_rows(const EdgeGrid &g, float x, float y, float z)
{
    const int ix = cell_coord(x, g.x0, g.inv, g.nx), iy = cell_coord(y, g.y0, g.inv, g.ny), iz = cell_coord(z, g.z0, g.inv, g.nz);
    return {ix > 0 ? ix - 1 : 0, ix + 1 < g.nx ? ix + 1 : g.nx - 1, iy, iz};
}
__device__ __forceinline__ SortedRange cell_row(const EdgeGrid &g, const int32_t *cstart, const CellRows &c, int r)
{
    const int z2 = c.iz + r / 3 - 1, y2 = c.iy + r % 3 - 1;
    if (z2 < 0 || z2 >= g.nz || y2 < 0 || y2 >= g.ny) return {false, 0, 0};
    const int base = (z2 * g.ny + y2) * g.nx;
    const int p1 = cstart[base + c.x_hi + 1];
    return {true, cstart[base + c.x_lo], p1};
}

// ---- a wave's candidate list in LDS: (d, j) pairs in ascending-j order of arrival, at most kCand of them ----
constexpr int kCand = 384;     // per-wave candidate list capacity; pruned to top-k whenever it could overflow

__device__ __forceinline__ void wave_lds_fence()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// keep only the k best (d, j)-ordered candidates, preserving ascending-j order; returns new count
__device__ int prune_topk(float *cd, int *cj, int cnt, int k, int lane)
{
    unsigned keepbits = 0;
    for (int base = 0, ch = 0; base < cnt; base += 64, ++ch) {
        const int idx = base + lane;
        const bool have = idx < cnt;
        const float d = have ? cd[idx] : 0.f;
        const int jj = have ? cj[idx] : 0;
        int rank = 0;
        for (int t = 0; t < cnt; ++t) {
            const float dt = cd[t];
            const int jt = cj[t];
            rank += (dt < d) || (dt == d && jt < jj);
        }
        if (have && rank < k) keepbits |= 1u << ch;
    }
    wave_lds_fence();
    int newcnt = 0;
    for (int base = 0, ch = 0; base < cnt; base += 64, ++ch) {
        const int idx = base + lane;
        const bool have = idx < cnt;
        const float d = have ? cd[idx] : 0.f;
        const int jj = have ? cj[idx] : 0;
        const bool keep = (keepbits >> ch) & 1u;
        const unsigned long long bal = __ballot(keep);
        wave_lds_fence();   // all lanes hold their (d, j) before anyone overwrites a slot
        if (keep) {
            const int pos = newcnt + ballot_rank(bal, lane);
            cd[pos] = d;
            cj[pos] = jj;
        }
        newcnt += __popcll(bal);
        wave_lds_fence();
    }
    return newcnt;
}

// the lanes with `c` set append their (d, j) in lane order; returns the new count
__device__ __forceinline__ int cand_append(float *cd, int *cj, int cnt, bool c, float d, int j, int k, int lane)
{
    const unsigned long long bal = __ballot(c);
    if (bal) {
        if (cnt + 64 > kCand) cnt = prune_topk(cd, cj, cnt, k, lane);   // wave-uniform; keeps the append below in bounds
        if (c) {
            const int p = cnt + ballot_rank(bal, lane);
            cd[p] = d;
            cj[p] = j;
        }
        cnt += __popcll(bal);
        wave_lds_fence();
    }
    return cnt;
}

// ---- connect_tools_all ----
// batch_mask (graph.py:123,135): some tool receiver of the sample keeps an edge from a non-tool sender.  `hit`: this thread saw one.
__device__ __forceinline__ void note_batch_mask(const AgEdgeArgs &a, int b, bool hit)
{
    if (a.connect && a.variant == 1 && hit) atomicOr(&a.flag[b], 1);
}
// the override of a receiver's row: merge {kept object senders} with {all tool senders}.
//   single (graph.py:77-80): tool receivers end with no edges; batch (:134-144): gated by batch_mask, and tool receivers
//   keep tool->tool edges (incl. the self loop) when it is set.
struct ConnectRule { bool add_tools, keep_sel; };
__device__ __forceinline__ ConnectRule connect_rule(const AgEdgeArgs &a, int b, bool mi, bool ti)
{
    return {mi && (a.variant == 1 ? (a.flag[b] != 0) : !ti), !ti};
}

// ---- the n = rows x cap sender slots of a workgroup's rows, read coalesced by `for (i0 = threadIdx.x; i0 < n; i0 += kRowSlotStep)`:
// four loads of a thread in flight per trip, v[u] = slot i0 + 256 * u (0 beyond n) ----
constexpr int kRowSlotStep = 4 * 256;
__device__ __forceinline__ void load_row_slots(const int32_t *src, int n, int i0, int (&v)[4])
{
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = i0 + 256 * u < n ? src[i0 + 256 * u] : 0;
}

}  // namespace
