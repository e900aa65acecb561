// ag_edges_select.hip — radius graph + per-receiver top-k: WHICH senders does each receiver keep.  Out: sel0 (B*N, cap0) ascending sender ids,
// deg (B*N), and with connect_tools_all the batch_mask word `flag` (B); ag_edges.hip turns those rows into the lists the model reads.
//
// Replaces the dense (B,N,N,3) difference tensor and the (B,N,N) distance / top-k matrices of construct_edges_from_states (variant 0,
// src/dynamics/dataset/graph.py:38-89) and construct_edges_from_states_batch (variant 1, graph.py:91-156), with no host sync.  The pair test and
// its exactness contract: ag_edges_dev.h.
#include "ag_edges_dev.h"

namespace {

constexpr int kRowsPerBlock = 16;

__global__ __launch_bounds__(256) void select_kernel(AgEdgeArgs a)
{
    // dynamic LDS: the sample's particle table staged once per block (SoA x|y|z + a 2-bit flag per particle),
    // then per-wave candidate lists.  Every receiver row of the block re-reads it N/64 times.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.y, N = a.N;
    if (a.active && !a.active[b]) return;      // (shared-state rollout: this sample's graph is the base sample's)
    const int Np = (N + 63) & ~63;
    float *sx = reinterpret_cast<float *>(smem), *sy = sx + Np, *sz = sy + Np;
    unsigned char *sf = reinterpret_cast<unsigned char *>(sz + Np);          // bit0 = mask, bit1 = tool
    float *s_d = reinterpret_cast<float *>(sf + Np);
    int *s_j = reinterpret_cast<int *>(s_d + 4 * kCand);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *cd = s_d + wave * kCand;
    int *cj = s_j + wave * kCand;
    const EdgeSample s = edge_sample(a, b);
    for (int j = threadIdx.x; j < Np; j += 256) {
        const bool in = j < N;
        sx[j] = in ? s.pos[j * 3] : 0.f;
        sy[j] = in ? s.pos[j * 3 + 1] : 0.f;
        sz[j] = in ? s.pos[j * 3 + 2] : 0.f;
        sf[j] = in ? (unsigned char)((s.mk[j] ? 1 : 0) | (s.tl[j] ? 2 : 0)) : 0;   // padding: invalid sender
    }
    __syncthreads();
    const float thr = *s.thr;

    for (int rr = wave; rr < kRowsPerBlock; rr += 4) {
        const int i = blockIdx.x * kRowsPerBlock + rr;
        if (i >= N) break;   // wave-uniform
        const float xi = sx[i], yi = sy[i], zi = sz[i];
        const bool mi = sf[i] & 1, ti = sf[i] & 2;
        int cnt = 0;
        for (int j0 = 0; j0 < Np; j0 += 64) {
            const int j = j0 + lane;
            const unsigned fj = sf[j];
            float d = pair_dist(xi, yi, zi, sx[j], sy[j], sz[j]);
            if (!(mi && (fj & 1))) d = kMaskedDist;          // also kills the j >= N padding (flag 0)
            if (ti && (fj & 2)) d = kMaskedDist;
            cnt = cand_append(cd, cj, cnt, in_radius(d, thr), d, j, s.k, lane);
        }
        if (cnt > s.k) cnt = prune_topk(cd, cj, cnt, s.k, lane);
        const size_t row = (size_t)b * N + i;
        const int jsel = lane < cnt ? cj[lane] : -1;
        if (lane < cnt) a.sel0[row * a.cap0 + lane] = jsel;
        if (lane == 0) a.deg[row] = cnt;       // provisional when connect_tools_all: finalize_connect_kernel rewrites it
        if (a.connect) {
            const bool hit = ti && lane < cnt && !(sf[jsel < 0 ? 0 : jsel] & 2);
            note_batch_mask(a, b, __ballot(hit) && lane == 0);      // (the ballot is taken by every lane, before the call: lane 0 notes for the wave)
        }
        wave_lds_fence();
    }
}

// ---- uniform-grid ("cell list") candidate search -------------------------------------------------------------
// For N in the thousands the O(N^2) scan above dominates the whole step (cloth-4k: 16.8 M pair tests per graph).
// bin_kernel sorts the valid particles of a sample into cubic cells of edge >= radius * 1.002 (one workgroup per
// sample, counting sort in LDS, x fastest so the 3 x-neighbour cells are one contiguous range); select_cells_kernel
// then tests only the <= 9 ranges around the receiver.  The candidate SET is exactly the in-radius set of the brute
// force scan (any pair with fp32 d < thr lies in adjacent cells: |dx|/cs <= 0.998 plus < 1e-3 of fp32 rounding in the
// cell coordinate), the distance arithmetic and the (d, j) ranking are the same code, and the <= k survivors are
// re-sorted by sender index, so the emitted edge lists are bit-identical (tests compare both paths to the oracle).
__global__ __launch_bounds__(256) void bin_kernel(AgEdgeArgs a)
{
    __shared__ int cnt[kCellMax];
    __shared__ float red[6][4];
    __shared__ EdgeGrid G;
    if ((int)blockIdx.x >= a.B) {       // rider workgroups (ag_rollout): the model step's per-node input rows of the edge features, a function of the state only
        const int gt = ((int)blockIdx.x - a.B) * 256 + (int)threadIdx.x;
        if (a.active && gt < a.B * a.N && !a.active[gt / a.N]) return;      // (no private edge names a node of an inactive sample)
        ag_edge_node_tab_row(a.tab_state, a.tab_attrs, a.tab_pinst, a.tab_n_inst, a.tab_n_p, a.B, a.N, a.tab_out, a.tab_status, gt,
                             a.self_attrs ? (long long)a.self_class_row0 : -1);
        return;
    }
    if (a.active && !a.active[blockIdx.x]) return;
    const int b = blockIdx.x, N = a.N, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // (the kernel that WRITES a sample's grid: its own pointers, at the places they have always been computed)
    const float *pos = a.pos + (size_t)b * a.pos_stride;
    const uint8_t *mk = a.mask + (size_t)b * N, *tl = a.tool + (size_t)b * N;
    // The sample's particles are read ONCE, all loads of a thread in flight together (kThreadSlots), and the three passes below
    // run from registers; a plain `if (mk[j]) ... pos[j]` loop per pass is a chain of dependent round trips (r05: 16 -> 8 us at 256 x 1 001).
    const bool cached = N <= 256 * kThreadSlots;
    float px[kThreadSlots], py[kThreadSlots], pz[kThreadSlots];
    unsigned vbits = 0, tbits = 0;
    if (cached) {
        unsigned char mv[kThreadSlots], tv[kThreadSlots];
#pragma unroll
        for (int i = 0; i < kThreadSlots; ++i) {
            const int j = tid + 256 * i, jc = j < N ? j : 0;
            mv[i] = mk[jc]; tv[i] = tl[jc];
            px[i] = pos[jc * 3]; py[i] = pos[jc * 3 + 1]; pz[i] = pos[jc * 3 + 2];
        }
#pragma unroll
        for (int i = 0; i < kThreadSlots; ++i) {
            if (tid + 256 * i < N && mv[i]) vbits |= 1u << i;
            if (tv[i]) tbits |= 1u << i;
        }
    }
    // f(j, x, y, z, is_tool) for every valid particle of this thread
    auto for_valid = [&](auto &&f) {
        if (cached) {
#pragma unroll
            for (int i = 0; i < kThreadSlots; ++i)
                if (vbits >> i & 1u) f(tid + 256 * i, px[i], py[i], pz[i], (tbits >> i & 1u) != 0);
        } else {
            for (int j = tid; j < N; j += 256)
                if (mk[j]) f(j, pos[j * 3], pos[j * 3 + 1], pos[j * 3 + 2], tl[j] != 0);
        }
    };
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for_valid([&](int, float x, float y, float z, bool) {
        lo[0] = fminf(lo[0], x); hi[0] = fmaxf(hi[0], x);
        lo[1] = fminf(lo[1], y); hi[1] = fmaxf(hi[1], y);
        lo[2] = fminf(lo[2], z); hi[2] = fmaxf(hi[2], z);
    });
    for (int c = 0; c < 3; ++c) {
        for (int o = 32; o > 0; o >>= 1) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], o)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o)); }      // (wave_fmin / wave_fmax, the two chains interleaved)
        if (lane == 0) { red[c][wave] = lo[c]; red[3 + c][wave] = hi[c]; }
    }
    __syncthreads();
    if (tid == 0) {
        float mn[3], mx[3];
        for (int c = 0; c < 3; ++c) {
            mn[c] = four_wave_min(red[c]);
            mx[c] = four_wave_max(red[3 + c]);
            if (!(mx[c] >= mn[c])) { mn[c] = 0.f; mx[c] = 0.f; }     // no valid particle
        }
        float cs = sqrtf(a.thr_sq[b]) * 1.002f;
        if (!(cs > 1e-20f)) cs = 1e-20f;
        int nx = 1, ny = 1, nz = 1;
        // coarsen until the grid fits the LDS histogram (larger cells stay exact, only less selective).  Non-finite
        // extents (an Inf coordinate of a diverged rollout; NaNs never enter the min/max) or a cell size that overflows
        // fall back to ONE cell: every valid particle is then a candidate of every receiver and the pair test itself
        // decides, exactly like the reference, which yields no edge for a NaN/Inf distance (graph.py:121: `dis < thresh`).
        bool ok = true;
        for (int c = 0; c < 3; ++c) ok = ok && isfinite(mn[c]) && isfinite(mx[c]) && isfinite(mx[c] - mn[c]);
        for (int it = 0; ok; ++it) {
            const float fx = (mx[0] - mn[0]) / cs, fy = (mx[1] - mn[1]) / cs, fz = (mx[2] - mn[2]) / cs;
            if (fx < 8000.f && fy < 8000.f && fz < 8000.f) {
                nx = (int)fx + 1; ny = (int)fy + 1; nz = (int)fz + 1;
                if ((long long)nx * ny * nz <= kCellMax) break;
            }
            cs *= 2.0f;
            if (it > 300 || !isfinite(cs)) ok = false;
        }
        if (!ok) { nx = ny = nz = 1; cs = 1.0f; for (int c = 0; c < 3; ++c) if (!isfinite(mn[c])) mn[c] = 0.f; }
        G.x0 = mn[0]; G.y0 = mn[1]; G.z0 = mn[2]; G.inv = 1.0f / cs; G.nx = nx; G.ny = ny; G.nz = nz; G.total = 0;
    }
    __syncthreads();
    if (a.connect && tid == 0) a.flag[b] = 0;        // batch_mask of this sample (set by the selection kernels, read by finalize_connect)
    const EdgeGrid g = G;
    const int ncell = g.nx * g.ny * g.nz;
    for (int c = tid; c < ncell; c += 256) cnt[c] = 0;
    __syncthreads();
    for_valid([&](int, float x, float y, float z, bool) { atomicAdd(&cnt[cell_id(g, x, y, z)], 1); });
    __syncthreads();
    // exclusive scan of cnt[0..ncell): thread t owns cells [t*32, t*32+32)
    int local = 0;
    for (int c = tid * 32; c < tid * 32 + 32 && c < ncell; ++c) local += cnt[c];
    int total;
    int run = block_exclusive_scan(local, &total);
    int32_t *cs_out = a.cell_start + (size_t)b * (kCellMax + 1);
    for (int c = tid * 32; c < tid * 32 + 32 && c < ncell; ++c) {
        const int v = cnt[c];
        cnt[c] = run;            // becomes the running insertion offset
        cs_out[c] = run;
        run += v;
    }
    if (tid == 0) { cs_out[ncell] = total; EdgeGrid out = g; out.total = total; a.grid[b] = out; }
    __syncthreads();
    float4 *sorted = a.sorted + (size_t)b * N;
    for_valid([&](int j, float x, float y, float z, bool tool) {
        const int p = atomicAdd(&cnt[cell_id(g, x, y, z)], 1);
        sorted[p] = make_float4(x, y, z, __int_as_float(sender_word(j, tool)));
    });
}

__global__ __launch_bounds__(256) void select_cells_kernel(AgEdgeArgs a)
{
    __shared__ float s_d[4][kCand];
    __shared__ int s_j[4][kCand];
    const int b = blockIdx.y, N = a.N;
    if (a.active && !a.active[b]) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *cd = s_d[wave];
    int *cj = s_j[wave];
    const EdgeSample s = edge_sample(a, b);
    const EdgeGrid g = *s.grid;
    const float thr = *s.thr;

    for (int rr = wave; rr < kRowsPerBlock; rr += 4) {
        const int i = blockIdx.x * kRowsPerBlock + rr;
        if (i >= N) break;   // wave-uniform
        const size_t row = (size_t)b * N + i;
        const bool mi = s.mk[i], ti = s.tl[i];
        int cnt = 0;
        if (mi) {
            const float xi = s.pos[i * 3], yi = s.pos[i * 3 + 1], zi = s.pos[i * 3 + 2];
            // lanes 0..8 fetch the (dz, dy) neighbour ranges in ONE round trip; the concatenation of the ranges is
            // then swept 64 candidates at a time (a serial loop over the 9 ranges is a chain of dependent loads)
            const CellRows nb = cell_rows(g, xi, yi, zi);
            int len = 0, p0 = 0;
            if (lane < 9) {
                const SortedRange q = cell_row(g, s.cstart, nb, lane);
                p0 = q.p0;
                len = q.p1 - q.p0;
            }
            int incl = len;
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                const int y = __shfl_up(incl, o);
                if (lane >= o) incl += y;
            }
            const int total = __shfl(incl, 8);
            const int excl = incl - len;
            for (int tb = 0; tb < total; tb += 64) {
                const int t = tb + lane;
                int p = -1;
#pragma unroll
                for (int r = 0; r < 9; ++r) {
                    const int e_r = __shfl(excl, r), n_r = __shfl(len, r), p_r = __shfl(p0, r);
                    if (t >= e_r && t < e_r + n_r) p = p_r + (t - e_r);
                }
                bool c = false;
                float d = 0.f;
                int j = 0;
                if (p >= 0) {
                    const float4 sj = s.sorted[p];
                    const int w = __float_as_int(sj.w);
                    j = sender_index(w);
                    d = pair_dist(xi, yi, zi, sj.x, sj.y, sj.z);
                    if (sender_is_tool(w) && ti) d = kMaskedDist;   // tool-tool (graph.py:118); invalid senders are not binned
                    c = in_radius(d, thr);
                }
                cnt = cand_append(cd, cj, cnt, c, d, j, s.k, lane);
            }
            if (cnt > s.k) cnt = prune_topk(cd, cj, cnt, s.k, lane);
        }
        // the survivors arrive in cell order: emit them in ascending sender index (k <= 64: one per lane)
        const int jsel = lane < cnt ? cj[lane] : 0x7fffffff;
        int rank = 0;
        for (int t = 0; t < cnt; ++t) rank += __shfl(jsel, t) < jsel;
        if (lane < cnt) a.sel0[row * a.cap0 + rank] = jsel;
        if (lane == 0) a.deg[row] = cnt;
        if (a.connect) {
            const bool hit = ti && lane < cnt && !s.tl[jsel == 0x7fffffff ? 0 : jsel];
            note_batch_mask(a, b, __ballot(hit) && lane == 0);      // (the ballot is taken by every lane, before the call: lane 0 notes for the wave)
        }
        wave_lds_fence();
    }
}

// Lane-per-receiver variant of the cell search for the shipped top-k values: every lane walks the <= 9 cell ranges of
// its own receiver and keeps its K best (d, j) in registers (compare-exchange insertion), so 64 receivers are in
// flight per wave instead of one — the wave-per-receiver kernel above is a chain of dependent round trips per row.
template <int K>
__device__ __forceinline__ int lanes_exact(bool active, float xi, float yi, float zi, bool ti, const EdgeGrid &g, const int32_t *cstart,
                                           const float4 *sorted, float thr, float (&bd)[K], int (&bj)[K])
{
#pragma unroll
    for (int s = 0; s < K; ++s) { bd[s] = 3.0e38f; bj[s] = 0x7fffffff; }
    int cnt = 0;
    if (active) {
        const CellRows nb = cell_rows(g, xi, yi, zi);
        for (int r = 0; r < 9; ++r) {
            const SortedRange q = cell_row(g, cstart, nb, r);
            if (!q.in_grid) continue;
            for (int p = q.p0; p < q.p1; ++p) {
                const float4 sj = sorted[p];
                const int w = __float_as_int(sj.w);
                float d = pair_dist(xi, yi, zi, sj.x, sj.y, sj.z);
                if (sender_is_tool(w) && ti) d = kMaskedDist;   // tool-tool (graph.py:118); invalid senders are not binned
                if (in_radius(d, thr)) {
                    float cdv = d;
                    int cjv = sender_index(w);
#pragma unroll
                    for (int s = 0; s < K; ++s) {   // keep bd/bj ascending in (d, j); the loser falls through
                        const bool lt = (cdv < bd[s]) || (cdv == bd[s] && cjv < bj[s]);
                        const float td = lt ? bd[s] : cdv;
                        const int tj = lt ? bj[s] : cjv;
                        bd[s] = lt ? cdv : bd[s];
                        bj[s] = lt ? cjv : bj[s];
                        cdv = td;
                        cjv = tj;
                    }
                    cnt = cnt < K ? cnt + 1 : K;
                }
            }
        }
    }
    return cnt;
}

template <int K>
__global__ __launch_bounds__(256) void select_lanes_kernel(AgEdgeArgs a)
{
    const int b = blockIdx.y, N = a.N;
    if (a.active && !a.active[b]) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const EdgeSample sm = edge_sample(a, b);
    const EdgeGrid g = *sm.grid;
    const float thr = *sm.thr;
    const size_t row = (size_t)b * N + i;
    const bool mi = sm.mk[i], ti = sm.tl[i];
    float bd[K];
    int bj[K];
    const float xi = mi ? sm.pos[i * 3] : 0.f, yi = mi ? sm.pos[i * 3 + 1] : 0.f, zi = mi ? sm.pos[i * 3 + 2] : 0.f;
    const int cnt = lanes_exact<K>(mi, xi, yi, zi, ti, g, sm.cstart, sm.sorted, thr, bd, bj);
    bool hit = false;
#pragma unroll
    for (int s = 0; s < K; ++s)
        if (s < cnt) {
            int rank = 0;
#pragma unroll
            for (int t = 0; t < K; ++t) rank += (t < cnt && bj[t] < bj[s]) ? 1 : 0;
            a.sel0[row * a.cap0 + rank] = bj[s];        // ascending sender index
            hit = hit || (ti && !sm.tl[bj[s]]);
        }
    a.deg[row] = cnt;
    note_batch_mask(a, b, hit);
}

// The same search with packed keys (the default for all three shipped top-k values; it matters most at top-k 20, the granular
// configuration, where the insertion network IS the cost): ~40 in-radius
// candidates per receiver x 20 compare-exchange steps x 7 VALU ops, executed by the whole wave whenever any lane accepts.
//  * keys are ONE 32-bit word, (d as fixed point: floor(d * 2^(32-jb) / thr), in-radius d lies in [0, thr)) << jb | j, so a
//    compare-exchange step is v_min_u32 + v_max_u32 (2 ops instead of 7).  The quantisation is monotone (fp32 multiply and
//    floor are), so the K smallest keys are the K nearest senders EXACTLY unless the K-th and (K+1)-th candidates fall into the
//    same quantum; the network therefore carries K+1 entries and a receiver whose boundary is ambiguous is redone with the
//    exact (d, j) network.  21 bits of d at N ~ 2k: relative resolution 5e-7 of thr against ~1/40 between neighbouring order
//    statistics, i.e. ~1e-5 of the receivers (keeping the fp32 bit pattern's leading bits instead — 12 mantissa bits — sent
//    0.5 % of the receivers, hence every fourth WAVE, through the exact network: 0.21 ms instead of 0.12).  The in-radius test
//    itself is made on the full fp32 d.
//  * receivers are taken in CELL order (thread t = t-th binned particle), so the lanes of a wave walk the same cell ranges:
//    equal trip counts and broadcast candidate loads instead of 64 unrelated walks.
// Results are bit-identical to select_lanes_kernel / the brute-force scan (tests compare all paths with the oracle).
template <int K>
__global__ __launch_bounds__(256, 4) void select_lanes_packed_kernel(AgEdgeArgs a, int jb)
{
    const int b = blockIdx.y, N = a.N;
    if (a.active && !a.active[b]) return;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const EdgeSample sm = edge_sample(a, b);
    if (t < N && !sm.mk[t]) a.deg[(size_t)b * N + t] = 0;            // receivers that were not binned have no edges
    const EdgeGrid g = *sm.grid;      // (behind that store, as a vector load)
    const int32_t *cstart = sm.cstart;
    const float4 *sorted = sm.sorted;
    const float thr = *sm.thr;
    const bool active = t < g.total;
    const float4 me = active ? sorted[t] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int wi = __float_as_int(me.w);
    const int i = sender_index(wi);
    const bool ti = sender_is_tool(wi) != 0;
    const float xi = me.x, yi = me.y, zi = me.z;
    const unsigned jmask = (1u << jb) - 1u;
    const float qmax = (float)(1u << (32 - jb));                 // quanta in [0, thr): a power of two, exact in fp32
    const float qscale = qmax / thr;
    const unsigned qtop = (1u << (32 - jb)) - 1u;
    unsigned kl[K + 1];
#pragma unroll
    for (int s = 0; s <= K; ++s) kl[s] = 0xffffffffu;
    int tot = 0;
    if (active) {
        const CellRows nb = cell_rows(g, xi, yi, zi);
        for (int r = 0; r < 9; ++r) {
            const SortedRange q = cell_row(g, cstart, nb, r);
            if (!q.in_grid) continue;
            const int p1 = q.p1;
            // candidates four at a time, their loads in flight together (one load, then its tests, per trip was a memory round trip per candidate)
            for (int p = q.p0; p < p1; p += 4) {
                float4 sq[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) sq[u] = sorted[p + u < p1 ? p + u : p1 - 1];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (p + u >= p1) break;
                    const float4 sj = sq[u];
                    const int w = __float_as_int(sj.w);
                    float d = pair_dist(xi, yi, zi, sj.x, sj.y, sj.z);
                    if (sender_is_tool(w) && ti) d = kMaskedDist;
                    if (in_radius(d, thr)) {
                        const unsigned qd = min((unsigned)(d * qscale), qtop);      // monotone in d (d >= 0; a NaN never gets here)
                        unsigned key = (qd << jb) | (unsigned)sender_index(w);
#pragma unroll
                        for (int s = 0; s <= K; ++s) {
                            const unsigned lo = min(kl[s], key);
                            key = max(kl[s], key);
                            kl[s] = lo;
                        }
                        ++tot;
                    }
                }
            }
        }
    }
    int cnt = tot < K ? tot : K;
    const bool ambiguous = tot > K && ((kl[K - 1] ^ kl[K]) & ~jmask) == 0u;
    if (__ballot(ambiguous)) {          // rare: the exact network for those lanes (the others idle through it)
        float bd[K];
        int bj[K];
        const int c2 = lanes_exact<K>(ambiguous, xi, yi, zi, ti, g, cstart, sorted, thr, bd, bj);
        if (ambiguous) {
            cnt = c2;
#pragma unroll
            for (int s = 0; s < K; ++s) kl[s] = (unsigned)bj[s];
        }
    }
    // senders in ascending index order: odd-even transposition sort of the K sender ids (unused slots sort to the end)
    unsigned js[K];
#pragma unroll
    for (int s = 0; s < K; ++s) js[s] = s < cnt ? (kl[s] & (ambiguous ? 0x7fffffffu : jmask)) : 0x7fffffffu;
#pragma unroll
    for (int round = 0; round < K; ++round)
#pragma unroll
        for (int s = round & 1; s + 1 < K; s += 2) {
            const unsigned lo = min(js[s], js[s + 1]), hi = max(js[s], js[s + 1]);
            js[s] = lo;
            js[s + 1] = hi;
        }
    if (!active) return;
    const size_t row = (size_t)b * N + i;
    bool hit = false;
#pragma unroll
    for (int s = 0; s < K; ++s)
        if (s < cnt) {
            a.sel0[row * a.cap0 + s] = (int)js[s];
            hit = hit || (ti && !sm.tl[js[s]]);
        }
    a.deg[row] = cnt;
    note_batch_mask(a, b, hit);
}

// the lane-per-receiver kernels of top-k K: packed keys while they leave >= 16 bits for d (else nearly every boundary would be ambiguous)
template <int K>
bool launch_lanes(const AgEdgeArgs &a, hipStream_t s)
{
    if (a.cap0 != K || a.topk != K) return false;
    const dim3 lgrid((a.N + 255) / 256, a.B);
    int jb = 1;
    while ((1 << jb) < a.N) ++jb;
    if (jb <= 16) hipLaunchKernelGGL(select_lanes_packed_kernel<K>, lgrid, dim3(256), 0, s, a, jb);
    else hipLaunchKernelGGL(select_lanes_kernel<K>, lgrid, dim3(256), 0, s, a);
    return true;
}

}  // namespace

int ag_launch_select_edges(const AgEdgeArgs &a, hipStream_t s)
{
    const dim3 rgrid((a.N + kRowsPerBlock - 1) / kRowsPerBlock, a.B);      // a wave per receiver
    if (a.N < 256) {      // the brute-force scan
        if (a.connect) ag_launch_zero_words(a.flag, a.B, s);      // (on the cell path bin_kernel clears the batch_mask word: one fill launch per step less)
        const int Np = (a.N + 63) & ~63;
        hipLaunchKernelGGL(select_kernel, rgrid, dim3(256), (size_t)Np * 13 + 4 * kCand * 8, s, a);
        return 0;
    }
    const int nb_tab = a.tab_out ? (a.B * a.N + 255) / 256 : 0;        // rider workgroups follow the B binning ones
    hipLaunchKernelGGL(bin_kernel, dim3(a.B + nb_tab), dim3(256), 0, s, a);
    if (!launch_lanes<5>(a, s) && !launch_lanes<10>(a, s) && !launch_lanes<20>(a, s))
        hipLaunchKernelGGL(select_cells_kernel, rgrid, dim3(256), 0, s, a);
    return nb_tab ? AG_RIDER_TAB : 0;
}
