// ag_edges.hip — radius-graph + per-receiver top-k adjacency, emitted as receiver-sorted CSR/COO.
//
// Replaces construct_edges_from_states (variant 0, src/dynamics/dataset/graph.py:38-89) and
// construct_edges_from_states_batch (variant 1, graph.py:91-156), without the dense (B,N,N,3) difference
// tensor, the (B,N,N) distance/top-k matrices or the one-hot (B,E,N) outputs, and with no host sync.
// ag_edges_select.hip answers which senders each receiver keeps (sel0, deg, flag); this file turns those rows into the lists the
// model reads: the connect_tools_all override, the degree scan and the COO fill.  The exactness contract of both: ag_edges_dev.h.
#include "ag_edges_dev.h"

namespace {

// connect_tools_all overrides (connect_rule): merge {kept object senders} with {all tool senders} in ascending order.
// One THREAD per receiver: the kept senders are already ascending and at most top-k long, the sample's tool indices are
// compacted once per workgroup into LDS (ascending), so a row is a two-pointer merge of two short sorted lists.
// (A wave per receiver sweeping all N candidate senders was 45 % of the whole cloth-4k step.)
constexpr int kKeepFast = 8;          // finalize_connect_kernel: kept-sender lists of top-k <= 8 are merged from LDS
constexpr int kToolListMax = 8192;     // LDS-resident tool list; more tools than this take the sweep kernel below

__global__ __launch_bounds__(256) void finalize_connect_kernel(AgEdgeArgs a)
{
    extern __shared__ int tools[];
    __shared__ int wcount[4];
    __shared__ int kept[256 * kKeepFast];           // per-thread list of the kept NON-tool senders (fast path: top-k <= kKeepFast)
    const int b = blockIdx.y, N = a.N, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (a.active && !a.active[b]) return;
    const EdgeSample s = edge_sample(a, b);
    const uint8_t *tl = s.tl;
    // the tool flags of the sample, all of a thread's loads in flight together (kThreadSlots; beyond that they are read in the loop)
    unsigned tflag = 0;
    const bool flags_cached = N <= 256 * kThreadSlots;
    if (flags_cached) {
        unsigned char tv[kThreadSlots];
#pragma unroll
        for (int u = 0; u < kThreadSlots; ++u) tv[u] = tl[tid + 256 * u < N ? tid + 256 * u : 0];
#pragma unroll
        for (int u = 0; u < kThreadSlots; ++u) tflag |= (tid + 256 * u < N && tv[u]) ? 1u << u : 0u;
    }
    // this receiver's kept senders and their tool flags: two batches of loads instead of a chain of two dependent loads per sender
    const int i = blockIdx.x * 256 + tid;
    const size_t row = (size_t)b * N + (i < N ? i : 0);
    const int deg0 = i < N ? a.deg[row] : 0;
    const bool fast = a.cap0 <= kKeepFast;
    int nkept = 0;
    if (fast) {
        int sv[kKeepFast];
        unsigned char sf[kKeepFast];
#pragma unroll
        for (int u = 0; u < kKeepFast; ++u) sv[u] = u < deg0 ? a.sel0[row * a.cap0 + u] : 0;
#pragma unroll
        for (int u = 0; u < kKeepFast; ++u) sf[u] = tl[sv[u]];
#pragma unroll
        for (int u = 0; u < kKeepFast; ++u)
            if (u < deg0 && !sf[u]) kept[tid * kKeepFast + nkept++] = sv[u];
    }
    int nt = 0;
    if (flags_cached) {          // ordered compaction of the sample's tool indices with two barriers in all (the loop below: two per 256 slots)
        __shared__ int wc[kThreadSlots][4], wbase[kThreadSlots][4], s_total;
        unsigned long long bal[kThreadSlots];
#pragma unroll
        for (int u = 0; u < kThreadSlots; ++u) {
            bal[u] = __ballot((tflag >> u & 1u) != 0);
            if (lane == 0) wc[u][wave] = __popcll(bal[u]);
        }
        __syncthreads();
        if (tid == 0) {
            int run = 0;
            for (int u = 0; u < kThreadSlots; ++u)
                for (int w = 0; w < 4; ++w) { wbase[u][w] = run; run += wc[u][w]; }
            s_total = run;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kThreadSlots; ++u)
            if (tflag >> u & 1u) {
                const int slot = wbase[u][wave] + ballot_rank(bal[u], lane);
                if (slot < a.cap) tools[slot] = tid + 256 * u;      // only the first `cap` tools can reach a (cap-long) output row
            }
        nt = s_total;
        __syncthreads();
    } else
    for (int j0 = 0, it = 0; j0 < N; j0 += 256, ++it) {
        const int j = j0 + tid;
        const bool t = j < N && tl[j];
        const unsigned long long bal = __ballot(t);
        if (lane == 0) wcount[wave] = __popcll(bal);
        __syncthreads();
        int base = nt;
        for (int w = 0; w < wave; ++w) base += wcount[w];
        const int slot = base + ballot_rank(bal, lane);
        if (t && slot < a.cap) tools[slot] = j;      // only the first `cap` tools can reach a (cap-long) output row
        nt += wcount[0] + wcount[1] + wcount[2] + wcount[3];
        __syncthreads();
    }
    if (i >= N) return;
    const ConnectRule rule = connect_rule(a, b, s.mk[i], tl[i]);
    const int32_t *in = a.sel0 + row * a.cap0;
    int32_t *dst = a.sel + row * a.cap;
    const int na = rule.keep_sel ? deg0 : 0, nb = rule.add_tools ? (nt < a.cap ? nt : a.cap) : 0;
    int ia = 0, ib = 0, out = 0;
    if (fast) {          // both lists in LDS: the merge is a few dozen LDS reads and the row's stores
        const int *ka = kept + tid * kKeepFast;
        const int nk = rule.keep_sel ? nkept : 0;
        while (ia < nk || ib < nb) {
            const bool take_a = ia < nk && (ib >= nb || ka[ia] < tools[ib]);
            const int j = take_a ? ka[ia] : tools[ib];
            if (out < a.cap) dst[out] = j;
            ++out;
            if (take_a) ++ia; else ++ib;
        }
        a.deg[row] = out < a.cap ? out : a.cap;
        return;
    }
    int sa = -1;
    while (ia < na) { sa = in[ia]; if (!tl[sa]) break; ++ia; }          // tool senders among the kept ones come from list B
    while (ia < na || ib < nb) {
        const bool take_a = ia < na && (ib >= nb || sa < tools[ib]);
        const int j = take_a ? sa : tools[ib];
        if (out < a.cap) dst[out] = j;
        ++out;
        if (take_a) { ++ia; while (ia < na) { sa = in[ia]; if (!tl[sa]) break; ++ia; } }
        else ++ib;
    }
    a.deg[row] = out < a.cap ? out : a.cap;
}

// same result for samples with more than kToolListMax tools: one wave per receiver sweeps every candidate sender
__global__ __launch_bounds__(256) void finalize_connect_sweep_kernel(AgEdgeArgs a)
{
    const int b = blockIdx.y, N = a.N;
    if (a.active && !a.active[b]) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const EdgeSample s = edge_sample(a, b);
    const int i = blockIdx.x * 4 + wave;
    if (i >= N) return;
    const size_t row = (size_t)b * N + i;
    const bool mi = s.mk[i], ti = s.tl[i];
    const int deg0 = a.deg[row];
    const int mysel = lane < deg0 ? a.sel0[row * a.cap0 + lane] : -1;
    const ConnectRule rule = connect_rule(a, b, mi, ti);
    int out = 0;
    for (int j0 = 0; j0 < N; j0 += 64) {
        const int j = j0 + lane;
        const bool inb = j < N;
        const bool tj = inb && s.tl[j];
        bool member = false;
        if (rule.keep_sel) {
            for (int t = 0; t < deg0; ++t) {
                const int st = __shfl(mysel, t);
                member |= (st == j);
            }
            member = member && inb && !tj;
        }
        if (rule.add_tools && tj) member = true;
        const unsigned long long bal = __ballot(member);
        if (member) {
            const int p = out + ballot_rank(bal, lane);
            if (p < a.cap) a.sel[row * a.cap + p] = j;
        }
        out += __popcll(bal);
    }
    if (lane == 0) a.deg[row] = out < a.cap ? out : a.cap;
}

// ---- exclusive scan of the per-row degrees -> row_ptr (the two-pass scan of ag_block_dev.h: kScanRows rows per block), then COO fill ----

// Self-edge elision (AgEdgeArgs::self_attrs): a row's self-loop is left out of the lists when the node's attribute pair is class 0 / 1
// (ag_self_class).  Its position in the (ascending) sender row is found here — the workgroup's 256 rows staged through LDS with coalesced
// loads (load_row_slots), each thread then walks its own row — and handed to rowptr_scatter_kernel in self_pos; the scanned degree excludes it.
__device__ __forceinline__ int self_position(const AgEdgeArgs &a, const int32_t *sel, int cap, int *stage, int row0, int nloc, int deg)
{
    const int n = nloc * cap;
    const int32_t *src = sel + (size_t)row0 * cap;
    for (int i0 = threadIdx.x; i0 < n; i0 += kRowSlotStep) {
        int v[4];
        load_row_slots(src, n, i0, v);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + 256 * u < n) stage[i0 + 256 * u] = v[u];
    }
    __syncthreads();
    int pos = -1;
    if ((int)threadIdx.x < nloc) {
        const int r = row0 + threadIdx.x, me = r % a.N;
        const int cls = ag_self_class(a.self_attrs[(size_t)r * 2], a.self_attrs[(size_t)r * 2 + 1]);
        if (cls >= 0)
            for (int k = 0; k < deg; ++k)
                if (stage[threadIdx.x * cap + k] == me) pos = k;
        if (pos > 0xffff) pos = -1;      // (self_info keeps the position in 16 bits; a longer row keeps its self-loop as a real edge)
    }
    return pos;
}
constexpr int kSelfStageMax = 256 * 40;      // ints of LDS for the staged rows; rows longer than 40 slots (top-k + tools) are read from global memory

// shared-state rollout: does any of the 256 rows of this block belong to an active sample?  (NULL `active`: yes)
// `with_prev`: ... or the row in front of the block (rowptr_scatter_kernel: row_ptr[row0] is also the END of that row)
__device__ __forceinline__ bool block_rows_active(const AgEdgeArgs &a, int row0, int rows, bool with_prev = false)
{
    if (!a.active) return true;
    const int last = (row0 + kScanRows <= rows ? row0 + kScanRows : rows) - 1;
    for (int b = (with_prev && row0 > 0 ? row0 - 1 : row0) / a.N; b <= last / a.N; ++b)
        if (a.active[b]) return true;
    return false;
}

__global__ __launch_bounds__(256) void scan_partial_kernel(AgEdgeArgs a, const int32_t *sel, int cap)
{
    __shared__ int stage[kSelfStageMax];
    const int rows = a.B * a.N;
    if (!block_rows_active(a, blockIdx.x * kScanRows, rows)) {      // (uniform) nothing to count: no row is read
        if (threadIdx.x == 0) a.blk_sum[blockIdx.x] = 0;
        return;
    }
    const int r = blockIdx.x * kScanRows + threadIdx.x;
    int d = r < rows ? a.deg[r] : 0;
    if (a.active && r < rows && !a.active[r / a.N]) d = 0;      // (shared-state rollout: skipped sample)
    if (a.self_attrs) {
        const int row0 = blockIdx.x * kScanRows, nloc = rows - row0 < kScanRows ? rows - row0 : kScanRows;
        int pos = -1;
        if (cap * 256 <= kSelfStageMax) pos = self_position(a, sel, cap, stage, row0, nloc, d);
        else if (r < rows && ag_self_class(a.self_attrs[(size_t)r * 2], a.self_attrs[(size_t)r * 2 + 1]) >= 0) {
            const int me = r % a.N;
            for (int k = 0; k < d && k <= 0xffff; ++k)
                if (sel[(size_t)r * cap + k] == me) pos = k;
        }
        if (r < rows) a.self_pos[r] = pos;
        d -= pos >= 0 ? 1 : 0;
    }
    int total;
    block_exclusive_scan(d, &total);
    if (threadIdx.x == 0) a.blk_sum[blockIdx.x] = total;
}

// Second and last pass: a block's base offset is the sum of the partial sums in front of it (every block adds them up itself: nblk values, 1 001 at
// 256 x 1 001 rows — cheaper than a one-workgroup launch that scans them), then row_ptr of its 256 rows and, from LDS, their COO entries: one
// thread per (row, slot), coalesced reads of the per-row sender lists, near-coalesced writes, four slots' loads in flight per thread.
// (r05: was scan_blocks + rowptr + scatter, three launches of 5 + 5 + 11 us at C2.)
__global__ __launch_bounds__(256) void rowptr_scatter_kernel(AgEdgeArgs a, const int32_t *sel, int cap)
{
    __shared__ int s_ptr[kScanRows], s_deg[kScanRows], s_self[kScanRows];
    const int rows = a.B * a.N;
    if (blockIdx.x != gridDim.x - 1 && !block_rows_active(a, blockIdx.x * kScanRows, rows, true)) return;      // (uniform; the last block also writes the totals)
    // rider (ag_rollout, de-duplicated node encoder): the sender column mapped to compact rows for round 0's reduce, written where edge_send is.
    // (The overflow word is read here, with the partial sums, not in front of the loop that uses it: one memory round trip less on the chain.)
    const bool map = a.map_send_c != nullptr;
    const bool ident = map && *a.map_ovf != 0;          // the call overflowed the compact tables: round 0 gathers the full-size table by node id
    const int base = block_offset(a.blk_sum);
    const int r = blockIdx.x * kScanRows + threadIdx.x;
    const bool live = r < rows && !(a.active && !a.active[r / a.N]);      // (rows of a skipped sample: degree 0, nothing of theirs is read — not even self_pos,
    const int d = live ? a.deg[r] : 0;                                    //  which the degree scan's early-exit blocks never wrote)
    // self-edge elision: the row's self-loop (slot ks) is not stored; self_info tells the segment reduce where it belongs
    const int ks = (a.self_attrs && live) ? a.self_pos[r] : -1;
    if (a.self_attrs && r < rows)
        a.self_info[r] = ks >= 0 ? ((ag_self_class(a.self_attrs[(size_t)r * 2], a.self_attrs[(size_t)r * 2 + 1]) << 16) | ks) : -1;
    int total;
    const int off = base + block_exclusive_scan(d - (ks >= 0 ? 1 : 0), &total);
    s_ptr[threadIdx.x] = off;
    s_deg[threadIdx.x] = d;
    s_self[threadIdx.x] = ks >= 0 ? ks : 0x7fffffff;
    if (r < rows) a.row_ptr[r] = off;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) a.row_ptr[rows] = base + total;
    if (a.self_attrs && blockIdx.x == gridDim.x - 1 && (int)threadIdx.x < AG_SELF_ROWS) {      // the class rows' synthetic edges, behind the list
        a.edge_recv[base + total + threadIdx.x] = a.self_class_row0 + (int)threadIdx.x / AG_SELF_REPL;      // (AG_SELF_REPL copies per class)
        a.edge_send[base + total + threadIdx.x] = a.self_class_row0 + (int)threadIdx.x / AG_SELF_REPL;
    }
    __syncthreads();
    const int row0 = blockIdx.x * kScanRows;
    const int nloc = rows - row0 < kScanRows ? rows - row0 : kScanRows;
    const int32_t *src = sel + (size_t)row0 * cap;
    const int n = nloc * cap;
    for (int i0 = threadIdx.x; i0 < n; i0 += kRowSlotStep) {
        int v[4], e[4], sg[4], rw[4];
        load_row_slots(src, n, i0, v);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = i0 + 256 * u;
            e[u] = -1; sg[u] = 0;
            if (idx >= n) continue;
            const int lr = idx / cap, slot = idx - lr * cap;
            if (slot >= s_deg[lr] || slot == s_self[lr]) continue;
            const int row = row0 + lr;
            e[u] = s_ptr[lr] + slot - (slot > s_self[lr] ? 1 : 0);
            sg[u] = (row / a.N) * a.N + v[u];
            a.edge_recv[e[u]] = row;
            a.edge_send[e[u]] = sg[u];
        }
        if (map) {
#pragma unroll
            for (int u = 0; u < 4; ++u) rw[u] = ident ? sg[u] : a.map_node_row[sg[u]];      // (slot 0 of an unused lane: row 0, in range, not stored)
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (e[u] >= 0) a.map_send_c[e[u]] = rw[u];
        }
    }
}

}  // namespace

int ag_launch_build_edges(const AgEdgeArgs &a, hipStream_t s)
{
    const int rows = a.B * a.N;
    int riders = ag_launch_select_edges(a, s);
    const int32_t *sel = a.sel0;
    int cap = a.cap0;
    if (a.connect) {
        if (a.cap <= kToolListMax)             // cap = top-k + the caller's bound on tools per sample
            hipLaunchKernelGGL(finalize_connect_kernel, dim3((a.N + 255) / 256, a.B), dim3(256), (size_t)a.cap * sizeof(int), s, a);
        else
            hipLaunchKernelGGL(finalize_connect_sweep_kernel, dim3((a.N + 3) / 4, a.B), dim3(256), 0, s, a);
        sel = a.sel;
        cap = a.cap;
    }
    const int nblk = (rows + kScanRows - 1) / kScanRows;
    hipLaunchKernelGGL(scan_partial_kernel, dim3(nblk), dim3(256), 0, s, a, sel, cap);
    hipLaunchKernelGGL(rowptr_scatter_kernel, dim3(nblk), dim3(256), 0, s, a, sel, cap);
    if (a.map_send_c) riders |= AG_RIDER_MAP;
    return riders;
}
