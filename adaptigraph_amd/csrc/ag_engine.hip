// ag_engine.hip — one model step on the host: workspace layouts, the call's kernel path and arguments, the kernel sequence; and the entry points
// that are one such step or one edge build (ag_forward, ag_build_edges, dense <-> CSR).  The rollout drivers (ag_drivers.hip) run the same sequence.
#include "ag_block_dev.h"
#include "ag_host.h"

#include <algorithm>

namespace { struct FwdLayout { size_t rows_pad, e_pad, rows_c; }; }

static FwdLayout fwd_layout(int B, int N, int64_t e_cap, bool full_dedup)
{
    FwdLayout L;
    L.rows_pad = align_up((size_t)B * N, AG_ROWS_PER_BLOCK);
    L.e_pad = ag_edge_rows_pad(e_cap);   // whole row tiles of either edge encoder (128 / 256 edges), incl. the class rows of elided self-loops
    // compact rows of the de-duplicated node encoder: AG_DEDUP_REPS shared rows per sample + a bounded private budget (the reference's drivers
    // use 2 rows per sample; until r04 this was sized for "every node private": 4 x B (N + 8) rows, 10.7 GB at the planner's 20 000 x 200)
    L.rows_c = align_up((size_t)B * AG_DEDUP_REPS + std::max<size_t>((size_t)B * N / 16, 1024), AG_ROWS_PER_BLOCK);
    // shared-state rollout: the propagation tables are numbered by compact row, so the per-node fallback of an overflowing call has nowhere to
    // write — a private row for every node instead (the budget cannot overflow)
    if (full_dedup) L.rows_c = align_up((size_t)B * (AG_DEDUP_REPS + (size_t)N), AG_ROWS_PER_BLOCK);
    return L;
}

void carve_forward(Carver &c, AgFwdArgs &a, int B, int N, int64_t e_cap, bool eterm16, bool full_dedup)
{
    const FwdLayout L = fwd_layout(B, N, e_cap, full_dedup);
    const size_t rc = L.rows_c + AG_ROWS_PER_BLOCK;              // + dump rows of the encoder's out-of-range lanes
    a.h = c.take<float>(L.rows_pad * AG_FP);
    a.pn = c.take<float>(L.rows_pad * AG_FP);
    a.hr = c.take<float>(L.rows_pad * AG_FP);
    a.hs = c.take<float>(L.rows_pad * AG_FP);
    a.hr_out = c.take<float>(L.rows_pad * AG_FP);
    a.hs_out = c.take<float>(L.rows_pad * AG_FP);
    a.h0c = c.take<float>(rc * AG_FP);
    a.pnc = c.take<float>(rc * AG_FP);
    a.hrc = c.take<float>(rc * AG_FP);
    a.hsc = c.take<float>(rc * AG_FP);
    a.node_row = c.take<int32_t>(L.rows_pad);
    a.enc_row = c.take<int32_t>(rc);
    a.enc_src = c.take<int32_t>(rc);
    a.send_c = c.take<int32_t>(L.e_pad);
    a.rows_c = (int)L.rows_c;
    a.agg = c.take<float>(L.rows_pad * AG_FP);
    // per-edge table: fp32 rows (640 B), or — sized for a model in precision mode 2 (ag_*_workspace_bytes_for) — q16 rows (320 B) + the
    // weight-stationary kernel's dump rows behind them
    a.eterm = eterm16 ? c.take<float>((L.e_pad + 256) * (AG_FP / 2)) : c.take<float>(L.e_pad * AG_FP);
    a.edge_node_tab = c.take<float>((L.rows_pad + AG_SELF_ROWS) * 16);      // + the class rows of elided self-loops (ag_edge_node_tab_row)
    a.self_class_row0 = (int)L.rows_pad;
    a.tile_ctr = c.take<int>(AG_TILE_CTRS);
    a.enc_count = a.tile_ctr + 1;                                // (zeroed by run_node_encode before the classification fills the work list)
    a.priv_count = a.tile_ctr + 2;
    a.ovf = a.tile_ctr + 3;
    a.shared_rows = B * AG_DEDUP_REPS;
}

void carve_edges(Carver &c, AgEdgeArgs &a)
{
    const size_t rows = (size_t)a.B * a.N;
    a.sel0 = c.take<int32_t>(rows * a.cap0);
    a.sel = a.connect ? c.take<int32_t>(rows * a.cap) : nullptr;
    a.deg = c.take<int32_t>(rows);
    a.flag = c.take<int32_t>(a.B);
    a.blk_sum = c.take<int32_t>(ag_scan_blocks(rows));
    a.grid = c.take<EdgeGrid>((size_t)a.B);
    a.cell_start = c.take<int32_t>((size_t)a.B * (kCellMax + 1));
    a.sorted = c.take<float4>(rows);
}

static void carve_dense(Carver &c, AgDenseArgs &a)
{
    const size_t pairs = (size_t)a.B * a.E, rows = (size_t)a.B * a.N;
    a.key_recv = c.take<int32_t>(pairs);
    a.key_send = c.take<int32_t>(pairs);
    a.cnt = c.take<int32_t>(rows);
    a.blk_sum = c.take<int32_t>(ag_scan_blocks(rows));
}

void edge_caps(int N, int topk, int connect, int max_tools, int *cap0, int *cap)
{
    *cap0 = N < topk ? N : topk;
    *cap = *cap0 + (connect ? max_tools : 0);
}

// A model step's arguments: the call's tensors and sizes, the model's constants, the edge lists the step reads
void bind_forward(const ag_model *m, AgFwdArgs &f, int B, int N, int n_p, int n_inst, const float *state, const float *attrs, const float *action,
                  const float *p_instance, const float *phys, const int32_t *row_ptr, const int32_t *edge_recv, const int32_t *edge_send,
                  float *pred_pos, float *pred_motion)
{
    f.state = state; f.attrs = attrs; f.action = action; f.p_instance = p_instance; f.phys = phys;
    f.row_ptr = row_ptr; f.edge_recv = edge_recv; f.edge_send = edge_send;
    f.pred_pos = pred_pos; f.pred_motion = pred_motion;
    f.B = B; f.N = N; f.n_p = n_p; f.n_inst = n_inst; f.phys_dim = m->cfg.phys_dim;
    f.pstep = m->cfg.pstep; f.clamp = m->cfg.motion_clamp;
}

// The kernels one call runs (AgPath, ag_common.h): the one place where the model's options and the call's shape become kernel choices.
// B, N: the batch of the call (ag_rollout's partition check passes the whole batch, the parts their own); steps: model steps per call; shared:
// the shared-state rollout, which reads the node encoder through its compact rows whatever "node_dedup" says (its carving leaves no overflow
// possible).  No model: fp32 tables (the workspace queries of any model).
AgPath resolve_path(const ag_model *m, int B, int N, int n_inst, int steps, bool shared)
{
    AgPath p{};
    if (!m) return p;
    p.b3 = m->precision >= 1;
    p.q16 = m->precision == 2;
    if (!p.b3) p.edge = AG_EDGE_F32;
    else if (!p.q16 || m->edge_products != 2 || !m->h2_ok) p.edge = AG_EDGE_B3;      // (edge-stack weights beyond fp16's range: split-bf16 edge stack)
    else if (m->edge_ws && n_inst <= 1 && (long long)B * N * 4 < 0x7fffffffLL) p.edge = AG_EDGE_H3_WS;
    else p.edge = AG_EDGE_H3;
    const bool fused = m->fuse_agg == 2 && p.q16;      // the fused reduce needs the q16 table: the other modes keep the launch
    const bool agg_q16 = m->agg_q16 && p.q16;          // the q16 reduce writes `agg` as q16 rows, every split-bf16 node_update reads them
    p.mid = {p.b3 && m->node_ws && !fused, fused, agg_q16, p.q16};
    p.last = {false, fused, agg_q16, false};
    p.agg_launch = !fused;
    // (below 32 768 node-rows x steps its two extra small launches cost more than the shorter kernels save: 0.126 vs 0.115 ms, 100 particles)
    p.dedup = shared || (m->node_dedup && (long long)B * (N + AG_DEDUP_REPS) < 0x7fffff00LL &&
                         (m->node_dedup >= 2 || (long long)B * N * (steps > 0 ? steps : 1) >= 32768));
    return p;
}

void setup_args(ag_model *m, AgFwdArgs &a, const AgPath &p, int max_blocks)      // the call's path -> its kernel arguments
{
    a.edge_counter = m->profiling ? m->edge_counter : nullptr;
    a.precision = p.b3 ? AG_PREC_B3 : AG_PREC_F32;
    a.eterm_half = p.q16;
    a.max_blocks = max_blocks;     // per call, not per model: a model shared by two callers is not mutated
    a.dedup = p.dedup;
    a.hr_row = nullptr; a.pn_rows = nullptr; a.h_rows = nullptr; a.hr_full = nullptr; a.hs_full = nullptr;
    if (!a.dedup) a.ovf = nullptr;
    // workgroups of the weight-stationary edge encoder (one per CU): a launch that shares the chip with the other rollout streams takes 1.5x its
    // share of the CUs, capped at all of them (two-stream rollout, C2, r04: 128 CUs -> 127.8 k, 160 -> 133.3 k, 192 -> 134.2 k, 224 -> 132.1 k,
    // 256 -> 132.0 k graph-steps/s)
    const int full = m->max_blocks / AG_MLP_WG_PER_CU, share = max_blocks / AG_MLP_WG_PER_CU * 3 / 2;
    a.ws_blocks = share < full ? (share > 0 ? share : 1) : (full > 0 ? full : 1);
    a.status = m->status;
}

// particle_encoder + hoisted Pn + the first round's Hr / Hs.  Their inputs (attrs, phys, action) do not change during a rollout
// (forward_dynamics.py:177-180: graph["action"] is constant across the inner steps), so with node de-duplication — whose compact
// tables no later kernel overwrites — ag_rollout runs this ONCE per call instead of once per model step.
void run_node_encode(ag_model *m, AgFwdArgs &a, hipStream_t s)
{
    if (a.dedup) ag_launch_zero_words(a.enc_count, 3, s);      // enc_count, priv_count, ovf (a kernel: memset nodes of a captured graph were not replayed reliably)
    { Timed t(m, AG_K_NODE_ENCODE, s); ag_launch_node_encode(m->w, a, s); }
}

// De-duplicated calls only: the per-node encoder behind a test of the overflow flag (a handful of workgroups that read one word and return,
// unless this call's inputs did not fit the compact tables).  Every model step: the full-size tables it fills are overwritten by the rounds.
void run_node_encode_fallback(ag_model *m, AgFwdArgs &a, hipStream_t s)
{
    if (a.dedup) ag_launch_node_encode_fallback(m->w, a, s);
}

void run_edge_encode(ag_model *m, AgFwdArgs &a, const AgPath &path, hipStream_t s)
{
    // row-tile claim counter of the STREAMING edge encoders; the weight-stationary kernel (default mode) deals its blocks statically: no fill launch
    const bool ws = path.edge == AG_EDGE_H3_WS;
    if (a.tile_ctr && !ws) ag_launch_zero_words(a.tile_ctr, 1, s);
    { Timed t(m, AG_K_EDGE_ENCODE, s); ag_launch_edge_encode(m->w, a, path, s); if (path.dedup && !ws && !a.remap_done) ag_launch_send_remap(a, s); }      // (ws: mapped by the node-table launch)
}

void run_propagate(ag_model *m, AgFwdArgs &a, const AgPath &path, hipStream_t s)
{
    for (int p = 0; p < a.pstep; ++p) {
        AgFwdArgs r = a;                 // this round's view of the tables
        if (a.dedup) {
            r.pn_rows = a.pnc;           // Pn: compact rows in every round
            if (p == 0) {                // round 0 reads the encoder's compact rows: Hr through node_row, Hs through send_c, h from h0c
                r.hr_full = a.hr;        // (or, when the call overflowed the compact tables, the per-node encoder's full-size ones)
                r.hs_full = a.hs;
                r.hr = a.hrc;
                r.hs = a.hsc;
                r.hr_row = a.node_row;
                r.edge_send = a.send_c;
                r.h_rows = a.h0c;
            }
        }
        // The per-edge table (0.8 GB at C2) is streamed once per round and is larger than the 256 MB memory-side cache, which after a pass
        // holds the END of what that pass touched: alternate the direction — the edge encoder writes the table front to back, so round 0
        // starts at the back, round 1 at the front, ... — and every pass begins where the last one ended.  Measured: segment reduce 0.2472 ->
        // 0.2452 ms per launch at C2 (-0.8 %: the cache holds a quarter of one pass, and the reduce is not latency-bound enough to care); same bits.
        // (With the non-temporal hints on the table's loads, ag_common.h, the direction no longer matters: never / always / alternating within 0.5 %.)
        r.agg_reverse = (p & 1) == 0 ? 1 : 0;
        const int last = p == a.pstep - 1;
        const AgNodeUpdate &v = last ? path.last : path.mid;
        r.hs_q16 = (path.q16 && p > 0) ? 1 : 0;                         // rounds after the first gather the q16 rows the previous node_update wrote
        r.hs_out_q16 = v.hs_q16;
        r.agg_q16 = v.agg_q16;
        if (path.agg_launch) { Timed t(m, AG_K_AGGREGATE, s); ag_launch_aggregate(r, path, last, s); }
        { Timed t(m, AG_K_NODE_UPDATE, s); ag_launch_node_update(m->w, r, path, last, s); }
        std::swap(a.hr, a.hr_out);
        std::swap(a.hs, a.hs_out);
    }
}

extern "C" {

int64_t ag_edge_capacity(int B, int N, int topk, int connect_tools_all, int max_tools)
{
    int cap0, cap;
    edge_caps(N, topk, connect_tools_all, max_tools, &cap0, &cap);
    return (int64_t)B * N * (connect_tools_all ? cap : cap0);
}

size_t ag_edges_workspace_bytes(int B, int N, int topk, int connect_tools_all, int max_tools)
{
    AgEdgeArgs a{};
    a.B = B; a.N = N; a.connect = connect_tools_all;
    edge_caps(N, topk, connect_tools_all, max_tools, &a.cap0, &a.cap);
    Carver c(nullptr, 0);
    carve_edges(c, a);
    return align_up(c.off, 256);
}

int ag_build_edges(const float *pos, const uint8_t *mask, const uint8_t *tool_mask, const float *thr_sq, int topk,
                   int connect_tools_all, int variant, int B, int N, int max_tools, int32_t *row_ptr,
                   int32_t *edge_recv, int32_t *edge_send, int64_t e_cap, void *workspace, size_t workspace_bytes,
                   ag_stream_t stream)
{
    if (!pos || !mask || !tool_mask || !thr_sq || !row_ptr || !edge_recv || !edge_send || !workspace)
        return ag_fail(AG_ERR_ARG, "ag_build_edges: null argument");
    if (B < 1 || N < 1 || topk < 1 || topk > 64) return ag_fail(AG_ERR_ARG, "ag_build_edges: B=%d N=%d topk=%d (1..64)", B, N, topk);
    if (variant != AG_VARIANT_SINGLE && variant != AG_VARIANT_BATCH) return ag_fail(AG_ERR_ARG, "bad variant %d", variant);
    if ((int64_t)B * N >= (1ll << 31) / 64) return ag_fail(AG_ERR_ARG, "B*N too large for int32 edge offsets");
    if (e_cap < ag_edge_capacity(B, N, topk, connect_tools_all, max_tools))
        return ag_fail(AG_ERR_ARG, "ag_build_edges: e_cap %lld < ag_edge_capacity()", (long long)e_cap);
    AgEdgeArgs a{};
    a.pos = pos; a.mask = mask; a.tool = tool_mask; a.thr_sq = thr_sq;
    a.topk = topk; a.connect = connect_tools_all ? 1 : 0; a.variant = variant; a.B = B; a.N = N; a.max_tools = max_tools;
    edge_caps(N, topk, a.connect, max_tools, &a.cap0, &a.cap);
    a.row_ptr = row_ptr; a.edge_recv = edge_recv; a.edge_send = edge_send;
    a.pos_stride = (size_t)N * 3;
    Carver c(workspace, workspace_bytes);
    carve_edges(c, a);
    if (!c.ok()) return ag_fail(AG_ERR_WS, "ag_build_edges: workspace %zu < %zu bytes", workspace_bytes, c.off);
    ag_launch_build_edges(a, static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

size_t ag_dense_edges_workspace_bytes(int B, int E, int N)
{
    if (B < 1 || E < 1 || N < 1) return 0;
    AgDenseArgs a{};
    a.B = B; a.E = E; a.N = N;
    Carver c(nullptr, 0);
    carve_dense(c, a);
    return align_up(c.off, 256);
}

int ag_edges_from_dense(const float *Rr, const float *Rs, int B, int E, int N, int32_t *row_ptr, int32_t *edge_recv, int32_t *edge_send,
                        void *workspace, size_t workspace_bytes, ag_stream_t stream)
{
    if (!Rr || !Rs || !row_ptr || !edge_recv || !edge_send || !workspace) return ag_fail(AG_ERR_ARG, "ag_edges_from_dense: null argument");
    if (B < 1 || E < 1 || N < 1) return ag_fail(AG_ERR_ARG, "ag_edges_from_dense: bad sizes B=%d E=%d N=%d", B, E, N);
    if ((int64_t)B * N >= (1ll << 31) - 1 || (int64_t)B * E >= (1ll << 31) - 1)
        return ag_fail(AG_ERR_ARG, "ag_edges_from_dense: B*N = %lld or B*E = %lld too large for int32 ids", (long long)B * N, (long long)B * E);
    AgDenseArgs a{};
    a.Rr = Rr; a.Rs = Rs; a.B = B; a.E = E; a.N = N;
    a.row_ptr = row_ptr; a.edge_recv = edge_recv; a.edge_send = edge_send;
    Carver c(workspace, workspace_bytes);
    carve_dense(c, a);
    if (!c.ok()) return ag_fail(AG_ERR_WS, "ag_edges_from_dense: workspace %zu < %zu bytes", workspace_bytes, c.off);
    ag_launch_edges_from_dense(a, static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_edges_to_dense(const int32_t *row_ptr, const int32_t *edge_recv, const int32_t *edge_send, int B, int N, int E_out, float *Rr, float *Rs,
                      int32_t *overflow, ag_stream_t stream)
{
    if (!row_ptr || !edge_recv || !edge_send || !Rr || !Rs || !overflow) return ag_fail(AG_ERR_ARG, "ag_edges_to_dense: null argument");
    if (B < 1 || N < 1 || E_out < 1) return ag_fail(AG_ERR_ARG, "ag_edges_to_dense: bad sizes B=%d N=%d E_out=%d", B, N, E_out);
    if ((int64_t)B * N >= (1ll << 31) - 1 || (int64_t)B * E_out >= (1ll << 31) - 1)
        return ag_fail(AG_ERR_ARG, "ag_edges_to_dense: B*N = %lld or B*E_out = %lld too large", (long long)B * N, (long long)B * E_out);
    ag_launch_edges_to_dense(row_ptr, edge_recv, edge_send, B, N, E_out, Rr, Rs, overflow, static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

size_t ag_forward_workspace_bytes(int B, int N, int64_t e_cap) { return ag_forward_workspace_bytes_for(nullptr, B, N, e_cap); }

size_t ag_forward_workspace_bytes_for(const ag_model *m, int B, int N, int64_t e_cap)
{
    AgFwdArgs a{};
    Carver c(nullptr, 0);
    carve_forward(c, a, B, N, e_cap, resolve_path(m, B, N, 0).q16);
    return align_up(c.off, 256);
}

int ag_forward(ag_model *m, const float *state, const float *attrs, const float *action, const float *p_instance,
               int n_instance, const float *phys, const int32_t *row_ptr, const int32_t *edge_recv,
               const int32_t *edge_send, int64_t e_cap, int B, int N, int n_p, float *pred_pos, float *pred_motion,
               void *workspace, size_t workspace_bytes, ag_stream_t stream)
{
    if (!m || !state || !attrs || !action || (!p_instance && n_instance > 0) || !row_ptr || !edge_recv || !edge_send || !pred_pos ||
        !pred_motion || !workspace)
        return ag_fail(AG_ERR_ARG, "ag_forward: null argument");
    if (m->cfg.phys_dim > 0 && !phys) return ag_fail(AG_ERR_ARG, "ag_forward: phys is null");
    if (B < 1 || N < 1 || n_p < 0 || n_p > N || n_instance < 0 || e_cap < 0 || e_cap > 0x7fffffff)
        return ag_fail(AG_ERR_ARG, "ag_forward: bad sizes B=%d N=%d n_p=%d e_cap=%lld", B, N, n_p, (long long)e_cap);
    AgFwdArgs a{};
    bind_forward(m, a, B, N, n_p, n_instance, state, attrs, action, p_instance, phys, row_ptr, edge_recv, edge_send, pred_pos, pred_motion);
    a.e_cap = (int)e_cap;
    const AgPath path = resolve_path(m, B, N, n_instance);
    Carver c(workspace, workspace_bytes);
    carve_forward(c, a, B, N, e_cap, path.q16);
    if (!c.ok()) return ag_fail(AG_ERR_WS, "ag_forward: workspace %zu < %zu bytes", workspace_bytes, c.off);
    hipStream_t s = static_cast<hipStream_t>(stream);
    setup_args(m, a, path, m->max_blocks);
    run_node_encode(m, a, s);
    run_node_encode_fallback(m, a, s);
    run_edge_encode(m, a, path, s);
    run_propagate(m, a, path, s);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

}  // extern "C"
