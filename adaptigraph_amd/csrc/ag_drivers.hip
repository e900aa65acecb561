// ag_drivers.hip — the rollout drivers of the C ABI: ag_rollout (round-robin or CU-partitioned scheduler), its shared-state form, ag_rollout_ragged
// (either form on one stream, every model step sized for the samples still running) and ag_rollout_scripted; each carves its lanes, binds a step's
// arguments once and runs the engine's kernel sequence (ag_engine.hip) per model step.
#include "ag_block_dev.h"
#include "ag_host.h"

static_assert(AG_ORDER_STEPS == AG_RAGGED_MAX_STEPS && AG_STATUS_ORDER_BIT == AG_STATUS_ORDER, "the kernels' constants are the header's");

namespace {

struct Lane {   // what a rollout driver keeps per batch part [b0, b0 + B) (the shared-state and the scripted rollout have one part; `st`: ag_rollout's state step)
    AgFwdArgs f{};
    AgEdgeArgs e{};
    AgStepArgs st{};
    AgPath path{};
    float *state = nullptr, *pred_pos = nullptr, *pred_motion = nullptr;
    hipStream_t s = nullptr;
    int b0 = 0, B = 0;
};

// ag_rollout_ragged: the samples are in non-increasing order of `repeat`, so the samples that still run at model step ai are the first active[ai - 1]
// (a HOST array) and every launch of that step is sized for them; table bases and row numbers stay those of the whole batch.  A sample records into row
// out_index[b] (device array; NULL: b) of out_seq and state_final
struct Ragged {
    const int32_t *active, *out_index;
};

// One step's buffers of a lane of B samples (Params: ag_rollout_params or ag_scripted_params): predictions of pred_n slots per sample, the lists the edge
// builder writes and the forward reads (`self_lists`: + the class edges of self-edge elision and its two per-node lists), its scratch, the forward's tables
template <class Params>
void carve_step(Carver &c, Lane &l, const Params *p, int B, int pred_n, bool self_lists, bool eterm16, bool full_dedup = false)
{
    const int64_t e_cap = ag_edge_capacity(B, p->N, p->topk, p->connect_tools_all, p->max_tools);
    const size_t rows = (size_t)B * p->N, ecoo = (size_t)e_cap + 1 + (self_lists ? AG_SELF_ROWS : 0);
    AgEdgeArgs &e = l.e;
    l.pred_pos = c.take<float>((size_t)B * pred_n * 3 + 4);
    l.pred_motion = c.take<float>((size_t)B * pred_n * 3 + 4);
    e.row_ptr = c.take<int32_t>(rows + 1);
    e.edge_recv = c.take<int32_t>(ecoo);
    e.edge_send = c.take<int32_t>(ecoo);
    if (self_lists) {
        e.self_info = c.take<int32_t>(rows);
        e.self_pos = c.take<int32_t>(rows);
    }
    e.B = B; e.N = p->N; e.connect = p->connect_tools_all ? 1 : 0;
    edge_caps(p->N, p->topk, e.connect, p->max_tools, &e.cap0, &e.cap);
    carve_edges(c, e);
    carve_forward(c, l.f, B, p->N, e_cap, eterm16, full_dedup);
    l.f.e_cap = (int)e_cap;
    l.B = B;
}

// A rollout lane's edge build: edges on the current frame = the last of the lane's n_his history frames (forward_dynamics.py:125 / :171)
template <class Params>
void bind_edges(Lane &l, const Params *p, int variant, int n_his, const uint8_t *mask, const uint8_t *tool_mask, const float *thr_sq)
{
    const size_t plane = (size_t)p->N * 3;
    AgEdgeArgs &e = l.e;
    e.mask = mask; e.tool = tool_mask; e.thr_sq = thr_sq; e.topk = p->topk; e.variant = variant; e.max_tools = p->max_tools;
    e.pos = l.state + (size_t)(n_his - 1) * plane; e.pos_stride = (size_t)n_his * plane;
}

// Rider of the edge builder's launches (AgEdgeArgs): the per-node input rows of the weight-stationary edge encoder.  After setup_args (f.status).
void wire_tab_rider(Lane &l)
{
    if (l.path.edge != AG_EDGE_H3_WS) return;
    AgEdgeArgs &e = l.e;
    const AgFwdArgs &f = l.f;
    e.tab_state = f.state; e.tab_attrs = f.attrs; e.tab_pinst = f.p_instance; e.tab_out = f.edge_node_tab;
    e.tab_n_inst = f.n_inst; e.tab_n_p = f.n_p; e.tab_status = f.status;
}

}  // namespace

extern "C" {

// The batch is rolled out as up to AG_MAX_PARTS independent parts on separate streams: graphs never interact,
// and co-running kernel streams de-phase the memory-bound stages (segment reduce, edge-feature gathers, edge
// build) of one part against the MFMA-bound stages of another — each part's persistent kernels take an equal
// share of the resident-workgroup slots.
// "rollout_streams" 0: two streams hide launch gaps and overlap the MFMA-bound edge encoder of one half with the HBM-bound kernels of the other, but the halves
// also evict each other's tables between a reduce and its node_update.  Measured with the r05 kernels (profiles/r05_nt_hints.txt, ab_streams): one stream wins where
// the edge encoder is a third of the step (rope, top-k 10: +1-2 % at 256 graphs, +4 % at 1 024; cloth, top-k 5: even), two where it is 40 % (granular, top-k 20: +1.7 %).
static int rollout_want(const ag_model *m, const ag_rollout_params *p) { return m && m->split > 0 ? m->split : (p->topk >= 16 ? 2 : 1); }
static int rollout_parts(int B, int want)
{
    int parts = want < 1 ? 1 : (want > AG_MAX_PARTS ? AG_MAX_PARTS : want);
    while (parts > 1 && B / parts < 8) --parts;
    return parts;
}
static void part_range(int B, int parts, int k, int *b0, int *nb)
{
    const int per = (B + parts - 1) / parts;
    *b0 = k * per < B ? k * per : B;
    *nb = (*b0 + per <= B) ? per : B - *b0;
}
// The batch parts of an ag_rollout call and of its workspace query: each part's samples, its kernels and its layout, one part behind the other
static void carve_parts(Carver &c, const ag_model *m, const ag_rollout_params *p, int parts, Lane *lane)
{
    for (int k = 0; k < parts; ++k) {
        Lane &l = lane[k];
        int B;
        part_range(p->B, parts, k, &l.b0, &B);
        l.path = resolve_path(m, B, p->N, p->n_instance, p->n_steps);
        l.state = c.take<float>((size_t)B * p->N * AG_NHIS * 3);
        carve_step(c, l, p, B, p->n_p, true, l.path.q16);
    }
}

struct RolloutIn {   // the ten input arrays of an ag_rollout call, whole batch
    const float *state0, *delta, *attrs, *p_instance, *phys;
    const uint8_t *mask, *tool_mask, *obj_mask;
    const float *thr_sq;
    const int32_t *repeat;
};

// A part's arguments from its carving, its stream and its slice of the batch (nothing is enqueued here).  `partitioned`: the CU-partitioned scheduler
static void bind_part(ag_model *m, const ag_rollout_params *p, Lane &l, const RolloutIn &in, float *out_seq, bool partitioned, int part_blocks)
{
    const int H = m->cfg.n_his, N = p->N, n_p = p->n_p, Pd = m->cfg.phys_dim;
    const size_t plane = (size_t)N * 3, b0 = (size_t)l.b0;
    AgEdgeArgs &e = l.e;
    AgFwdArgs &f = l.f;
    bind_edges(l, p, AG_VARIANT_BATCH, H, in.mask + b0 * N, in.tool_mask + b0 * N, in.thr_sq + b0);
    bind_forward(m, f, l.B, N, n_p, p->n_instance, l.state, in.attrs + b0 * N * 2, in.delta + b0 * plane, in.p_instance + b0 * n_p * p->n_instance,
                 in.phys ? in.phys + b0 * Pd : nullptr, e.row_ptr, e.edge_recv, e.edge_send, l.pred_pos, l.pred_motion);
    if (m->self_edges) {      // self-edge elision: the builder leaves class-0 / class-1 self-loops out of the lists, the encoder adds one row per class
        e.self_attrs = f.attrs; e.self_class_row0 = f.self_class_row0;
        f.self_info = e.self_info; f.self_rows = AG_SELF_ROWS;
    }
    if (partitioned) {
        setup_args(m, f, l.path, AG_MLP_WG_PER_CU * (m->n_cus - m->cu_split));   // persistent node kernels: the HBM partition's CUs
        f.ws_blocks = m->cu_split;                                                // edge encoder: one workgroup per CU of the MFMA partition
    } else {
        setup_args(m, f, l.path, part_blocks);
        // riders of the edge builder's launches (one 15 us launch per model step less each): the edge encoder's per-node input rows and, for a
        // de-duplicated node encoder, the sender column mapped to compact rows
        wire_tab_rider(l);
        if (f.dedup) { e.map_node_row = f.node_row; e.map_ovf = f.ovf; e.map_send_c = f.send_c; }
    }
    AgStepArgs &st = l.st;
    st.state = l.state; st.delta = in.delta + b0 * plane; st.pred_pos = l.pred_pos;
    st.obj_mask = in.obj_mask ? in.obj_mask + b0 * n_p : nullptr; st.repeat = in.repeat + b0;
    st.out_seq = out_seq + b0 * n_p * 3; st.B = l.B; st.N = N; st.n_p = n_p; st.H = H;
    st.height_mode = p->height_mode; st.raise = p->gripper_raise;
}

// The two CU-masked streams of the partitioned rollout (created once per cu_split value).  Mask bit b is CU slot b / 8 of XCD b % 8
// (tools/ubench/cu_mask_map.hip -> profiles/r05_cu_mask_map.txt), so bits [0, X) and [X, n_cus) with X a multiple of 8 are disjoint sets of
// X / 8 and (n_cus - X) / 8 CUs of EVERY XCD: both partitions keep all eight L2s and all memory channels.
static int ensure_partition(ag_model *m)
{
    if (m->mfma_stream && m->hbm_stream && m->part_cus == m->cu_split) return AG_OK;
    if (m->mfma_stream) { (void)hipStreamSynchronize(m->mfma_stream); (void)hipStreamDestroy(m->mfma_stream); m->mfma_stream = nullptr; }
    if (m->hbm_stream) { (void)hipStreamSynchronize(m->hbm_stream); (void)hipStreamDestroy(m->hbm_stream); m->hbm_stream = nullptr; }
    const int words = (m->n_cus + 31) / 32;
    std::vector<uint32_t> lo(words, 0u), hi(words, 0u);
    for (int b = 0; b < m->n_cus; ++b) (b < m->cu_split ? lo : hi)[b >> 5] |= 1u << (b & 31);
    AG_HIP(hipExtStreamCreateWithCUMask(&m->mfma_stream, (uint32_t)words, lo.data()));
    AG_HIP(hipExtStreamCreateWithCUMask(&m->hbm_stream, (uint32_t)words, hi.data()));
    for (int k = 0; k < 4; ++k) {
        if (!m->ev_ready[k]) AG_HIP(hipEventCreateWithFlags(&m->ev_ready[k], hipEventDisableTiming));
        if (!m->ev_enc[k]) AG_HIP(hipEventCreateWithFlags(&m->ev_enc[k], hipEventDisableTiming));
    }
    if (!m->ev_join_mfma) AG_HIP(hipEventCreateWithFlags(&m->ev_join_mfma, hipEventDisableTiming));
    m->part_cus = m->cu_split;
    return AG_OK;
}

// ---- shared-state rollout (ag_shared.hip): one stream, the batch as ONE part behind the base sample -------------------------------------------------
static bool shared_applicable(const ag_model *m, const ag_rollout_params *p)
{
    if (!m || !p || !m->shared_state || p->B < 2 || p->n_steps < 1) return false;
    if (m->cfg.pstep > 3) return false;      // (ag_launch_shared_compact marks the touched rows plus two hops: exact for up to three propagation rounds)
    if (m->fuse_agg != 0 || m->cu_split != 0) return false;      // (the fused reduce and the CU-partitioned pipeline keep the plain path)
    if ((long long)(p->B + 1) * (p->N + AG_DEDUP_REPS) >= 0x7fffff00LL) return false;
    if (ag_edge_capacity(p->B + 1, p->N, p->topk, p->connect_tools_all, p->max_tools) >= 0x7fffff00LL) return false;
    return true;
}

static void carve_shared(Carver &c, const ag_model *m, const ag_rollout_params *p, AgSharedArgs &s, Lane &l, bool eterm16)
{
    const int B1 = p->B + 1, N = p->N, n_p = p->n_p, H = AG_NHIS, Pd = m->cfg.phys_dim, I = p->n_instance;
    const int64_t e_cap = ag_edge_capacity(B1, N, p->topk, p->connect_tools_all, p->max_tools);
    const size_t rows = (size_t)B1 * N, ecoo = (size_t)e_cap + 1 + AG_SELF_ROWS;
    l.state = s.s_state = c.take<float>(rows * H * 3);
    s.s_delta = c.take<float>(rows * 3);
    s.s_attrs = c.take<float>(rows * 2);
    s.s_pinst = c.take<float>((size_t)B1 * n_p * (I > 0 ? I : 1));
    s.s_phys = c.take<float>((size_t)B1 * (Pd > 0 ? Pd : 1));
    s.s_thr = c.take<float>(B1);
    s.s_mask = c.take<uint8_t>(rows);
    s.s_tool = c.take<uint8_t>(rows);
    s.s_obj_mask = c.take<uint8_t>((size_t)B1 * n_p);
    s.s_repeat = c.take<int32_t>(B1);
    s.dirty = c.take<uint8_t>(rows);
    s.sel_a = c.take<uint8_t>(rows);
    s.sel_b = c.take<uint8_t>(rows);
    s.sample_dirty = c.take<int32_t>(B1);
    s.active = c.take<int32_t>(B1);
    s.cmap = c.take<int32_t>(rows);
    s.orig = c.take<int32_t>(rows);
    s.row_ptr_c = c.take<int32_t>(rows + 1);
    s.self_info_c = c.take<int32_t>(rows);
    s.node_row_c = c.take<int32_t>(rows + AG_ROWS_PER_BLOCK);
    s.recv_o = c.take<int32_t>(ecoo);
    s.send_o = c.take<int32_t>(ecoo);
    s.send_r0 = c.take<int32_t>(ecoo);
    s.send_cm = c.take<int32_t>(ecoo);
    s.blk_cnt = c.take<int32_t>(ag_scan_blocks(rows));
    s.blk_deg = c.take<int32_t>(ag_scan_blocks(rows));
    s.n_rows = c.take<int>(4);
    s.n_edges = s.n_rows + 1;
    carve_step(c, l, p, B1, N, true, eterm16, true);
}

static int rollout_shared(ag_model *m, const ag_rollout_params *p, const float *state0, const float *delta, const float *attrs,
                          const float *p_instance, const float *phys, const uint8_t *mask, const uint8_t *tool_mask, const uint8_t *obj_mask,
                          const float *thr_sq, const int32_t *repeat, float *out_seq, float *state_final, void *workspace, size_t workspace_bytes,
                          hipStream_t s, const Ragged *rg = nullptr)
{
    Lane l;
    l.path = resolve_path(m, p->B + 1, p->N, p->n_instance, p->n_steps, true);
    Carver c(workspace, workspace_bytes);
    AgSharedArgs sh{};
    carve_shared(c, m, p, sh, l, l.path.q16);
    if (!c.ok()) return ag_fail(AG_ERR_WS, "ag_rollout (shared state): workspace %zu < %zu bytes", workspace_bytes, c.off);
    AgFwdArgs &f = l.f;
    AgEdgeArgs &e = l.e;
    const int B1 = p->B + 1, N = p->N, n_p = p->n_p, H = m->cfg.n_his, Pd = m->cfg.phys_dim;
    const size_t plane = (size_t)N * 3;
    sh.B1 = B1; sh.N = N; sh.n_p = n_p; sh.n_inst = p->n_instance; sh.phys_dim = Pd; sh.H = H;
    sh.state0 = state0; sh.delta = delta; sh.attrs = attrs; sh.p_instance = p_instance; sh.phys = phys; sh.thr_sq = thr_sq;
    sh.mask = mask; sh.tool = tool_mask; sh.obj_mask = obj_mask; sh.repeat = repeat;
    sh.max_tools = p->max_tools;
    ag_launch_shared_stage(sh, s);      // internal sample 0 = the base (caller sample 0 without its tools), 1 .. B = the caller's samples; first dirty flags
    bind_edges(l, p, AG_VARIANT_BATCH, H, sh.s_mask, sh.s_tool, sh.s_thr);
    e.active = sh.active;
    bind_forward(m, f, B1, N, n_p, p->n_instance, sh.s_state, sh.s_attrs, sh.s_delta, sh.s_pinst, Pd > 0 ? sh.s_phys : nullptr, e.row_ptr, e.edge_recv,
                 e.edge_send, l.pred_pos, l.pred_motion);
    setup_args(m, f, l.path, m->max_blocks);
    const int self_rows = m->self_edges ? AG_SELF_ROWS : 0;
    if (self_rows) { e.self_attrs = f.attrs; e.self_class_row0 = f.self_class_row0; }
    wire_tab_rider(l);                  // (the input rows of all B1 N nodes: the compact edges name their endpoints as nodes)
    run_node_encode(m, f, s);           // classification + compact encoder, once per call
    sh.row_ptr = e.row_ptr; sh.edge_send = e.edge_send; sh.self_info = self_rows ? e.self_info : nullptr; sh.node_row = f.node_row;
    sh.self_rows = self_rows; sh.self_class_row0 = f.self_class_row0;
    AgFwdArgs fE = f, fP = f;           // the edge encoder's and the propagation rounds' views of the compact graph
    fE.edge_recv = sh.recv_o; fE.edge_send = sh.send_o; fE.e_count_dev = sh.n_edges; fE.remap_done = 1; fE.self_rows = self_rows;
    fP.row_ptr = sh.row_ptr_c; fP.edge_send = sh.send_cm; fP.send_c = sh.send_r0; fP.node_row = sh.node_row_c;
    fP.self_info = self_rows ? sh.self_info_c : nullptr; fP.self_rows = self_rows;
    fP.n_rows_dev = sh.n_rows; fP.e_count_dev = sh.n_edges; fP.row_orig = sh.orig;
    AgStepArgs &st = l.st;
    st.state = sh.s_state; st.delta = sh.s_delta; st.pred_pos = l.pred_pos; st.obj_mask = obj_mask ? sh.s_obj_mask : nullptr;
    st.repeat = sh.s_repeat; st.out_seq = out_seq; st.B = B1; st.N = N; st.n_p = n_p; st.H = H;
    st.height_mode = p->height_mode; st.raise = p->gripper_raise; st.cmap = sh.cmap; st.dirty = sh.dirty; st.sample_dirty = sh.sample_dirty;
    if (rg) { st.out_index = rg->out_index; st.out_rows = p->B; st.status = m->status; }
    for (int ai = 1; ai <= p->n_steps; ++ai) {
        if (rg) {      // the base and the samples still running: internal samples [0, 1 + active)
            if (rg->active[ai - 1] < 1) break;
            sh.B1 = e.B = fE.B = fP.B = st.B = 1 + rg->active[ai - 1];
        }
        int riders;
        { Timed tm(m, AG_K_EDGES, s); ag_launch_shared_active(sh, s); riders = ag_launch_build_edges(e, s); ag_launch_shared_compact(sh, s); }
        fE.tab_done = (riders & AG_RIDER_TAB) != 0;
        run_edge_encode(m, fE, l.path, s);
        run_propagate(m, fP, l.path, s);
        st.step = ai;
        { Timed tm(m, AG_K_ROLLOUT_STEP, s); ag_launch_rollout_step(st, s); }
    }
    if (rg) ag_launch_ragged_finish(sh.s_state + (size_t)H * plane, repeat, rg->out_index, state_final, p->B, H, N, m->status, s);
    else if (state_final)
        AG_HIP(hipMemcpyAsync(state_final, sh.s_state + (size_t)H * plane, (size_t)p->B * H * plane * sizeof(float), hipMemcpyDeviceToDevice, s));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

size_t ag_rollout_workspace_bytes(const ag_rollout_params *p) { return ag_rollout_workspace_bytes_for(nullptr, p); }
int ag_rollout_streams_for(const ag_model *m, const ag_rollout_params *p) { return m && p ? (shared_applicable(m, p) ? 1 : rollout_parts(p->B, rollout_want(m, p))) : 0; }

size_t ag_rollout_workspace_bytes_for(const ag_model *m, const ag_rollout_params *p)
{
    if (!p) return 0;
    // ag_rollout carves one layout per batch part and the number of parts is a model option ("rollout_streams", 1..4) the
    // caller may change between this query and the call: size for the largest of the four possible carvings, exactly.
    size_t need = 0;
    Lane lane[AG_MAX_PARTS];
    for (int want = 1; want <= AG_MAX_PARTS; ++want) {
        Carver c(nullptr, 0);
        carve_parts(c, m, p, rollout_parts(p->B, want), lane);
        need = c.off > need ? c.off : need;
    }
    if (shared_applicable(m, p)) {      // (an option the caller may switch off again before the call: the larger of the two layouts)
        Carver c(nullptr, 0);
        AgSharedArgs sh{};
        carve_shared(c, m, p, sh, lane[0], resolve_path(m, p->B, p->N, p->n_instance).q16);
        need = c.off > need ? c.off : need;
    }
    return align_up(need, 256);
}

struct Join {   // RAII: whichever way ag_rollout returns, the streams it forked off the caller's stream join it again (success: join(), for its code)
    hipStream_t caller;
    int n = 0;
    hipEvent_t event[AG_MAX_PARTS];
    hipStream_t forked[AG_MAX_PARTS];
    hipError_t fork(hipStream_t stream, hipEvent_t ev_fork, hipEvent_t ev_join)     // `stream` waits on the fork event; once it does, it is joined
    {
        hipError_t rc = hipStreamWaitEvent(stream, ev_fork, 0);
        if (rc == hipSuccess) { event[n] = ev_join; forked[n++] = stream; }
        return rc;
    }
    hipError_t join()
    {
        hipError_t rc = hipSuccess;
        for (int k = 0; k < n; ++k) {
            hipError_t e = hipEventRecord(event[k], forked[k]);
            if (e == hipSuccess) e = hipStreamWaitEvent(caller, event[k], 0);
            if (rc == hipSuccess) rc = e;
        }
        n = 0;
        return rc;
    }
    ~Join() { (void)join(); }
};

// Model step ai of a lane on its own stream, in two halves: the step's graph up to the edge encoder, then the propagation rounds and the state step
static void step_graph(ag_model *m, Lane &l, int ai)
{
    AgFwdArgs &f = l.f;
    // (step-invariant when de-duplicated, see run_node_encode; in front of the edge build, whose sender-map rider needs its node_row)
    if (ai == 1 || !f.dedup) run_node_encode(m, f, l.s);
    int riders;
    { Timed tm(m, AG_K_EDGES, l.s); riders = ag_launch_build_edges(l.e, l.s); }
    f.tab_done = (riders & AG_RIDER_TAB) != 0;
    f.remap_done = (riders & AG_RIDER_MAP) != 0;
    run_node_encode_fallback(m, f, l.s);
    run_edge_encode(m, f, l.path, l.s);
}
static void step_rounds(ag_model *m, Lane &l, int ai)
{
    run_propagate(m, l.f, l.path, l.s);
    l.st.step = ai;
    { Timed tm(m, AG_K_ROLLOUT_STEP, l.s); ag_launch_rollout_step(l.st, l.s); }
}

// One stream per part, the steps issued round-robin over the parts so every stream always has work queued
static int issue_round_robin(ag_model *m, hipStream_t s0, Lane *lane, int parts, int n_steps)
{
    for (int ai = 1; ai <= n_steps; ++ai)
        for (int k = 0; k < parts; ++k) {
            step_graph(m, lane[k], ai);
            if (ai == 1 && k == 0 && parts > 1) {
                // phase offset: the other parts start once part 0 has finished its first MFMA-bound encode stage, so
                // from then on one stream's HBM-bound segment reduce co-runs with another stream's MFMA-bound stage
                AG_HIP(hipEventRecord(m->ev_fork, s0));
                for (int kk = 1; kk < parts; ++kk) AG_HIP(hipStreamWaitEvent(m->aux_stream[kk], m->ev_fork, 0));
            }
            step_rounds(m, lane[k], ai);
        }
    return AG_OK;
}

// Two in-order queues with disjoint CU masks.  HBM queue (sR): edge build -> [ready] ... [encoded] -> three propagation rounds -> state step;
// MFMA queue (sE): [ready] -> per-node input rows + edge encoder + sender remap -> [encoded].  Part k's step ai + 1 cannot start before its
// step ai has finished (the edges are rebuilt from the predicted positions), so with two parts the steady state is
//     sE:  E(A, i+1)  E(B, i+1)  E(A, i+2) ...          sR:  R(B, i)  R(A, i+1)  R(B, i+1) ...
// each partition always busy with its own kind of work, the other part's.  Every table is per part, and E(k, i+1) is ordered behind
// R(k, i) through `ready`, so nothing is overwritten while it is read.
// Enqueue order matters (both queues are in order): a part's NEXT edge build follows its own state step directly, and the wait for the
// encoder stands in front of the rounds that need it — not in front of the other part's edge build.
static int issue_partitioned(ag_model *m, Lane *lane, int parts, int n_steps)
{
    hipStream_t sE = m->mfma_stream, sR = m->hbm_stream;
    auto graph_of_step = [&](int k, int ai) -> int {       // sR: edge build, node encoder -> ready;  sE: ready -> edge encoder -> encoded
        AgFwdArgs &f = lane[k].f;
        { Timed tm(m, AG_K_EDGES, sR); ag_launch_build_edges(lane[k].e, sR); }
        if (ai == 1 || !f.dedup) run_node_encode(m, f, sR);
        run_node_encode_fallback(m, f, sR);
        AG_HIP(hipEventRecord(m->ev_ready[k], sR));
        AG_HIP(hipStreamWaitEvent(sE, m->ev_ready[k], 0));
        run_edge_encode(m, f, lane[k].path, sE);
        AG_HIP(hipEventRecord(m->ev_enc[k], sE));
        return AG_OK;
    };
    for (int k = 0; k < parts && n_steps > 0; ++k)
        if (int rc = graph_of_step(k, 1)) return rc;
    for (int ai = 1; ai <= n_steps; ++ai)
        for (int k = 0; k < parts; ++k) {
            AG_HIP(hipStreamWaitEvent(sR, m->ev_enc[k], 0));
            run_propagate(m, lane[k].f, lane[k].path, sR);
            lane[k].st.step = ai;
            { Timed tm(m, AG_K_ROLLOUT_STEP, sR); ag_launch_rollout_step(lane[k].st, sR); }
            if (ai < n_steps)
                if (int rc = graph_of_step(k, ai + 1)) return rc;
        }
    return AG_OK;
}

// The argument checks ag_rollout and ag_rollout_ragged share, up to the first read of the model (`who`: the entry point, for the message)
static int rollout_args_ok(const char *who, const ag_model *m, const ag_rollout_params *p, const RolloutIn &in, const float *out_seq, const void *workspace)
{
    if (!m || !p || !in.state0 || !in.delta || !in.attrs || (!in.p_instance && p->n_instance > 0) || !in.mask || !in.tool_mask || !in.thr_sq ||
        !in.repeat || !out_seq || !workspace)
        return ag_fail(AG_ERR_ARG, "%s: null argument", who);
    if (p->height_mode == AG_HEIGHT_MASKED_MEAN && !in.obj_mask) return ag_fail(AG_ERR_ARG, "%s: obj_mask is null", who);
    if (p->B < 1 || p->N < 1 || p->n_p < 1 || p->n_p > p->N || p->topk < 1 || p->topk > 64 || p->n_steps < 0)
        return ag_fail(AG_ERR_ARG, "%s: bad sizes", who);
    return AG_OK;
}

int ag_rollout(ag_model *m, const ag_rollout_params *p, const float *state0, const float *delta, const float *attrs,
               const float *p_instance, const float *phys, const uint8_t *mask, const uint8_t *tool_mask,
               const uint8_t *obj_mask, const float *thr_sq, const int32_t *repeat, float *out_seq,
               float *state_final, void *workspace, size_t workspace_bytes, ag_stream_t stream)
{
    const RolloutIn in{state0, delta, attrs, p_instance, phys, mask, tool_mask, obj_mask, thr_sq, repeat};
    if (int rc = rollout_args_ok("ag_rollout", m, p, in, out_seq, workspace)) return rc;
    if (m->cfg.phys_dim > 0 && !phys) return ag_fail(AG_ERR_ARG, "ag_rollout: phys is null");
    hipStream_t s0 = static_cast<hipStream_t>(stream);
    if (shared_applicable(m, p))
        return rollout_shared(m, p, state0, delta, attrs, p_instance, phys, mask, tool_mask, obj_mask, thr_sq, repeat, out_seq, state_final, workspace,
                              workspace_bytes, s0);
    const int H = m->cfg.n_his, N = p->N;
    const int parts = rollout_parts(p->B, rollout_want(m, p));
    for (int k = 1; k < parts; ++k)
        if (!m->aux_stream[k]) {
            AG_HIP(hipStreamCreateWithFlags(&m->aux_stream[k], hipStreamNonBlocking));
            AG_HIP(hipEventCreateWithFlags(&m->ev_join[k], hipEventDisableTiming));
        }
    if (parts > 1 && !m->ev_fork) AG_HIP(hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming));
    Lane lane[AG_MAX_PARTS];
    Carver c(workspace, workspace_bytes);
    carve_parts(c, m, p, parts, lane);
    if (!c.ok()) return ag_fail(AG_ERR_WS, "ag_rollout: workspace %zu < %zu bytes", workspace_bytes, c.off);
    // (needs >= 2 batch parts and the weight-stationary edge encoder for the whole batch, whose grid is one workgroup per CU)
    const bool partitioned = m->cu_split > 0 && parts >= 2 && resolve_path(m, p->B, N, p->n_instance).edge == AG_EDGE_H3_WS;
    if (partitioned)
        if (int rc = ensure_partition(m)) return rc;
    const size_t plane = (size_t)N * 3;
    const int part_blocks = m->max_blocks / parts > 0 ? m->max_blocks / parts : 1;   // each part's persistent kernels take an equal share
    for (int k = 0; k < parts; ++k) {      // the parts' arguments (nothing is enqueued here)
        lane[k].s = partitioned ? m->hbm_stream : (k == 0 ? s0 : m->aux_stream[k]);
        bind_part(m, p, lane[k], in, out_seq, partitioned, part_blocks);
    }
    Join join{s0};
    if (parts > 1) AG_HIP(hipEventRecord(m->ev_fork, s0));
    for (int k = 1; k < parts; ++k)
        if (partitioned) AG_HIP(hipStreamWaitEvent(m->aux_stream[k], m->ev_fork, 0));    // (the part streams wait on the fork and get no work)
        else AG_HIP(join.fork(m->aux_stream[k], m->ev_fork, m->ev_join[k]));
    if (partitioned) {      // (joined in this order: the MFMA queue, then the HBM queue)
        AG_HIP(join.fork(m->mfma_stream, m->ev_fork, m->ev_join_mfma));
        AG_HIP(join.fork(m->hbm_stream, m->ev_fork, m->ev_join[1]));
    }
    for (const Lane *l = lane; l < lane + parts; ++l)
        AG_HIP(hipMemcpyAsync(l->state, state0 + (size_t)l->b0 * H * plane, (size_t)l->B * H * plane * sizeof(float), hipMemcpyDeviceToDevice, l->s));
    if (int rc = partitioned ? issue_partitioned(m, lane, parts, p->n_steps) : issue_round_robin(m, s0, lane, parts, p->n_steps)) return rc;
    for (const Lane *l = lane; l < lane + parts && state_final; ++l)
        AG_HIP(hipMemcpyAsync(state_final + (size_t)l->b0 * H * plane, l->state, (size_t)l->B * H * plane * sizeof(float), hipMemcpyDeviceToDevice, l->s));
    AG_HIP(join.join());
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_rollout_order(const int32_t *repeat, int B, int32_t *order, int32_t *active, ag_stream_t stream)
{
    if (!repeat || !order || !active) return ag_fail(AG_ERR_ARG, "ag_rollout_order: null argument");
    if (B < 1) return ag_fail(AG_ERR_ARG, "ag_rollout_order: B=%d (>= 1)", B);
    ag_launch_rollout_order(repeat, B, order, active, static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

// ag_rollout on a batch in the order of ag_rollout_order, one stream: the plain driver as ONE part, or the shared-state driver, with every launch of
// model step ai sized for the first active_per_step[ai - 1] samples.  A retired sample's rows are never touched again: its history stands still at its
// own last step (state_final), and nothing it would have computed later is recorded anywhere (forward_dynamics.py:160-161).
int ag_rollout_ragged(ag_model *m, const ag_rollout_params *p, const float *state0, const float *delta, const float *attrs, const float *p_instance,
                      const float *phys, const uint8_t *mask, const uint8_t *tool_mask, const uint8_t *obj_mask, const float *thr_sq,
                      const int32_t *repeat, const int32_t *active_per_step, const int32_t *out_index, float *out_seq, float *state_final,
                      void *workspace, size_t workspace_bytes, ag_stream_t stream)
{
    const RolloutIn in{state0, delta, attrs, p_instance, phys, mask, tool_mask, obj_mask, thr_sq, repeat};
    if (int rc = rollout_args_ok("ag_rollout_ragged", m, p, in, out_seq, workspace)) return rc;
    // (the step counts are checked before the model is read)
    if (p->n_steps > AG_RAGGED_MAX_STEPS) return ag_fail(AG_ERR_ARG, "ag_rollout_ragged: n_steps=%d (<= %d)", p->n_steps, AG_RAGGED_MAX_STEPS);
    if (!active_per_step && p->n_steps > 0) return ag_fail(AG_ERR_ARG, "ag_rollout_ragged: null argument (active_per_step)");
    for (int ai = 0; ai < p->n_steps; ++ai)
        if (active_per_step[ai] < 0 || active_per_step[ai] > (ai > 0 ? active_per_step[ai - 1] : p->B))
            return ag_fail(AG_ERR_ARG, "ag_rollout_ragged: active_per_step[%d]=%d (non-increasing, 0..B=%d)", ai, active_per_step[ai], p->B);
    if (m->cfg.phys_dim > 0 && !phys) return ag_fail(AG_ERR_ARG, "ag_rollout_ragged: phys is null");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Ragged rg{active_per_step, out_index};
    if (shared_applicable(m, p))
        return rollout_shared(m, p, state0, delta, attrs, p_instance, phys, mask, tool_mask, obj_mask, thr_sq, repeat, out_seq, state_final, workspace,
                              workspace_bytes, s, &rg);
    Lane l;
    Carver c(workspace, workspace_bytes);
    carve_parts(c, m, p, 1, &l);
    if (!c.ok()) return ag_fail(AG_ERR_WS, "ag_rollout_ragged: workspace %zu < %zu bytes", workspace_bytes, c.off);
    l.s = s;
    bind_part(m, p, l, in, out_seq, false, m->max_blocks);
    const int H = m->cfg.n_his;
    l.st.out_index = out_index; l.st.out_rows = p->B; l.st.status = m->status;
    AG_HIP(hipMemcpyAsync(l.state, state0, (size_t)p->B * H * p->N * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    for (int ai = 1; ai <= p->n_steps && active_per_step[ai - 1] > 0; ++ai) {
        l.e.B = l.f.B = l.st.B = active_per_step[ai - 1];      // counts and grids shrink; bases and row numbers are the whole batch's
        step_graph(m, l, ai);
        step_rounds(m, l, ai);
    }
    ag_launch_ragged_finish(l.state, repeat, out_index, state_final, p->B, H, p->N, m->status, s);
    AG_HIP(hipGetLastError());
    return AG_OK;
}

// ---- scripted rollout (ag_scripted.hip): per step exactly the launches of ag_build_edges + ag_forward, then the scripted state update -------------
static bool scripted_sizes_ok(const ag_scripted_params *p)
{
    return p->B >= 1 && p->N >= 1 && p->n_p >= 1 && p->n_p <= p->N && p->n_instance >= 0 && p->topk >= 1 && p->topk <= 64 && p->max_tools >= 0 &&
           p->n_steps >= 1 && (p->variant == AG_VARIANT_SINGLE || p->variant == AG_VARIANT_BATCH) && (int64_t)p->B * p->N < (1ll << 31) / 64 &&
           ag_edge_capacity(p->B, p->N, p->topk, p->connect_tools_all, p->max_tools) <= 0x7fffffff;
}

// its layout (the forward is ag_forward's: no self-edge elision); returns the buffer of the next step's action, which the state update writes
static float *carve_scripted(Carver &c, const ag_scripted_params *p, Lane &l, bool eterm16)
{
    const size_t rows = (size_t)p->B * p->N;
    l.state = c.take<float>(rows * AG_NHIS * 3);
    float *action = c.take<float>(rows * 3);
    carve_step(c, l, p, p->B, p->n_p, false, eterm16);
    return action;
}

size_t ag_rollout_scripted_workspace_bytes_for(const ag_model *m, const ag_scripted_params *p)
{
    if (!p || !scripted_sizes_ok(p)) return 0;
    Carver c(nullptr, 0);
    Lane l;
    carve_scripted(c, p, l, resolve_path(m, p->B, p->N, p->n_instance).q16);
    return align_up(c.off, 256);
}

int ag_rollout_scripted(ag_model *m, const ag_scripted_params *p, const float *state0, const float *action0, const float *tool_pos,
                        const float *tool_delta, const float *attrs, const float *p_instance, const float *phys, const uint8_t *mask,
                        const uint8_t *tool_mask, const float *thr_sq, const float *gt, const uint8_t *obj_mask, float *pred_seq, float *err,
                        float *state_final, void *workspace, size_t workspace_bytes, ag_stream_t stream)
{
    if (!m || !p || !state0 || !action0 || !attrs || (!p_instance && p->n_instance > 0) || !mask || !tool_mask || !thr_sq || !workspace)
        return ag_fail(AG_ERR_ARG, "ag_rollout_scripted: null argument");
    if (p->n_steps < 1) return ag_fail(AG_ERR_ARG, "ag_rollout_scripted: n_steps=%d (>= 1)", p->n_steps);
    if (p->n_p > p->N || p->topk < 1 || p->topk > 64)
        return ag_fail(AG_ERR_ARG, "ag_rollout_scripted: n_p=%d (<= N=%d) topk=%d (1..64)", p->n_p, p->N, p->topk);
    if (!scripted_sizes_ok(p))
        return ag_fail(AG_ERR_ARG, "ag_rollout_scripted: bad sizes B=%d N=%d n_p=%d n_instance=%d max_tools=%d variant=%d", p->B, p->N, p->n_p,
                    p->n_instance, p->max_tools, p->variant);
    if ((gt != nullptr) != (err != nullptr)) return ag_fail(AG_ERR_ARG, "ag_rollout_scripted: gt and err are given together or not at all");
    if (!pred_seq && !err && !state_final) return ag_fail(AG_ERR_ARG, "ag_rollout_scripted: no output: pred_seq, err and state_final are all null");
    if (p->N > p->n_p && p->n_steps > 1 && (!tool_pos || !tool_delta))
        return ag_fail(AG_ERR_ARG, "ag_rollout_scripted: null tool script (%d tool slots, %d steps)", p->N - p->n_p, p->n_steps);
    if (m->cfg.phys_dim > 0 && !phys) return ag_fail(AG_ERR_ARG, "ag_rollout_scripted: phys is null");
    // the path of an ag_forward call of this batch (one model step per forward: the node inputs change every step, nothing is hoisted)
    Lane l;
    l.path = resolve_path(m, p->B, p->N, p->n_instance);
    Carver c(workspace, workspace_bytes);
    float *action = carve_scripted(c, p, l, l.path.q16);
    // (against the query's rounded-up figure: a buffer one byte short of what the query asked for is refused, whatever the carving's last offset)
    if (!c.ok() || workspace_bytes < align_up(c.off, 256))
        return ag_fail(AG_ERR_WS, "ag_rollout_scripted: workspace %zu < %zu bytes", workspace_bytes, align_up(c.off, 256));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int N = p->N, n_p = p->n_p, T = p->n_steps;
    const size_t plane = (size_t)N * 3, state_bytes = (size_t)p->B * AG_NHIS * plane * sizeof(float);
    AG_HIP(hipMemcpyAsync(l.state, state0, state_bytes, hipMemcpyDeviceToDevice, s));
    AgEdgeArgs &e = l.e;
    AgFwdArgs &f = l.f;
    bind_edges(l, p, p->variant, AG_NHIS, mask, tool_mask, thr_sq);
    bind_forward(m, f, p->B, N, n_p, p->n_instance, l.state, attrs, action0, p_instance, phys, e.row_ptr, e.edge_recv, e.edge_send, l.pred_pos,
                 l.pred_motion);
    setup_args(m, f, l.path, m->max_blocks);
    AgScriptArgs st{};
    st.state = l.state; st.action = action; st.pred_pos = l.pred_pos; st.tool_pos = tool_pos; st.tool_delta = tool_delta;
    st.gt = gt; st.obj_mask = obj_mask; st.pred_seq = pred_seq; st.err = err;
    st.B = p->B; st.N = N; st.n_p = n_p; st.T = T;
    for (int t = 0; t < T; ++t) {
        { Timed tm(m, AG_K_EDGES, s); ag_launch_build_edges(e, s); }
        f.action = t == 0 ? action0 : action;
        run_node_encode(m, f, s);
        run_node_encode_fallback(m, f, s);
        run_edge_encode(m, f, l.path, s);
        run_propagate(m, f, l.path, s);
        st.t = t;
        { Timed tm(m, AG_K_ROLLOUT_STEP, s); ag_launch_scripted_step(st, s); }
    }
    if (state_final) AG_HIP(hipMemcpyAsync(state_final, l.state, state_bytes, hipMemcpyDeviceToDevice, s));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

}  // extern "C"
