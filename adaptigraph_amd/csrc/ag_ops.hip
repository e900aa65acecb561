// ag_ops.hip — the stateless operators of the C ABI (include/adaptigraph_hip.h): chamfer, planner cost, key-point sampling, batch assembly, the
// training ops.  Argument checks and one launch each; nothing here knows a model.
#include "ag_host.h"

extern "C" {

// ---- the cloud-distance operators: what their entry points check alike, before anything is launched ----
// have_all: every pointer the call cannot do without is there; masks come as a pair or not at all
static int cloud_pointers(const char *who, bool have_all, const uint8_t *xm, const uint8_t *ym)
{
    if (!have_all) return ag_fail(AG_ERR_ARG, "%s: null argument", who);
    if ((xm == nullptr) != (ym == nullptr)) return ag_fail(AG_ERR_ARG, "%s: give both masks or neither", who);
    return AG_OK;
}

static int cloud_sizes(const char *who, int B, int N, int M)
{
    if (B < 1 || N < 1 || M < 1) return ag_fail(AG_ERR_ARG, "%s: bad sizes B=%d N=%d M=%d", who, B, N, M);
    return AG_OK;
}

static int cloud_args(const char *who, bool have_all, const uint8_t *xm, const uint8_t *ym, int B, int N, int M)
{
    if (int rc = cloud_pointers(who, have_all, xm, ym)) return rc;
    return cloud_sizes(who, B, N, M);
}

static int cloud_launched()      // behind a launcher that took the call
{
    AG_HIP(hipGetLastError());
    return AG_OK;
}

static int over_resident_limit(const char *who, int N, int M)
{
    return ag_fail(AG_ERR_ARG, "%s: N + M = %lld exceeds the LDS-resident limit (%d points)", who, (long long)N + M, kCloudResidentPoints);
}

static int chamfer_common(const char *who, const float *x, const uint8_t *xm, const float *y, const uint8_t *ym, int B, int N, int M,
                          int y_batched, float *out, ag_stream_t stream)
{
    if (int rc = cloud_args(who, x && y && out, xm, ym, B, N, M)) return rc;
    if (ag_launch_chamfer(x, y, xm, ym, B, N, M, y_batched ? 1 : 0, out, static_cast<hipStream_t>(stream)) != 0)
        return over_resident_limit(who, N, M);
    return cloud_launched();
}

int ag_chamfer(const float *x, const float *y, int B, int N, int M, int y_batched, float *out, ag_stream_t stream)
{
    return chamfer_common("ag_chamfer", x, nullptr, y, nullptr, B, N, M, y_batched, out, stream);
}

int ag_chamfer_masked(const float *x, const uint8_t *x_mask, const float *y, const uint8_t *y_mask, int B, int N, int M,
                      int y_batched, float *out, ag_stream_t stream)
{
    if (!x_mask || !y_mask) return ag_fail(AG_ERR_ARG, "ag_chamfer_masked: null mask");
    return chamfer_common("ag_chamfer_masked", x, x_mask, y, y_mask, B, N, M, y_batched, out, stream);
}

int ag_chamfer_fwd_idx(const float *x, const uint8_t *x_mask, const float *y, const uint8_t *y_mask, int B, int N, int M, int y_batched,
                       float *out, int32_t *idx_x, int32_t *idx_y, ag_stream_t stream)
{
    const char *who = "ag_chamfer_fwd_idx";
    if (int rc = cloud_args(who, x && y && out && idx_x && idx_y, x_mask, y_mask, B, N, M)) return rc;
    if (ag_launch_chamfer_idx(x, y, x_mask, y_mask, B, N, M, y_batched ? 1 : 0, out, idx_x, idx_y, static_cast<hipStream_t>(stream)) != 0)
        return over_resident_limit(who, N, M);
    return cloud_launched();
}

int ag_chamfer_backward(const float *x, const uint8_t *x_mask, const float *y, const uint8_t *y_mask, const int32_t *idx_x, const int32_t *idx_y,
                        const float *grad_out, int B, int N, int M, int y_batched, float *gx, float *gy, ag_stream_t stream)
{
    const char *who = "ag_chamfer_backward";
    if (int rc = cloud_args(who, x && y && idx_x && idx_y && grad_out && gx, x_mask, y_mask, B, N, M)) return rc;
    if (ag_launch_chamfer_backward(x, x_mask, y, y_mask, idx_x, idx_y, grad_out, B, N, M, y_batched ? 1 : 0, gx, gy,
                                   static_cast<hipStream_t>(stream)) != 0)
        return over_resident_limit(who, N, M);
    return cloud_launched();
}

// ---- the tiled chamfer: clouds of any size up to 2^24 points a side (the valid counts are float adds of 1, exact up to there) ----
static const int kChamMaxPoints = 1 << 24;

void ag_chamfer_tile_sizes(int *query_tile, int *other_chunk)
{
    if (query_tile) *query_tile = kChamTQ;
    if (other_chunk) *other_chunk = kChamTO;
}

// near: one float per point of both clouds of every sample
size_t ag_chamfer_tiled_workspace_bytes(int B, int N, int M)
{
    if (B < 1 || N < 1 || M < 1 || N > kChamMaxPoints || M > kChamMaxPoints) return 0;
    return align_up((size_t)B * ((size_t)N + (size_t)M) * sizeof(float), 256);
}

static int chamfer_tiled_sizes(const char *who, int N, int M)
{
    if (N > kChamMaxPoints || M > kChamMaxPoints) return ag_fail(AG_ERR_ARG, "%s: N=%d M=%d exceed %d points a side", who, N, M, kChamMaxPoints);
    return AG_OK;
}

int ag_chamfer_tiled(const float *x, const uint8_t *x_mask, const float *y, const uint8_t *y_mask, int B, int N, int M, int y_batched, float *out,
                     int32_t *idx_x, int32_t *idx_y, void *ws, size_t ws_bytes, ag_stream_t stream)
{
    const char *who = "ag_chamfer_tiled";
    if (int rc = cloud_pointers(who, x && y && out, x_mask, y_mask)) return rc;
    if ((idx_x == nullptr) != (idx_y == nullptr)) return ag_fail(AG_ERR_ARG, "%s: give both index outputs or neither", who);
    if (int rc = cloud_sizes(who, B, N, M)) return rc;
    if (int rc = chamfer_tiled_sizes(who, N, M)) return rc;
    const size_t need = ag_chamfer_tiled_workspace_bytes(B, N, M);
    if (!ws || ws_bytes < need) return ag_fail(AG_ERR_WS, "%s: workspace %zu < %zu bytes", who, ws ? ws_bytes : (size_t)0, need);
    float *near = static_cast<float *>(ws);
    if (ag_launch_chamfer_tiled(x, y, x_mask, y_mask, B, N, M, y_batched ? 1 : 0, out, idx_x, idx_y, near, static_cast<hipStream_t>(stream)) != 0)
        return ag_fail(AG_ERR_ARG, "%s: B=%d samples of %d + %d points need more workgroups than one launch holds", who, B, N, M);
    return cloud_launched();
}

int ag_chamfer_tiled_backward(const float *x, const uint8_t *x_mask, const float *y, const uint8_t *y_mask, const int32_t *idx_x,
                              const int32_t *idx_y, const float *grad_out, int B, int N, int M, int y_batched, float *gx, float *gy,
                              ag_stream_t stream)
{
    const char *who = "ag_chamfer_tiled_backward";
    if (int rc = cloud_args(who, x && y && idx_x && idx_y && grad_out && gx, x_mask, y_mask, B, N, M)) return rc;
    if (int rc = chamfer_tiled_sizes(who, N, M)) return rc;
    if (ag_launch_chamfer_tiled_backward(x, x_mask, y, y_mask, idx_x, idx_y, grad_out, B, N, M, y_batched ? 1 : 0, gx, gy,
                                         static_cast<hipStream_t>(stream)) != 0)
        return ag_fail(AG_ERR_ARG, "%s: B=%d samples of %d + %d points need more workgroups than one launch holds", who, B, N, M);
    return cloud_launched();
}

// ---- the matching losses (ag_match.hip) ----
static_assert(kEmdMaxPoints == AG_EMD_MAX_POINTS, "the kernel's register budget and the header's limit are one number");

int ag_emd(const float *x, const uint8_t *x_mask, const float *y, const uint8_t *y_mask, int B, int N, int M, int y_batched, float *out,
           int32_t *col, int32_t *row, ag_stream_t stream)
{
    const char *who = "ag_emd";
    if (int rc = cloud_args(who, x && y && out && col && row, x_mask, y_mask, B, N, M)) return rc;
    if (N > AG_EMD_MAX_POINTS || M > AG_EMD_MAX_POINTS)
        return ag_fail(AG_ERR_ARG, "%s: N=%d M=%d exceed AG_EMD_MAX_POINTS = %d points a side", who, N, M, AG_EMD_MAX_POINTS);
    if (ag_launch_emd(x, y, x_mask, y_mask, B, N, M, y_batched ? 1 : 0, out, col, row, static_cast<hipStream_t>(stream)) != 0)
        return ag_fail(AG_ERR_ARG, "%s: bad sizes N=%d M=%d", who, N, M);
    return cloud_launched();
}

int ag_emd_backward(const float *x, const float *y, const int32_t *col, const int32_t *row, const float *grad_out, int B, int N, int M, int y_batched,
                    float *gx, float *gy, ag_stream_t stream)
{
    const char *who = "ag_emd_backward";
    if (int rc = cloud_args(who, x && y && col && row && grad_out && gx, nullptr, nullptr, B, N, M)) return rc;
    if (N > AG_EMD_MAX_POINTS || M > AG_EMD_MAX_POINTS)
        return ag_fail(AG_ERR_ARG, "%s: N=%d M=%d exceed AG_EMD_MAX_POINTS = %d points a side", who, N, M, AG_EMD_MAX_POINTS);
    ag_launch_emd_backward(x, y, col, row, grad_out, B, N, M, y_batched ? 1 : 0, gx, gy, static_cast<hipStream_t>(stream));
    return cloud_launched();
}

int ag_hausdorff(const float *x, const uint8_t *x_mask, const float *y, const uint8_t *y_mask, int B, int N, int M, int y_batched, float *out,
                 int32_t *arg, ag_stream_t stream)
{
    const char *who = "ag_hausdorff";
    if (int rc = cloud_args(who, x && y && out && arg, x_mask, y_mask, B, N, M)) return rc;
    if (!ag_cloud_resident(N, M)) return over_resident_limit(who, N, M);
    if (ag_launch_hausdorff(x, y, x_mask, y_mask, B, N, M, y_batched ? 1 : 0, out, arg, static_cast<hipStream_t>(stream)) != 0)
        return ag_fail(AG_ERR_HIP, "%s: the kernel's LDS size was refused", who);
    return cloud_launched();
}

// ---- the planner's trajectory cost (ag_plan_cost.hip) ----
static const char *plan_cost_refusal(const ag_plan_cost_params *p)
{
    if (!p) return "null parameters";
    if (p->B < 1 || p->L < 1 || p->n < 1) return "B, L and n must be at least 1";
    if ((long long)p->B * p->L > (1LL << 30)) return "B * L exceeds 2^30 clouds";
    if (p->penalty < AG_PENALTY_NONE || p->penalty > AG_PENALTY_GRANULAR) return "unknown penalty";
    if (p->criterion != AG_ERROR_GIVEN && p->criterion != AG_ERROR_BOX) return "unknown criterion";
    return nullptr;
}

// the per-(b, l) term table of a call that passes no `terms`
size_t ag_plan_cost_workspace_bytes(const ag_plan_cost_params *p)
{
    if (plan_cost_refusal(p)) return 0;
    return align_up((size_t)p->B * p->L * AG_PLAN_TERMS * sizeof(float), 256);
}

static int plan_cost_call(const char *who, const ag_plan_cost_params *p, int n_chunk, const float *state_seqs, const float *action,
                          const float *state_init, const float *error_in, float *reward, float *terms, void *ws, size_t ws_bytes,
                          ag_stream_t stream)
{
    if (const char *why = plan_cost_refusal(p))
        return ag_fail(AG_ERR_ARG, "%s: %s (B=%d L=%d n=%d penalty=%d criterion=%d)", who, why, p ? p->B : 0, p ? p->L : 0, p ? p->n : 0,
                    p ? p->penalty : 0, p ? p->criterion : 0);
    if (n_chunk < 1 || p->B % n_chunk != 0)
        return ag_fail(AG_ERR_ARG, "%s: B=%d is not n_chunk=%d chunks of S >= 1 samples each", who, p->B, n_chunk);
    if (!state_seqs || !action || !state_init || !reward) return ag_fail(AG_ERR_ARG, "%s: null argument", who);
    if (p->criterion == AG_ERROR_GIVEN && !error_in) return ag_fail(AG_ERR_ARG, "%s: AG_ERROR_GIVEN needs error_in", who);
    const size_t need = ag_plan_cost_workspace_bytes(p);
    if (!ws || ws_bytes < need) return ag_fail(AG_ERR_WS, "%s: workspace %zu < %zu bytes", who, ws ? ws_bytes : (size_t)0, need);
    AgPlanCostArgs a{};
    a.state_seqs = state_seqs; a.action = action; a.state_init = state_init; a.error_in = error_in;
    a.reward = reward;
    a.terms = terms ? terms : static_cast<float *>(ws);
    a.B = p->B; a.L = p->L; a.n = p->n; a.penalty = p->penalty; a.box_criterion = p->criterion == AG_ERROR_BOX;
    // the reference's thresholds are Python doubles (0.05 * sim_real_ratio ...) that a tensor op rounds to float once
    const double r = (double)p->sim_real_ratio;
    a.rad = (float)(0.05 * r); a.touch = (float)(0.02 * r); a.grasp = (float)(0.005 * r); a.far_cap = (float)(0.4 * r);
    for (int i = 0; i < 4; ++i) { a.bbox[i] = p->bbox[i]; a.box[i] = p->box[i]; }
    ag_launch_plan_cost(a, n_chunk, static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_plan_cost(const ag_plan_cost_params *p, const float *state_seqs, const float *action, const float *state_init, const float *error_in,
                 float *reward, float *terms, void *ws, size_t ws_bytes, ag_stream_t stream)
{
    return plan_cost_call("ag_plan_cost", p, 1, state_seqs, action, state_init, error_in, reward, terms, ws, ws_bytes, stream);
}

int ag_plan_cost_chunked(const ag_plan_cost_params *p, int n_chunk, const float *state_seqs, const float *action, const float *state_init,
                         const float *error_in, float *reward, float *terms, void *ws, size_t ws_bytes, ag_stream_t stream)
{
    return plan_cost_call("ag_plan_cost_chunked", p, n_chunk, state_seqs, action, state_init, error_in, reward, terms, ws, ws_bytes, stream);
}

// ---- the MPPI update of every chunk of a planning step (ag_mppi.hip) ----
int ag_mppi_update(const ag_mppi_params *p, const float *actions, const float *reward, float *new_seq, int32_t *best_idx, float *best_seq,
                   float *best_reward, ag_stream_t stream)
{
    const char *who = "ag_mppi_update";
    if (!p) return ag_fail(AG_ERR_ARG, "%s: null parameters", who);
    if (p->n_chunk < 1 || p->S < 1 || p->L < 1)
        return ag_fail(AG_ERR_ARG, "%s: n_chunk, S and L must be at least 1 (n_chunk=%d S=%d L=%d)", who, p->n_chunk, p->S, p->L);
    if ((long long)p->n_chunk * p->S > (1LL << 30) || (long long)p->n_chunk * p->S * p->L > (1LL << 30))
        return ag_fail(AG_ERR_ARG, "%s: n_chunk * S * L exceeds 2^30 (n_chunk=%d S=%d L=%d)", who, p->n_chunk, p->S, p->L);
    if (!actions || !reward) return ag_fail(AG_ERR_ARG, "%s: null argument", who);
    AgMppiArgs a{};
    a.actions = actions; a.reward = reward;
    a.new_seq = new_seq; a.best_idx = best_idx; a.best_seq = best_seq; a.best_reward = best_reward;
    a.n_chunk = p->n_chunk; a.S = p->S; a.L = p->L;
    a.reward_weight = p->reward_weight; a.push_length = p->push_length;
    for (int i = 0; i < 4; ++i) { a.lo[i] = p->lo[i]; a.hi[i] = p->hi[i]; }
    ag_launch_mppi_update(a, static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

// kept distances of the streaming form: one float per point of every cloud (asked of every call, so that the caller's buffer never depends on which
// form the library picks for a size)
size_t ag_fps_workspace_bytes(int B, int N)
{
    if (B < 1 || N < 1) return 0;
    return align_up((size_t)B * (size_t)N * sizeof(float), 256);
}

int ag_fps(const float *pts, const int32_t *count, const int32_t *start, int B, int N, int K, int metric, const double *radius, int32_t *idx,
           int32_t *n_out, void *workspace, size_t workspace_bytes, ag_stream_t stream)
{
    if (!pts || !start || !idx || !n_out) return ag_fail(AG_ERR_ARG, "ag_fps: null argument");
    if (B < 1 || N < 1 || K < 1) return ag_fail(AG_ERR_ARG, "ag_fps: bad sizes B=%d N=%d K=%d", B, N, K);
    if (metric != AG_FPS_SQUARED && metric != AG_FPS_NORM) return ag_fail(AG_ERR_ARG, "ag_fps: unknown metric %d", metric);
    if (radius && metric != AG_FPS_NORM) return ag_fail(AG_ERR_ARG, "ag_fps: a radius stop needs AG_FPS_NORM (the radius is a distance, not a squared one)");
    const size_t need = ag_fps_workspace_bytes(B, N);
    if (!workspace || workspace_bytes < need)
        return ag_fail(AG_ERR_ARG, "ag_fps: workspace of %zu bytes, ag_fps_workspace_bytes(%d, %d) = %zu", workspace ? workspace_bytes : (size_t)0, B, N, need);
    ag_launch_fps(pts, count, start, B, N, K, metric, radius, idx, n_out, static_cast<float *>(workspace), static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_gather_clouds(const float *obj_store, const int64_t *episodes, int n_episodes, const int32_t *epi, const int32_t *frame, int B, int Nmax,
                     float *pts, int32_t *count, ag_stream_t stream)
{
    const struct { const void *p; const char *name; } ptrs[] = {{obj_store, "obj_store"}, {episodes, "episodes"}, {epi, "epi"}, {frame, "frame"},
                                                                {pts, "pts"}, {count, "count"}};
    for (const auto &a : ptrs)
        if (!a.p) return ag_fail(AG_ERR_ARG, "ag_gather_clouds: %s is null", a.name);
    if (n_episodes < 1 || B < 1 || B > 65535 || Nmax < 1)
        return ag_fail(AG_ERR_ARG, "ag_gather_clouds: bad sizes n_episodes=%d B=%d (1..65535) Nmax=%d", n_episodes, B, Nmax);
    ag_launch_gather_clouds(obj_store, episodes, n_episodes, epi, frame, B, Nmax, pts, count, static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_assemble_batch(const ag_batch_dims *dims, const float *obj_store, const void *tool_store, const int64_t *episodes, const int32_t *epi,
                      const int32_t *frames, const int32_t *picks, const double *noise, const float *rot, const ag_batch_out *out,
                      ag_stream_t stream)
{
    if (!dims) return ag_fail(AG_ERR_ARG, "ag_assemble_batch: dims is null");
    if (!out) return ag_fail(AG_ERR_ARG, "ag_assemble_batch: out is null");
    const ag_batch_dims &d = *dims;
    if (d.B < 1 || d.B > 65535 || d.H < 1 || d.Fu < 1 || d.H + d.Fu > 65535 || d.no < 1 || d.n_eef < 1 || d.K < 1 || d.n_episodes < 1)
        return ag_fail(AG_ERR_ARG, "ag_assemble_batch: bad sizes B=%d (1..65535) H=%d Fu=%d no=%d n_eef=%d K=%d n_episodes=%d", d.B, d.H, d.Fu, d.no,
                    d.n_eef, d.K, d.n_episodes);
    if (d.n_mat < 1 || d.mat_col < 0 || d.mat_col >= d.n_mat)
        return ag_fail(AG_ERR_ARG, "ag_assemble_batch: mat_col=%d outside n_mat=%d", d.mat_col, d.n_mat);
    if ((noise == nullptr) != (rot == nullptr))
        return ag_fail(AG_ERR_ARG, "ag_assemble_batch: give both noise and rot or neither (%s is null)", noise ? "rot" : "noise");
    const bool futures = d.Fu > 1;      // with Fu == 1 the two (B, Fu - 1, ns, 3) tensors are empty
    const struct { const void *p; const char *name; bool needed; } ptrs[] = {
        {obj_store, "obj_store", true}, {tool_store, "tool_store", true}, {episodes, "episodes", true}, {epi, "epi", true}, {frames, "frames", true},
        {picks, "picks", true}, {out->state, "out.state", true}, {out->action, "out.action", true}, {out->eef_future, "out.eef_future", futures},
        {out->action_future, "out.action_future", futures}, {out->state_future, "out.state_future", true}, {out->attrs, "out.attrs", true},
        {out->p_instance, "out.p_instance", true}, {out->obj_mask, "out.obj_mask", true}, {out->state_mask, "out.state_mask", true},
        {out->eef_mask, "out.eef_mask", true}, {out->material_index, "out.material_index", true}};
    for (const auto &a : ptrs)
        if (a.needed && !a.p) return ag_fail(AG_ERR_ARG, "ag_assemble_batch: %s is null", a.name);
    ag_launch_assemble_batch(d, obj_store, tool_store, episodes, epi, frames, picks, noise, rot, *out, static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_gather_rows(const float *x, const int32_t *idx, float *out, int64_t n_out, int D, ag_stream_t stream)
{
    if (n_out < 0 || D < 1) return ag_fail(AG_ERR_ARG, "ag_gather_rows: bad sizes n_out=%lld D=%d", (long long)n_out, D);
    if (n_out > 0 && (!x || !idx || !out)) return ag_fail(AG_ERR_ARG, "ag_gather_rows: null argument");
    ag_launch_gather_rows(x, idx, out, n_out, D, static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_segment_sum(const float *vals, const int32_t *ptr, const int32_t *perm, float *out, int64_t n_seg, int D, ag_stream_t stream)
{
    if (n_seg < 0 || D < 1) return ag_fail(AG_ERR_ARG, "ag_segment_sum: bad sizes n_seg=%lld D=%d", (long long)n_seg, D);
    if (n_seg > 0 && (!vals || !ptr || !out)) return ag_fail(AG_ERR_ARG, "ag_segment_sum: null argument");
    ag_launch_segment_sum(vals, ptr, perm, out, n_seg, D, static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_message_forward(const float *eterm, const float *hr, const float *hs, const int32_t *row_ptr, const int32_t *send, float *agg,
                       int64_t n_nodes, int D, ag_stream_t stream)
{
    if (n_nodes < 0 || D < 1) return ag_fail(AG_ERR_ARG, "ag_message_forward: bad sizes");
    if (n_nodes > 0 && (!eterm || !hr || !hs || !row_ptr || !send || !agg)) return ag_fail(AG_ERR_ARG, "ag_message_forward: null argument");
    ag_launch_message_fwd(eterm, hr, hs, row_ptr, send, agg, n_nodes, D, static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_message_backward(const float *eterm, const float *hr, const float *hs, const int32_t *row_ptr, const int32_t *send,
                        const float *grad_agg, float *grad_edge, float *grad_hr, int64_t n_nodes, int D, ag_stream_t stream)
{
    if (n_nodes < 0 || D < 1) return ag_fail(AG_ERR_ARG, "ag_message_backward: bad sizes");
    if (n_nodes > 0 && (!eterm || !hr || !hs || !row_ptr || !send || !grad_agg || !grad_edge || !grad_hr))
        return ag_fail(AG_ERR_ARG, "ag_message_backward: null argument");
    ag_launch_message_bwd(eterm, hr, hs, row_ptr, send, grad_agg, grad_edge, grad_hr, n_nodes, D, static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

size_t ag_edge_views_workspace_bytes(int B, int N)
{
    return (B > 0 && N > AG_VIEWS_LDS_N) ? (size_t)B * N * sizeof(int32_t) : 0;
}

int ag_edge_views(const int32_t *row_ptr, const int32_t *edge_send, int B, int N, int32_t *col_ptr, int32_t *send_perm, void *workspace,
                  ag_stream_t stream)
{
    if (B < 1 || N < 1 || (long long)B * N >= 0x7fffffffLL) return ag_fail(AG_ERR_ARG, "ag_edge_views: bad sizes B=%d N=%d", B, N);
    if (!row_ptr || !edge_send || !col_ptr || !send_perm) return ag_fail(AG_ERR_ARG, "ag_edge_views: null argument");
    if (N > AG_VIEWS_LDS_N && !workspace) return ag_fail(AG_ERR_WS, "ag_edge_views: N=%d needs a workspace of %zu bytes", N, ag_edge_views_workspace_bytes(B, N));
    ag_launch_edge_views(row_ptr, edge_send, B, N, col_ptr, send_perm, static_cast<int32_t *>(workspace), static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

static int step_update_check(const char *what, int B, int H, int N, int n_p, int height_mode, const void *obj_mask)
{
    if (B < 1 || H < 1 || n_p < 1 || N < n_p || (long long)B * H * N * 3 >= 0x7fffffffLL)
        return ag_fail(AG_ERR_ARG, "%s: bad sizes B=%d H=%d N=%d n_p=%d", what, B, H, N, n_p);
    if (height_mode != AG_HEIGHT_MIN && height_mode != AG_HEIGHT_MASKED_MEAN) return ag_fail(AG_ERR_ARG, "%s: height_mode=%d", what, height_mode);
    if (height_mode == AG_HEIGHT_MASKED_MEAN && !obj_mask) return ag_fail(AG_ERR_ARG, "%s: AG_HEIGHT_MASKED_MEAN needs obj_mask", what);
    return AG_OK;
}

int ag_step_update_forward(const float *pred, const float *state, const float *delta, const float *rec, const int32_t *repeat, const uint8_t *obj_mask,
                           int B, int H, int N, int n_p, int step, int height_mode, float raise, float *state_out, float *rec_out, ag_stream_t stream)
{
    if (const int rc = step_update_check("ag_step_update_forward", B, H, N, n_p, height_mode, obj_mask)) return rc;
    if (!pred || !state || !delta || !repeat || !state_out || !rec_out) return ag_fail(AG_ERR_ARG, "ag_step_update_forward: null argument");
    AgStepUpdateArgs a{};
    a.pred = pred; a.state = state; a.delta = delta; a.rec = rec; a.repeat = repeat; a.obj_mask = obj_mask;
    a.B = B; a.H = H; a.N = N; a.n_p = n_p; a.step = step; a.height_mode = height_mode; a.raise = raise;
    a.state_out = state_out; a.rec_out = rec_out;
    ag_launch_step_update(a, 0, static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_step_update_backward(const float *pred, const int32_t *repeat, const uint8_t *obj_mask, int B, int H, int N, int n_p, int step, int height_mode,
                            const float *grad_state_out, const float *grad_rec_out, float *grad_pred, float *grad_state, float *grad_delta,
                            float *grad_rec, ag_stream_t stream)
{
    if (const int rc = step_update_check("ag_step_update_backward", B, H, N, n_p, height_mode, obj_mask)) return rc;
    if (!pred || !repeat || !grad_state_out || !grad_pred || !grad_state || !grad_delta) return ag_fail(AG_ERR_ARG, "ag_step_update_backward: null argument");
    AgStepUpdateArgs a{};
    a.pred = pred; a.repeat = repeat; a.obj_mask = obj_mask;
    a.B = B; a.H = H; a.N = N; a.n_p = n_p; a.step = step; a.height_mode = height_mode;
    a.g_state_out = grad_state_out; a.g_rec_out = grad_rec_out; a.g_pred = grad_pred; a.g_state = grad_state; a.g_delta = grad_delta; a.g_rec = grad_rec;
    ag_launch_step_update(a, 1, static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_train_pack(const float *W, const float *bias, int n_out, int n_in, int ld, int col0, int transposed, int compact, int n_tiles,
                  int precision, float *dst, ag_stream_t stream)
{
    if (!W || !dst) return ag_fail(AG_ERR_ARG, "ag_train_pack: null argument");
    if (n_out < 1 || n_in < 1 || n_in > AG_F || ld < 1 || col0 < 0 || n_tiles < 1 || n_tiles > AG_NT || n_out > 32 * n_tiles * (compact ? AG_NT : 1))
        return ag_fail(AG_ERR_ARG, "ag_train_pack: bad sizes n_out=%d n_in=%d ld=%d n_tiles=%d", n_out, n_in, ld, n_tiles);
    if (compact && n_in + (bias ? 1 : 0) > 32) return ag_fail(AG_ERR_ARG, "ag_train_pack: compact image holds <= 32 input columns");
    ag_launch_train_pack(W, bias, n_out, n_in, ld, col0, transposed ? 1 : 0, compact ? 1 : 0, n_tiles, precision ? 1 : 0, dst, static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_train_chain(int kind, int backward, int precision, const float *x, const float *packed, float *const *y, const float *dy,
                   float *const *dz, float *dx, int64_t rows, int d_in, ag_stream_t stream)
{
    if (kind < AG_CHAIN_EDGE || kind > AG_CHAIN_DECODER) return ag_fail(AG_ERR_ARG, "ag_train_chain: bad kind %d", kind);
    const int L = kind == AG_CHAIN_EDGE ? 4 : 3;
    if (!packed || !y || rows < 0 || (!backward && !x) || (backward && (!dy || !dz))) return ag_fail(AG_ERR_ARG, "ag_train_chain: null argument");
    if ((kind == AG_CHAIN_EDGE && d_in != AG_EDGE_IN) || (kind == AG_CHAIN_NODE && (d_in < 1 || d_in >= AG_NODE_IN_MAX)) ||
        (kind == AG_CHAIN_DECODER && d_in != AG_F))
        return ag_fail(AG_ERR_ARG, "ag_train_chain: d_in=%d does not fit kind %d", d_in, kind);
    AgChainArgsPOD p{};
    p.x = x; p.w = packed; p.dy = dy; p.dx = dx; p.rows = rows; p.d_in = d_in;
    for (int l = 0; l < L; ++l) {
        if (!y[l] || (backward && !dz[l])) return ag_fail(AG_ERR_ARG, "ag_train_chain: table %d is null", l);
        p.y[l] = y[l];
        p.dz[l] = backward ? dz[l] : nullptr;
    }
    if (rows == 0) return AG_OK;
    static int cus_of[64];      // CU count per device, queried once (hipGetDeviceProperties is far too slow for a per-launch call)
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64) {
        if (cus_of[dev] == 0) {
            hipDeviceProp_t prop;
            cus_of[dev] = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
        }
        cus = cus_of[dev];
    }
    ag_launch_chain(kind, backward ? 1 : 0, precision ? 1 : 0, p, AG_MLP_WG_PER_CU * cus, static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_edge_inputs_forward(const float *tab, int D, int attr_dim, int group_dim, const int32_t *recv, const int32_t *send, float *out, int64_t n_edges,
                           ag_stream_t stream)
{
    if (D < 1 || attr_dim < 0 || group_dim < 0 || attr_dim + group_dim > D || n_edges < 0) return ag_fail(AG_ERR_ARG, "ag_edge_inputs_forward: bad sizes");
    if (n_edges > 0 && (!tab || !recv || !send || !out)) return ag_fail(AG_ERR_ARG, "ag_edge_inputs_forward: null argument");
    ag_launch_edge_inputs_fwd(tab, D, attr_dim, group_dim, recv, send, out, n_edges, static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_edge_inputs_backward(const float *tab, int D, int attr_dim, int group_dim, const int32_t *recv, const int32_t *send, const int32_t *row_ptr,
                            const int32_t *col_ptr, const int32_t *send_perm, const float *grad_out, float *scratch_r, float *scratch_s, float *grad_tab,
                            int64_t n_edges, int64_t n_nodes, ag_stream_t stream)
{
    if (D < 1 || attr_dim < 0 || group_dim < 0 || attr_dim + group_dim > D || n_edges < 0 || n_nodes < 0) return ag_fail(AG_ERR_ARG, "ag_edge_inputs_backward: bad sizes");
    if (n_nodes > 0 && (!row_ptr || !col_ptr || !grad_tab)) return ag_fail(AG_ERR_ARG, "ag_edge_inputs_backward: null argument");
    if (n_edges > 0 && (!tab || !recv || !send || !send_perm || !grad_out || !scratch_r || !scratch_s)) return ag_fail(AG_ERR_ARG, "ag_edge_inputs_backward: null argument");
    ag_launch_edge_inputs_bwd(tab, D, attr_dim, group_dim, recv, send, row_ptr, col_ptr, send_perm, grad_out, scratch_r, scratch_s, grad_tab, n_edges, n_nodes,
                              static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_add3_relu(const float *a, const float *b, const float *c, float *y, int64_t n, ag_stream_t stream)
{
    if (n < 0 || (n & 3) || (n > 0 && (!a || !b || !c || !y))) return ag_fail(AG_ERR_ARG, "ag_add3_relu: n=%lld must be a non-negative multiple of 4, tensors non-null", (long long)n);
    ag_launch_add3_relu(a, b, c, y, n, static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

int ag_relu_mask(const float *g, const float *y, float *out, int64_t n, ag_stream_t stream)
{
    if (n < 0 || (n & 3) || (n > 0 && (!g || !y || !out))) return ag_fail(AG_ERR_ARG, "ag_relu_mask: n=%lld must be a non-negative multiple of 4, tensors non-null", (long long)n);
    ag_launch_relu_mask(g, y, out, n, static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

size_t ag_train_weight_grads_workspace_bytes(int64_t rows, int n_layers)
{
    return ag_weight_grads_ws_floats(rows, n_layers < 1 ? 1 : n_layers) * sizeof(float);
}

int ag_train_weight_grads(int n_layers, const float *const *dz, const int32_t *dz_ld, const float *const *prev, const int32_t *prev_ld, const int32_t *n_in,
                          int64_t rows, float *out, void *workspace, size_t workspace_bytes, ag_stream_t stream)
{
    return ag_train_weight_grads_into(n_layers, dz, dz_ld, prev, prev_ld, n_in, rows, out, nullptr, nullptr, nullptr, nullptr, workspace, workspace_bytes,
                                      stream);
}

int ag_train_weight_grads_into(int n_layers, const float *const *dz, const int32_t *dz_ld, const float *const *prev, const int32_t *prev_ld,
                               const int32_t *n_in, int64_t rows, float *out, float *const *w_grad, const int32_t *w_grad_ld, float *const *b_grad,
                               const int32_t *n_out, void *workspace, size_t workspace_bytes, ag_stream_t stream)
{
    if (n_layers < 1 || n_layers > 4 || !dz || !dz_ld || !prev || !prev_ld || !n_in || rows < 0) return ag_fail(AG_ERR_ARG, "ag_train_weight_grads: bad argument");
    if (!w_grad && !out) return ag_fail(AG_ERR_ARG, "ag_train_weight_grads: no destination");
    for (int l = 0; l < n_layers; ++l) {
        if (!dz[l] || !prev[l] || n_in[l] < 1 || n_in[l] > AG_F || prev_ld[l] < n_in[l] || dz_ld[l] < 1 || dz_ld[l] > AG_FP)
            return ag_fail(AG_ERR_ARG, "ag_train_weight_grads: layer %d: null table or n_in=%d ld=%d", l, n_in[l], prev_ld[l]);
        if (w_grad && (!w_grad_ld || !n_out || (w_grad[l] && (n_out[l] < 1 || n_out[l] > AG_FP || w_grad_ld[l] < n_in[l]))))
            return ag_fail(AG_ERR_ARG, "ag_train_weight_grads_into: layer %d: bad destination", l);
        if (w_grad && !w_grad[l] && !out) return ag_fail(AG_ERR_ARG, "ag_train_weight_grads_into: layer %d has no destination", l);
    }
    if (!workspace || workspace_bytes < ag_train_weight_grads_workspace_bytes(rows, n_layers))
        return ag_fail(AG_ERR_WS, "ag_train_weight_grads: workspace %zu < %zu bytes", workspace_bytes, ag_train_weight_grads_workspace_bytes(rows, n_layers));
    ag_launch_weight_grads(n_layers, dz, dz_ld, prev, prev_ld, n_in, rows, static_cast<float *>(workspace), out, w_grad, w_grad_ld, b_grad, n_out,
                           static_cast<hipStream_t>(stream));
    AG_HIP(hipGetLastError());
    return AG_OK;
}

}  // extern "C"
