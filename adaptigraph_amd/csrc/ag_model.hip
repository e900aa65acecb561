// ag_model.hip — the model object of the C ABI (include/adaptigraph_hip.h): create / update / destroy, the engine options, the status word,
// profiling, and the error text of every entry point.
#include "ag_host.h"
#include "ag_pack.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

static thread_local std::string g_err;

int ag_fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

namespace {

// The host image of the weight streams (ag_pack.hip) -> the model's one device allocation and its stream pointers
int pack_and_upload(ag_model *m, const float *const *t)
{
    const AgPackedWeights p = ag_pack_weights(m->cfg, t);
    if (!m->dev) {
        AG_HIP(hipMalloc(reinterpret_cast<void **>(&m->dev), p.image.size() * sizeof(float)));
        m->dev_floats = p.image.size();
    } else {
        // Re-packing a LIVE model: kernels still running on any stream (torch side streams are non-blocking, so the
        // null-stream copy below is not ordered against them) may be reading the old streams.  Weight updates are rare
        // (once per checkpoint / optimiser step evaluated through the engine): drain the device first.
        AG_HIP(hipDeviceSynchronize());
    }
    AG_HIP(hipMemcpy(m->dev, p.image.data(), p.image.size() * sizeof(float), hipMemcpyHostToDevice));
    m->h2_ok = p.h2_ok;      // fp16 edge stack (precision mode 2, PrecH3): only if every edge-stack weight and bias is representable in fp16
    auto at = [&](int b3, int k) { return reinterpret_cast<const float4 *>(m->dev + p.off[b3][k]); };
    m->w.node_encode = at(0, 0); m->w.edge_encode = at(0, 1); m->w.node_mid = at(0, 2); m->w.node_last = at(0, 3);
    m->w.node_encode_b3 = at(1, 0); m->w.edge_encode_b3 = at(1, 1); m->w.node_mid_b3 = at(1, 2); m->w.node_last_b3 = at(1, 3);
    m->w.edge_encode_h2 = reinterpret_cast<const float4 *>(m->dev + p.off_h2);
    m->w.edge_scale_h3 = reinterpret_cast<const uint32_t *>(m->dev + p.off_sc);
    return AG_OK;
}

// ---- engine options: one row each — the name of ag_set_option / ag_get_option, the environment variable ag_model_create reads, the field, and
// validate (the value to store, or -1: refused).  An environment value is validated exactly as ag_set_option validates it.
struct Option {
    const char *name, *env;
    int ag_model::*field;
    int (*accept)(const ag_model *m, int v);
    const char *takes;      // what `accept` takes (error messages)
};
int flag(const ag_model *, int v) { return v != 0; }
const Option kOptions[] = {
    {"rollout_streams", "AG_SPLIT", &ag_model::split, [](const ag_model *, int v) { return v >= 0 && v <= AG_MAX_PARTS ? v : -1; }, "0 (by the workload) or 1..4"},
    {"fuse_aggregate", "AG_FUSE_AGG", &ag_model::fuse_agg, [](const ag_model *, int v) { return v == 0 || v == 2 ? v : -1; }, "0 (separate launch) or 2 (reduce inside node_update)"},
    {"precision", "AG_PRECISION", &ag_model::precision, [](const ag_model *, int v) { return v >= 0 && v <= 2 ? v : -1; }, "0 (f32), 1 (bf16x3) or 2 (fast)"},
    {"max_blocks", "AG_MAX_BLOCKS", &ag_model::max_blocks, [](const ag_model *, int v) { return v >= 1 ? v : -1; }, "a positive workgroup count"},
    {"edge_products", "AG_EDGE_PRODUCTS", &ag_model::edge_products, [](const ag_model *, int v) { return v == 2 || v == 3 ? v : -1; }, "2 (fp16 edge stack) or 3 (split-bf16)"},
    {"edge_stationary", "AG_EDGE_WS", &ag_model::edge_ws, flag, "any integer (0 = off)"},
    {"node_stationary", "AG_NODE_WS", &ag_model::node_ws, flag, "any integer (0 = off)"},
    {"agg_q16", "AG_AGG_Q16", &ag_model::agg_q16, flag, "any integer (0 = off)"},
    {"node_dedup", "AG_NODE_DEDUP", &ag_model::node_dedup, [](const ag_model *, int v) { return v < 0 ? 0 : (v > 2 ? 2 : v); }, "any integer (clamped to 0..2)"},
    {"self_edges", "AG_SELF_EDGES", &ag_model::self_edges, flag, "any integer (0 = off)"},
    {"shared_state", "AG_SHARED_STATE", &ag_model::shared_state, flag, "any integer (0 = off)"},
    {"cu_split", "AG_CU_SPLIT", &ag_model::cu_split, [](const ag_model *m, int v) { return v == 0 || (v >= 8 && v <= m->n_cus - 8 && !(v & 7)) ? v : -1; },
     "0 (off) or a multiple of 8 in [8, #CUs - 8]"},
};

const Option *find_option(const char *name)
{
    for (const Option &o : kOptions)
        if (!strcmp(name, o.name)) return &o;
    return nullptr;
}

// ag_model_create: every option's environment variable, if set — an integer, or for AG_PRECISION also f32 / bf16x3 / fast
int load_env_options(ag_model *m)
{
    static const char *const kPrecisionNames[] = {"f32", "bf16x3", "fast"};
    for (const Option &o : kOptions) {
        const char *text = getenv(o.env);
        if (!text) continue;
        char *end = nullptr;
        long long v = strtoll(text, &end, 10);
        bool parsed = *text && !*end && v == (int)v;
        for (int i = 0; i < 3 && !parsed && o.field == &ag_model::precision; ++i)
            if (!strcmp(text, kPrecisionNames[i])) { v = i; parsed = true; }
        const int stored = parsed ? o.accept(m, (int)v) : -1;
        if (stored < 0) return ag_fail(AG_ERR_CONFIG, "%s=%s: %s takes %s", o.env, text, o.name, o.takes);
        m->*o.field = stored;
    }
    return AG_OK;
}

}  // namespace

extern "C" {

const char *ag_last_error(void) { return g_err.c_str(); }
int ag_version(void) { return 1; }

int ag_model_create(const ag_model_config *cfg, const float *const *weights, ag_model **out)
{
    if (!cfg || !weights || !out) return ag_fail(AG_ERR_ARG, "ag_model_create: null argument");
    // The kernels are compiled for the shipped model_config family (config/dynamics/{rope,granular,cloth}.yaml).
    if (cfg->nf != AG_F) return ag_fail(AG_ERR_CONFIG, "nf=%d unsupported (kernels built for %d)", cfg->nf, AG_F);
    if (cfg->n_his != AG_NHIS) return ag_fail(AG_ERR_CONFIG, "n_his=%d unsupported (built for %d)", cfg->n_his, AG_NHIS);
    if (cfg->attr_dim != AG_ATTR || cfg->action_dim != 3)
        return ag_fail(AG_ERR_CONFIG, "attr_dim=%d action_dim=%d unsupported", cfg->attr_dim, cfg->action_dim);
    if (cfg->phys_dim < 0 || cfg->attr_dim + cfg->phys_dim + cfg->action_dim >= AG_NODE_IN_MAX)
        return ag_fail(AG_ERR_CONFIG, "phys_dim=%d unsupported", cfg->phys_dim);
    if (cfg->pstep < 1) return ag_fail(AG_ERR_CONFIG, "pstep=%d unsupported", cfg->pstep);
    for (int i = 0; i < ag_pack::N_TENSORS; ++i)
        if (!weights[i]) return ag_fail(AG_ERR_ARG, "ag_model_create: weight %d is null", i);
    ag_model *m = new ag_model();
    m->cfg = *cfg;
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) {
        m->max_blocks = AG_MLP_WG_PER_CU * prop.multiProcessorCount;
        m->n_cus = prop.multiProcessorCount;
    }
    int rc = load_env_options(m);      // (after the CU count: "cu_split" is validated against it)
    if (rc != AG_OK) {
        delete m;
        return rc;
    }
    rc = pack_and_upload(m, weights);
    if (rc == AG_OK && (hipMalloc(reinterpret_cast<void **>(&m->status), sizeof(int)) != hipSuccess ||
                        hipMemset(m->status, 0, sizeof(int)) != hipSuccess))
        rc = ag_fail(AG_ERR_HIP, "ag_model_create: status word allocation failed");
    if (rc != AG_OK) {
        if (m->status) (void)hipFree(m->status);
        if (m->dev) (void)hipFree(m->dev);
        delete m;
        return rc;
    }
    *out = m;
    return AG_OK;
}

int ag_model_update_weights(ag_model *m, const float *const *weights)
{
    if (!m || !weights) return ag_fail(AG_ERR_ARG, "ag_model_update_weights: null argument");
    return pack_and_upload(m, weights);
}

int ag_model_destroy(ag_model *m)
{
    if (!m) return AG_OK;
    for (auto &v : m->ev)
        for (auto &pr : v) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    if (m->edge_counter) (void)hipFree(m->edge_counter);
    for (int k = 0; k < 4; ++k) {
        if (m->aux_stream[k]) (void)hipStreamDestroy(m->aux_stream[k]);
        if (m->ev_join[k]) (void)hipEventDestroy(m->ev_join[k]);
    }
    if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
    if (m->mfma_stream) (void)hipStreamDestroy(m->mfma_stream);
    if (m->hbm_stream) (void)hipStreamDestroy(m->hbm_stream);
    for (int k = 0; k < 4; ++k) {
        if (m->ev_ready[k]) (void)hipEventDestroy(m->ev_ready[k]);
        if (m->ev_enc[k]) (void)hipEventDestroy(m->ev_enc[k]);
    }
    if (m->ev_join_mfma) (void)hipEventDestroy(m->ev_join_mfma);
    if (m->status) (void)hipFree(m->status);
    if (m->dev) (void)hipFree(m->dev);
    delete m;
    return AG_OK;
}

int ag_set_option(ag_model *m, const char *name, int value)
{
    if (!m || !name) return ag_fail(AG_ERR_ARG, "ag_set_option: null argument");
    const Option *o = find_option(name);
    if (!o) return ag_fail(AG_ERR_ARG, "ag_set_option: unknown option '%s'", name);
    const int stored = o->accept(m, value);
    if (stored < 0) return ag_fail(AG_ERR_ARG, "ag_set_option: %s takes %s, not %d", name, o->takes, value);
    m->*o->field = stored;
    return AG_OK;
}

int ag_get_option(const ag_model *m, const char *name, int *value)
{
    if (!m || !name || !value) return ag_fail(AG_ERR_ARG, "ag_get_option: null argument");
    const Option *o = find_option(name);
    if (!o) return ag_fail(AG_ERR_ARG, "ag_get_option: unknown option '%s'", name);
    *value = m->*o->field;
    return AG_OK;
}

int ag_model_status(ag_model *m, int *flags, ag_stream_t stream)
{
    if (!m || !flags) return ag_fail(AG_ERR_ARG, "ag_model_status: null argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    AG_HIP(hipMemcpyAsync(flags, m->status, sizeof(int), hipMemcpyDeviceToHost, s));
    AG_HIP(hipMemsetAsync(m->status, 0, sizeof(int), s));
    AG_HIP(hipStreamSynchronize(s));
    return AG_OK;
}

int ag_profile_enable(ag_model *m, int enable)
{
    if (!m) return ag_fail(AG_ERR_ARG, "ag_profile_enable: null model");
    if (enable && !m->edge_counter) {
        AG_HIP(hipMalloc(reinterpret_cast<void **>(&m->edge_counter), sizeof(unsigned long long)));
    }
    if (enable) AG_HIP(hipMemset(m->edge_counter, 0, sizeof(unsigned long long)));
    for (auto &u : m->ev_used) u = 0;
    m->profiling = enable != 0;
    return AG_OK;
}

int ag_profile_read(ag_model *m, double *ms, int64_t *launches, int64_t *edges)
{
    if (!m || !ms || !launches || !edges) return ag_fail(AG_ERR_ARG, "ag_profile_read: null argument");
    for (int k = 0; k < AG_K_COUNT; ++k) {
        double tot = 0.0;
        for (size_t i = 0; i < m->ev_used[k]; ++i) {
            float t = 0.f;
            AG_HIP(hipEventSynchronize(m->ev[k][i].second));
            AG_HIP(hipEventElapsedTime(&t, m->ev[k][i].first, m->ev[k][i].second));
            tot += t;
        }
        ms[k] = tot;
        launches[k] = (int64_t)m->ev_used[k];
    }
    unsigned long long e = 0;
    if (m->edge_counter) AG_HIP(hipMemcpy(&e, m->edge_counter, sizeof e, hipMemcpyDeviceToHost));
    *edges = (int64_t)e;
    return AG_OK;
}

}  // extern "C"
