// ag_host.h — what more than one host unit of the C ABI needs: the error return, the workspace carver, the model, and the engine's
// cross-unit functions.  ag_model.hip (model, options), ag_engine.hip (layouts, kernel sequencing), ag_drivers.hip (rollouts), ag_ops.hip (operators).
#pragma once
#include "../../include/adaptigraph_hip.h"
#include "ag_common.h"

#include <utility>
#include <vector>

int ag_fail(int code, const char *fmt, ...);      // records the text ag_last_error returns (per thread) and returns `code`  (ag_model.hip)

#define AG_HIP(x)                                                                                    \
    do {                                                                                             \
        hipError_t e_ = (x);                                                                         \
        if (e_ != hipSuccess) return ag_fail(AG_ERR_HIP, "%s: %s", #x, hipGetErrorString(e_));       \
    } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Carver {   // bump allocator over the caller's workspace, 256-byte aligned
    char *base;
    size_t off = 0, cap;
    Carver(void *p, size_t c) : base(static_cast<char *>(p)), cap(c) {}
    template <class T> T *take(size_t n)
    {
        off = align_up(off, 256);
        T *r = reinterpret_cast<T *>(base + off);
        off += n * sizeof(T);
        return r;
    }
    bool ok() const { return off <= cap && (base != nullptr || off == 0); }
};

#define AG_MAX_PARTS 4      // batch parts (streams) of a rollout
struct ag_model {
    ag_model_config cfg;
    float *dev = nullptr;       // all packed streams, one allocation
    size_t dev_floats = 0;
    AgWeights w{};
    // optional profiling (ag_profile_enable): event pairs per kernel class, recorded on the caller's stream
    // engine options (kOptions in ag_model.hip, their meaning include/adaptigraph_hip.h; max_blocks is set from the device's CU count), cu_split further
    // down; resolve_path turns them into a call's kernels
    int split = 0, fuse_agg = 0, precision = 2, max_blocks = 512, edge_products = 2, edge_ws = 1, node_ws = 1, agg_q16 = 1, node_dedup = 1, self_edges = 1,
        shared_state = 0;
    bool h2_ok = true;          // every edge-stack weight fits fp16 (else mode 2 keeps the split-bf16 edge stack)
    hipStream_t aux_stream[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[4] = {nullptr, nullptr, nullptr, nullptr};
    // CU partitioning of the rollout (env AG_CU_SPLIT / "cu_split"): the first `cu_split` CU-mask bits — cu_split / 8 CUs of EVERY
    // XCD (tools/ubench/cu_mask_map.hip: bit b = CU slot b / 8 of XCD b % 8) — run the MFMA-bound edge encoder, the other CUs the HBM-bound
    // edge build / segment reduce / node update / state step, the batch parts pipelined through the two partitions.  0 = off.
    int cu_split = 0;
    int n_cus = 256;
    int part_cus = 0;           // cu_split the two masked streams below were created for
    hipStream_t mfma_stream = nullptr, hbm_stream = nullptr;
    hipEvent_t ev_ready[4] = {nullptr, nullptr, nullptr, nullptr}, ev_enc[4] = {nullptr, nullptr, nullptr, nullptr}, ev_join_mfma = nullptr;
    bool profiling = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[AG_K_COUNT];
    size_t ev_used[AG_K_COUNT] = {0, 0, 0, 0, 0, 0};
    unsigned long long *edge_counter = nullptr;
    int *status = nullptr;      // device word, sticky: bit 0 = a forward left the range of its arithmetic (fp16 activation overflow, non-finite values)
};

struct Timed {   // RAII: bracket one kernel launch with an event pair when profiling is on
    ag_model *m;
    int k;
    hipStream_t s;
    hipEvent_t stop = nullptr;
    Timed(ag_model *m_, int k_, hipStream_t s_) : m(m_), k(k_), s(s_)
    {
        if (!m->profiling) return;
        if (m->ev_used[k] == m->ev[k].size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
            m->ev[k].emplace_back(a, b);
        }
        auto &pr = m->ev[k][m->ev_used[k]++];
        (void)hipEventRecord(pr.first, s);
        stop = pr.second;
    }
    ~Timed() { if (stop) (void)hipEventRecord(stop, s); }
};

// ---- ag_engine.hip: a model step's layout, arguments and kernel sequence ----
void carve_forward(Carver &c, AgFwdArgs &a, int B, int N, int64_t e_cap, bool eterm16 = false, bool full_dedup = false);
void carve_edges(Carver &c, AgEdgeArgs &a);
void edge_caps(int N, int topk, int connect, int max_tools, int *cap0, int *cap);
void bind_forward(const ag_model *m, AgFwdArgs &f, int B, int N, int n_p, int n_inst, const float *state, const float *attrs, const float *action,
                  const float *p_instance, const float *phys, const int32_t *row_ptr, const int32_t *edge_recv, const int32_t *edge_send,
                  float *pred_pos, float *pred_motion);
AgPath resolve_path(const ag_model *m, int B, int N, int n_inst, int steps = 1, bool shared = false);
void setup_args(ag_model *m, AgFwdArgs &a, const AgPath &p, int max_blocks);
void run_node_encode(ag_model *m, AgFwdArgs &a, hipStream_t s);
void run_node_encode_fallback(ag_model *m, AgFwdArgs &a, hipStream_t s);
void run_edge_encode(ag_model *m, AgFwdArgs &a, const AgPath &path, hipStream_t s);
void run_propagate(ag_model *m, AgFwdArgs &a, const AgPath &path, hipStream_t s);
