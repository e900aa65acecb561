/*
 * adaptigraph_hip.h — C ABI of libadaptigraph_hip.so, the MI355X (gfx950) engine for AdaptiGraph's
 * message-passing rollout hot path.
 *
 * The reference has no FFI/plugin layer: its boundary is a Python call surface.  Each
 * entry point below names the reference symbol it stands behind; INTEGRATION.md shows the ctypes stub a
 * reference maintainer would add.  Conventions:
 *   - every data pointer is a DEVICE pointer (tensor.data_ptr()) unless marked host; fp32 / int32 / uint8
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises the host
 *   - the caller owns all memory, including the scratch `workspace` sized by the *_workspace_bytes queries;
 *     the library allocates only the packed weights inside ag_model
 *   - return 0 on success, negative on error; ag_last_error() gives the message (thread-local)
 *   - one ag_model may be used from one host thread at a time; distinct models/streams may run concurrently
 *   - inputs are never mutated; outputs are fully overwritten
 */
#ifndef ADAPTIGRAPH_HIP_H
#define ADAPTIGRAPH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the functions declared between this push and the pop at the end of the
 * header are exported (tests/test_abi.py holds `nm -D` to that list). */
#pragma GCC visibility push(default)

typedef struct ag_model ag_model;
typedef void *ag_stream_t; /* hipStream_t */

enum { AG_VARIANT_SINGLE = 0, AG_VARIANT_BATCH = 1 };
enum { AG_HEIGHT_MIN = 0, AG_HEIGHT_MASKED_MEAN = 1 };

/* Derived from model_config / material_config / dataset_config exactly as DynamicsPredictor.__init__ does
 * (src/dynamics/gnn/model.py:63-126). */
typedef struct ag_model_config {
    int32_t nf;           /* nf_particle == nf_relation == nf_effect (150)                  model.py:79-81   */
    int32_t n_his;        /* dataset_config['n_his'] (4)                                    model.py:77      */
    int32_t attr_dim;     /* model_config['attr_dim'] == rel_attr_dim (2)                   model.py:98,110  */
    int32_t phys_dim;     /* #physics_params with use: True                                 model.py:91-94   */
    int32_t action_dim;   /* 3                                                              model.py:99      */
    int32_t pstep;        /* propagation steps (3)                                          model.py:278     */
    float motion_clamp;   /* 100                                                            model.py:85      */
} ag_model_config;

const char *ag_last_error(void);
int ag_version(void);

/* DynamicsPredictor.__init__ + load_state_dict (model.py:63-126; checkpoint layout SURVEY.md §8b):
 * `weights` = 22 HOST pointers to fp32 tensors in state_dict order
 *   particle_encoder.model.{0,2,4}.{weight,bias}, relation_encoder.model.{0,2,4}.{weight,bias},
 *   particle_propagator.linear.{weight,bias}, relation_propagator.linear.{weight,bias},
 *   non_rigid_predictor.linear_{0,1,2}.{weight,bias}           (nn.Linear weight = (out,in) row-major).
 * Packs them into MFMA-ready chunk streams on the current HIP device. */
int ag_model_create(const ag_model_config *cfg, const float *const *weights, ag_model **out);
int ag_model_update_weights(ag_model *m, const float *const *weights);
int ag_model_destroy(ag_model *m);

/* Engine knobs (all have sane defaults; used by bench.py for A/B passes).  ag_model_create also reads each from an environment variable, an integer
 * validated as here (AG_PRECISION also takes f32 / bf16x3 / fast); an invalid value makes it return AG_ERR_CONFIG:
 *   AG_SPLIT rollout_streams, AG_FUSE_AGG fuse_aggregate, AG_MAX_BLOCKS max_blocks, AG_EDGE_PRODUCTS edge_products, AG_EDGE_WS edge_stationary,
 *   AG_NODE_WS node_stationary, AG_NODE_DEDUP node_dedup, AG_SELF_EDGES self_edges, AG_SHARED_STATE shared_state, AG_AGG_Q16 agg_q16,
 *   AG_CU_SPLIT cu_split, AG_PRECISION precision.
 * Values outside an option's list are refused (AG_ERR_ARG), except that the 0/1 switches take any integer (non-zero = 1) and "node_dedup" clamps to 0..2.
 *   "rollout_streams"  0..4  ag_rollout runs the batch as this many independent parts on separate streams; 0 (default): the engine's choice by
 *                            workload, see ag_rollout_streams_for
 *   "fuse_aggregate"   0/2   segment reduce as its own HBM-streaming kernel (0, default) or inside node_update through an LDS stage
 *                            (2, precision 2 only, other modes keep the launch: no `agg` table; measured equal solo, -4 % in the two-stream rollout); bit-identical results
 *   "max_blocks"       n >= 1 persistent grid size (default 2 x #CUs): the workgroups of the streaming MLP kernels, n / 2 (at least one) of the
 *                            weight-stationary ones; a rollout part takes its share n / parts.  No kernel reduces across workgroups, so a row's
 *                            result does not depend on which workgroup computes it: bit-identical results for ANY value, down to one workgroup
 *                            walking every block (tests/test_persistent_trips.py)
 *   "edge_products"    2/3   precision 2 only: arithmetic of the EDGE stack: 2 = fp16 (default: split-fp16 weights x fp16 activations + an e5m2
 *                            residual byte per activation, three fp16 MFMAs per fp32 product; models whose edge weights exceed the fp16 range
 *                            keep 3), 3 = split-bf16 like precision 1
 *   "edge_stationary"  0/1   with edge_products 2: 1 = weight-stationary kernel (default: weights in registers, activations handed from wave
 *                            to wave through LDS), 0 = streaming kernel (weights through LDS per 128 edges); bit-identical results
 *   "node_stationary"  0/1   precision 1 / 2, rounds before the last: 1 = weight-stationary node update (default: one workgroup per CU keeps the three
 *                            layers' split-bf16 weights in registers, 32-row blocks pipelined through LDS), 0 = streaming kernel (weights through
 *                            LDS per 128 rows); bit-identical results
 *   "node_dedup"       0/1/2 particle_encoder / hoisted Pn / the first round's Hr, Hs computed once per DISTINCT [attrs | phys | action] row of a sample
 *                            (the node encoder sees no positions, model.py:168-195) and read through an index, once per ag_rollout call: 1 (default) =
 *                            where it pays (>= 32 768 node-rows x steps per call), 2 = always, 0 = never (once per node and model step).
 *                            Bit-identical results
 *   "self_edges"       0/1   ag_rollout (the engine's own edge builder): 1 (default) = a particle's self-loop (graph.py:68-75; its edge inputs are
 *                            [a_n, a_n, 0, 0 ...], model.py:228-253 with r = s, a function of the node's attribute pair only) is left out of the edge
 *                            encoder and of the per-edge table for the attribute classes (1, 0) and (0, 1) — every driver of the reference produces
 *                            nothing else — one table row per class is encoded instead and the segment reduce adds it at the self-loop's position
 *                            in the receiver's order (10 % / 17 % / 5 % fewer rows at rope-1k / cloth-4k / granular-2k); other attribute pairs keep
 *                            their self-loops as real edges.  0 = every edge through the pipeline.  Bit-identical results
 *   "shared_state"     0/1   ag_rollout: 1 = exploit that dynamics() rolls ONE cloud out under `B` sampled pushes (forward_dynamics.py:11-38;
 *                            config/planning/rope.yaml:39-42: 20 000 samples per planning step).  The trajectory of the cloud WITHOUT a tool (the caller's
 *                            sample 0 with its tool slots invalid) is rolled out once as an extra internal sample; per model step every sample's full edge
 *                            lists are still built, but the encoders and the propagation rounds run only over the rows whose result can differ from the
 *                            base's — nodes whose inputs or earlier predictions differ in any bit (tool slots always), rows whose edge list differs from
 *                            the base's, and their 3-hop closure (three propagation rounds) — and every other particle takes the base's prediction
 *                            (models with more than three rounds, pstep > 3, take the plain path).
 *                            Results equal the plain rollout bit for bit for ANY input (samples whose states differ from sample 0's are simply all
 *                            private); one stream, node de-duplication forced on, workspace of ag_rollout_workspace_bytes_for(model, ...) with the option
 *                            set.  0 (default) = every sample in full — what the headline benchmark is quoted on.  Not combined with
 *                            "fuse_aggregate" 2 / "cu_split" (those calls take the plain path)
 *   "agg_q16"          0/1   precision 2 with the defaults of "fuse_aggregate" / "node_stationary": 1 = the per-node sums of a propagation round (`agg`,
 *                            model.py:295) travel from the segment reduce to node_update as 16-bit block-scaled rows (the per-edge table's format, 320 B
 *                            instead of 640 B per node and round; default 1).  One more rounding per node and round: NOT bit-identical to 0 — measured
 *                            deviation and gain in docs/NEGATIVE_RESULTS.md R6.4; ignored where a kernel of the round does not read the format
 *   "cu_split"         0|8k  CU-partitioned rollout (off by default): the first `cu_split` CU-mask bits (cu_split / 8 CUs of every XCD) run the
 *                            MFMA-bound edge encoder, the other CUs the HBM-bound edge build / segment reduce / node update / state step, the batch
 *                            parts pipelined through the two partitions on two CU-masked queues (hipExtStreamCreateWithCUMask).  Bit-identical
 *                            results; measured NOT faster than sharing the chip (docs/NEGATIVE_RESULTS.md R5.1, profiles/r05_cu_split_sweep_rope.txt)
 *   "precision"        0/1/2 0 = exact fp32 MFMA; 1 = split-bf16 ("bf16x3": x = hi + lo, 3 bf16 MFMAs per product,
 *                            fp32 accumulate; 1e-6..8e-6 abs deviation from the reference forward, gate 1e-4);
 *                            2 (default) = mode 1 for the node-level stacks, the edge stack in fp16 with residual bytes ("edge_products" 2) and the
 *                            per-edge Eterm table in 16-bit block-scaled fixed point (q16: half the dominant HBM stream); the same deviation
 *                            class as mode 1 at any motion size (random sweeps, trained weights, actions up to +-0.5) */
int ag_set_option(ag_model *m, const char *name, int value);

/* The model's CURRENT value of an option of ag_set_option — whatever set it (default, AG_* environment at ag_model_create, ag_set_option):
 * what a caller that accounts for the engine's work (bench.py's roofline bytes) must ask instead of re-reading the environment.
 * No reference counterpart (the reference has no engine options). */
int ag_get_option(const ag_model *m, const char *name, int *value);

/* Sticky numeric status of a model, read-and-clear (synchronises `stream`): bit 0 (AG_STATUS_NONFINITE) = some forward on this
 * model left the range of its arithmetic.  In precision mode 2 that is (a) an activation of the fp16 edge stack beyond +-65504 — detected in
 * the epilogue that produces it, whatever later layers make of the inf — or (b) a non-finite value reaching the per-edge table or a message
 * sum; with finite inputs both mean a checkpoint with large activations: switch the model to precision 1 (fp32 range).  In every mode,
 * non-finite inputs raise it through the message sums.  The reference has no counterpart (fp32 throughout, model.py:283-295).
 * (Until r03 bit 1 flagged mode-2 forwards that predicted motions above 0.125, where that round's arithmetic could leave the 1e-4 gate; the
 * r04 arithmetic has no such range and the bit is never set.)
 * Bit 2 (AG_STATUS_ORDER, declared with ag_rollout_ragged): a ragged rollout was given a batch that is not in the promised order, or an output row
 * outside the batch. */
enum { AG_STATUS_NONFINITE = 1 };
int ag_model_status(ag_model *m, int *flags /*host*/, ag_stream_t stream);

/* Upper bound on the edge count the builder can emit: B*N*(min(N,topk) + (connect_tools_all ? max_tools : 0)). */
int64_t ag_edge_capacity(int B, int N, int topk, int connect_tools_all, int max_tools);
size_t ag_edges_workspace_bytes(int B, int N, int topk, int connect_tools_all, int max_tools);

/* construct_edges_from_states (variant SINGLE, src/dynamics/dataset/graph.py:38-89) and
 * construct_edges_from_states_batch (variant BATCH, graph.py:91-156) for B samples at once.
 *   pos (B,N,3) f32; mask, tool_mask (B,N) u8; thr_sq (B) f32 = squared radius rounded as the variant does
 *   (SINGLE: (float)((double)r*r), BATCH: (float)r*(float)r); topk <= 64; max_tools >= #tool slots per sample.
 * Out: row_ptr (B*N+1) i32 over global rows b*N+i (row_ptr[B*N] = total edges, stays on device),
 *      edge_recv / edge_send (e_cap) i32 GLOBAL node ids in the reference's (receiver, sender) order.
 * Equivalent dense outputs: Rr[b, e - row_ptr[b*N], edge_recv[e] - b*N] = 1 (graph.py:152-155). */
int ag_build_edges(const float *pos, const uint8_t *mask, const uint8_t *tool_mask, const float *thr_sq, int topk,
                   int connect_tools_all, int variant, int B, int N, int max_tools, int32_t *row_ptr,
                   int32_t *edge_recv, int32_t *edge_send, int64_t e_cap, void *workspace, size_t workspace_bytes,
                   ag_stream_t stream);

/* ---- the reference's dense relation matrices <-> the CSR adjacency, on the device, with no host synchronisation (safe to capture).
 *
 * ag_edges_from_dense: the input contract of DynamicsPredictor.forward (src/dynamics/model.py:129-160): Rr, Rs (B,E,N) fp32 one-hot, all-zero rows
 *   = padding (pad_torch / truncate_graph).  Row (b,e) is an edge iff Rr[b,e,:] and Rs[b,e,:] both hold a non-zero entry (a NaN counts as
 *   non-zero); its receiver / sender is the LOWEST index of one — for 0/1 entries what sum(-1) > 0 and argmax(-1) give, multi-hot rows
 *   included.  Other values are outside the contract but never lead to an out-of-range index (indices are positions, not values).
 *   Out, in the layout of ag_build_edges: row_ptr (B*N+1), row_ptr[B*N] = number of edges (stays on the device); edge_recv / edge_send of
 *   capacity B*E, GLOBAL node ids, sorted by receiver and STABLY: within one receiver in ascending e (the order the segment reduce adds in).
 *   Rr, Rs need 4-byte alignment only.  B*N and B*E must stay below 2^31.
 * ag_edges_to_dense: the outputs of construct_edges_from_states_batch (src/dynamics/dataset/graph.py:146-155), padded to E_out rows as
 *   pad_torch(Rr, max_nR) pads them (src/dynamics/utils.py): row e - row_ptr[b*N] of sample b is one-hot at edge_recv[e] - b*N (Rr) and
 *   edge_send[e] - b*N (Rs).  Rr, Rs (B,E_out,N) fp32 are written completely, zeros included.  A sample with more than E_out edges
 *   sets *overflow (device word) to 1 and its surplus edges are dropped; otherwise *overflow is set to 0.  Node ids read from the arrays are
 *   range-checked (an id outside its sample leaves the row zero); edge_recv / edge_send must hold row_ptr[B*N] entries. */
size_t ag_dense_edges_workspace_bytes(int B, int E, int N);
int ag_edges_from_dense(const float *Rr, const float *Rs, int B, int E, int N,
                        int32_t *row_ptr, int32_t *edge_recv, int32_t *edge_send /* capacity B*E */,
                        void *workspace, size_t workspace_bytes, ag_stream_t stream);
int ag_edges_to_dense(const int32_t *row_ptr, const int32_t *edge_recv, const int32_t *edge_send,
                      int B, int N, int E_out, float *Rr, float *Rs, int32_t *overflow, ag_stream_t stream);

/* Scratch sizes.  ag_*_workspace_bytes(...) holds for ANY model / option setting (per-edge table sized as fp32 rows);
 * ag_*_workspace_bytes_for(m, ...) is exact for model `m` as configured NOW — in precision mode 2 the per-edge table is 16-bit (q16) rows,
 * half the largest buffer: query right before the call (a call checks its own carving against workspace_bytes and fails with AG_ERR_WS,
 * never overruns).  The compact tables of the node-encoder de-duplication are bounded (8 shared rows per sample + ~B N / 16 private
 * rows): inputs with more distinct [attrs | phys | action] rows run through the per-node encoder, same bits.
 * Rollout, rope-1k x 256: 3.5 -> 2.1 GB (2.9 for any mode); the reference planner's 20 000 x 200: 56 -> 33 GB (46). */
size_t ag_forward_workspace_bytes(int B, int N, int64_t e_cap);
size_t ag_forward_workspace_bytes_for(const ag_model *m, int B, int N, int64_t e_cap);

/* DynamicsPredictor.forward (model.py:129-313) on a CSR adjacency instead of one-hot Rr/Rs.
 *   state (B,n_his,N,3), attrs (B,N,2), action (B,N,3), p_instance (B,n_p,n_instance), phys (B,phys_dim)
 *   (p_instance may be NULL when n_instance is 0, phys when phys_dim is 0: an empty tensor has no address; the same holds for the rollouts)
 *   row_ptr/edge_recv/edge_send as produced by ag_build_edges (edges sorted by receiver).
 * Out: pred_pos, pred_motion (B,n_p,3). */
int ag_forward(ag_model *m, const float *state, const float *attrs, const float *action, const float *p_instance,
               int n_instance, const float *phys, const int32_t *row_ptr, const int32_t *edge_recv,
               const int32_t *edge_send, int64_t e_cap, int B, int N, int n_p, float *pred_pos, float *pred_motion,
               void *workspace, size_t workspace_bytes, ag_stream_t stream);

/* Inner rollout loop of dynamics() / dynamics_masked() (src/planning/forward_dynamics.py:125-197 / :319-393):
 * edges -> forward -> record-on-repeat -> tool advance -> history shift -> edge rebuild, n_steps times,
 * with no host synchronisation. */
typedef struct ag_rollout_params {
    int32_t B, N, n_p;            /* samples, slots per sample (objects + tools), object slots                */
    int32_t n_instance;
    int32_t topk, connect_tools_all, max_tools;
    int32_t n_steps;              /* max(action_repeat), forward_dynamics.py:156                              */
    int32_t height_mode;          /* AG_HEIGHT_MIN (:163) or AG_HEIGHT_MASKED_MEAN (:359)                     */
    float gripper_raise;          /* 0.01 * sim_real_ratio if gripper_enable else 0 (:167-168)                */
} ag_rollout_params;

size_t ag_rollout_workspace_bytes(const ag_rollout_params *p);
size_t ag_rollout_workspace_bytes_for(const ag_model *m, const ag_rollout_params *p);
/* Number of batch parts (one HIP stream each) ag_rollout will use for these parameters: the "rollout_streams" option, or with its default 0 the engine's
 * choice by workload (one stream, two where the edge stack dominates: top-k >= 16), never more than B / 8. */
int ag_rollout_streams_for(const ag_model *m, const ag_rollout_params *p);

/*   state0 (B,n_his,N,3) initial history incl. tool slots; delta (B,N,3) per-step tool motion (graph["action"]);
 *   attrs (B,N,2); p_instance (B,n_p,n_instance); phys (B,phys_dim); mask/tool_mask (B,N) u8;
 *   obj_mask (B,n_p) u8 (only read in MASKED_MEAN mode, may be NULL otherwise); thr_sq (B);
 *   repeat (B) i32 = action_repeat.
 * Out: out_seq (B,n_p,3) = prediction of step repeat[b] (rows with repeat outside 1..n_steps are left untouched);
 *      state_final (B,n_his,N,3) optional (may be NULL). */
int ag_rollout(ag_model *m, const ag_rollout_params *p, const float *state0, const float *delta, const float *attrs,
               const float *p_instance, const float *phys, const uint8_t *mask, const uint8_t *tool_mask,
               const uint8_t *obj_mask, const float *thr_sq, const int32_t *repeat, float *out_seq,
               float *state_final, void *workspace, size_t workspace_bytes, ag_stream_t stream);

/* ---- scripted rollout: a cloud advanced under a RECORDED tool trajectory, every step's prediction recorded and its mean key-point error
 * against ground truth reduced on the device.  Replaces the step loop of the evaluation rollout, src/dynamics/rollout/rollout.py:62-93, with
 * the frame walk of src/dynamics/rollout/graph.py:373-399 resolved by the caller up front (which frames a rollout visits never depends on the
 * predictions): one call instead of a host round trip per step, no host synchronisation, no allocation, safe to capture — and the script
 * arrays are read at replay time, so a captured call follows whatever script they hold then.
 * Per step t = 0 .. T-1 (T = n_steps), on ONE stream: ag_build_edges(variant) on state[:, -1]; ag_forward on the current action; then
 *   pred_seq[b, t] = pred;   err[b, t] = sum_i obj_mask[b,i] ||pred[b,i] - gt[b,t,i]||_2 / max(sum_i obj_mask[b,i], 1)
 *   and, unless t = T-1:  state = [state[1:], [pred | tool_pos[b, t+1]]],  action = [0 (object rows) | tool_delta[b, t+1]].
 * The tool slots are the last N - n_p of a sample and are placed absolutely from the script (rollout.py:84: eef_kp from the recorded frames):
 * no last + delta, no tool-height rule.  pred_seq and state_final equal, bit for bit, a loop of ag_build_edges + ag_forward calls with the same
 * model options; the error sum is taken in one fixed order without atomics (two calls give the same bits; a sample without a valid point
 * gives exactly 0).  "precision" and the kernel-choice options are honoured as ag_forward honours them; "rollout_streams", "cu_split",
 * "shared_state", "self_edges" and the edge builder's riders belong to ag_rollout and do not apply.
 * Argument errors and a workspace below the query come back as codes before anything is launched. */
typedef struct ag_scripted_params {
    int32_t B, N, n_p, n_instance;
    int32_t topk, connect_tools_all, max_tools;
    int32_t variant;      /* AG_VARIANT_SINGLE | AG_VARIANT_BATCH: what ag_build_edges takes */
    int32_t n_steps;      /* T >= 1 */
} ag_scripted_params;
size_t ag_rollout_scripted_workspace_bytes_for(const ag_model *m, const ag_scripted_params *p);
int ag_rollout_scripted(ag_model *m, const ag_scripted_params *p,
                        const float *state0,      /* (B, n_his, N, 3) */
                        const float *action0,     /* (B, N, 3): the action of step 0 */
                        const float *tool_pos,    /* (B, T, N - n_p, 3): entries t = 1 .. T-1 are read, entry 0 never; NULL if none is read */
                        const float *tool_delta,  /* same shape, same rule */
                        const float *attrs, const float *p_instance, const float *phys,
                        const uint8_t *mask, const uint8_t *tool_mask, const float *thr_sq,
                        const float *gt,          /* (B, T, n_p, 3) or NULL */
                        const uint8_t *obj_mask,  /* (B, n_p) or NULL: all ones */
                        float *pred_seq,          /* (B, T, n_p, 3) or NULL */
                        float *err,               /* (B, T); given exactly when gt is */
                        float *state_final,       /* (B, n_his, N, 3) or NULL: the history the last step's forward read */
                        void *workspace, size_t workspace_bytes, ag_stream_t stream);

/* ---- ragged rollout: a sample is computed for exactly repeat[b] model steps.  ag_rollout runs every sample for n_steps = max(repeat) steps although
 * a sample's prediction is recorded at step repeat[b] only (forward_dynamics.py:160-161) and nothing reads its later state: with push lengths sampled
 * uniformly between the task limits (rope [5, 15), granular and cloth [2, 10)) a third or more of the sample-steps are discarded.  Graphs of a batch
 * never interact, so leaving them out changes no recorded bit.  One mechanism, for the plain and the shared-state driver: the batch is ORDERED by
 * non-increasing repeat, the samples still running at step s are then a prefix of the batch, and the host — which knows the prefix length of every
 * step — sizes every launch of step s for it.
 *
 * ag_rollout_order: the ordering contract, computed on the device in ONE launch (no scratch, no host synchronisation, no allocation; capturable):
 *   order[r]  (B) = the sample of rank r: sorted by repeat DESCENDING (negative values count as 0), ties by ASCENDING index — a stable sort,
 *             deterministic: two calls give the same words
 *   active[s] (AG_RAGGED_MAX_STEPS + 1) = #{b : repeat[b] >= s + 1} for s < AG_RAGGED_MAX_STEPS: the samples that run model step s + 1; the LAST word
 *             counts the samples with repeat > AG_RAGGED_MAX_STEPS (non-zero: the batch is not for ag_rollout_ragged)
 * Any B >= 1.  The number of model steps of the batch is the number of non-zero words among the first AG_RAGGED_MAX_STEPS.
 *
 * ag_rollout_ragged: ag_rollout on inputs the caller has gathered into that order (input row r = sample order[r] of the original batch; repeat too), and
 *   active_per_step (HOST, p->n_steps words, read when the call is enqueued) = active[0 .. n_steps): model step s (1-based) runs the edge builder, the
 *             forward and the state step for the samples [0, active_per_step[s - 1]) only.  Table bases and row numbers stay those of the whole batch;
 *             counts and grids shrink, so a running sample's rows are computed exactly as ag_rollout computes them: out_seq holds ag_rollout's bits
 *   out_index (device, B; may be NULL = the identity): sample b's row of out_seq and of state_final is out_index[b] — pass `order` and the results land in
 *             the original batch's rows.  Rows of samples with repeat outside 1..n_steps are left untouched, as by ag_rollout
 *   state_final[out_index[b]] = sample b's history right AFTER ITS OWN step repeat[b] (state0[b] for repeat[b] <= 0) — not the history after n_steps
 *             steps, which ag_rollout returns and this call never computes
 * One stream: "rollout_streams" and "cu_split" are ignored; "shared_state" applies as in ag_rollout (the base is input sample 0 without its tools and runs
 * every step); every other option as in ag_rollout.  Workspace: ag_rollout_workspace_bytes_for(m, p), the same carving.  No host synchronisation.
 * AG_ERR_ARG, before anything is launched: a null argument, n_steps > AG_RAGGED_MAX_STEPS, active_per_step not non-increasing, above B or below 0.
 * On the device: if repeat is not in non-increasing order, or an out_index[b] is outside [0, B), the model's sticky status gets AG_STATUS_ORDER
 * (ag_model_status) and a write to such a row is skipped; every index the call forms is bounded by B whatever repeat holds, so misuse gives undefined
 * VALUES, never an access out of bounds. */
enum { AG_RAGGED_MAX_STEPS = 1024 };
enum { AG_STATUS_ORDER = 4 };
int ag_rollout_order(const int32_t *repeat, int B, int32_t *order /*B*/, int32_t *active /*AG_RAGGED_MAX_STEPS + 1*/, ag_stream_t stream);
int ag_rollout_ragged(ag_model *m, const ag_rollout_params *p, const float *state0, const float *delta, const float *attrs,
                      const float *p_instance, const float *phys, const uint8_t *mask, const uint8_t *tool_mask,
                      const uint8_t *obj_mask, const float *thr_sq, const int32_t *repeat,
                      const int32_t *active_per_step /*host, p->n_steps*/, const int32_t *out_index /*device, B, may be NULL*/,
                      float *out_seq, float *state_final, void *workspace, size_t workspace_bytes, ag_stream_t stream);

/* chamfer(x, y) of src/planning/losses.py:4-10 — the MPPI error term:
 *   x (B,N,3) predicted particles, y (B,M,3) if y_batched else (1,M,3) target cloud  ->  out (B)
 *   out[b] = mean_m min_n ||x[b,n]-y[.,m]|| + mean_n min_m ||x[b,n]-y[.,m]||; N + M <= 12800. */
int ag_chamfer(const float *x, const float *y, int B, int N, int M, int y_batched, float *out, ag_stream_t stream);

/* mean_chamfer(state_pred, state_real, pred_mask, real_mask) of src/planning/losses.py:12-24 — the sys-id objective
 *  — for the whole batch in one launch: chamfer over the points whose mask byte is non-zero.
 *   x (B,N,3), x_mask (B,N) u8, y (B|1,M,3), y_mask (B|1,M) u8  ->  out (B); NaN where a side has no valid point. */
int ag_chamfer_masked(const float *x, const uint8_t *x_mask, const float *y, const uint8_t *y_mask, int B, int N, int M,
                      int y_batched, float *out, ag_stream_t stream);

/* chamfer with its nearest-neighbour indices: the forward of the differentiable chamfer of src/planning/losses.py:4-24 (the planner's error
 * term and the sys-id objective under autograd).  Arguments as ag_chamfer / ag_chamfer_masked: x_mask and y_mask are both given or both NULL;
 * N + M <= 12800.  out (B) is bit-identical to ag_chamfer (masks NULL) / ag_chamfer_masked on the same arguments.  Also writes, as int32:
 *   idx_x (B,N): for every particle the index of its nearest target point; idx_y (B,M): for every target point the index of its nearest particle.
 * Ties go to the lowest index; masked-out points (and points of a sample whose other side is empty) get -1. */
int ag_chamfer_fwd_idx(const float *x, const uint8_t *x_mask, const float *y, const uint8_t *y_mask, int B, int N, int M, int y_batched,
                       float *out, int32_t *idx_x, int32_t *idx_y, ag_stream_t stream);

/* Backward of ag_chamfer_fwd_idx for grad_out (B) = dL/dout, with the indices that call wrote (losses.py:4-24: the min picks one pair per point):
 *   gx[b,n] = g_b (u(x_n - y_{idx_x[n]}) / Nx + sum_{m: idx_y[m] = n} u(x_n - y_m) / My),   u(v) = v / ||v||, u(0) = 0,
 * Nx / My the masked-in counts; gy likewise with the roles swapped, computed only when gy is not NULL.  Masked-out points, and every point of a
 * sample with an empty side (value NaN), get zero.  No atomics: the scatter sums are gathers in ascending index order, bit-reproducible.
 *   gx (B,N,3).  gy: (B,M,3) for a batched y; for a broadcast y (y_batched == 0) also a (B,M,3) buffer, of which row 0 holds the gradient of
 *   the shared cloud on return (the per-sample rows summed in ascending b) and rows 1.. are scratch. */
int ag_chamfer_backward(const float *x, const uint8_t *x_mask, const float *y, const uint8_t *y_mask, const int32_t *idx_x, const int32_t *idx_y,
                        const float *grad_out, int B, int N, int M, int y_batched, float *gx, float *gy, ag_stream_t stream);

/* ---- chamfer for clouds of any size (src/planning/losses.py:4-10 has no size limit; src/planning/plan.py:139-146 hands it every point of a
 * goal .pcd file).  The entry points above keep both clouds of a sample in the LDS of one workgroup; these split a sample into query tiles
 * (one workgroup each) and stream the other cloud through LDS in chunks, so N and M may each be anything from 1 to 2^24 and a call with few
 * samples still fills the device.  Where both forms apply, every output is bit-identical to the resident form's. ---- */

/* The tile sizes, for callers and tests that want shapes on either side of them: query points per workgroup, points per LDS chunk. */
void ag_chamfer_tile_sizes(int *query_tile, int *other_chunk);

/* Scratch of ag_chamfer_tiled (one float per point of both clouds of every sample); 0 for sizes the call refuses. */
size_t ag_chamfer_tiled_workspace_bytes(int B, int N, int M);

/* chamfer(x, y) of src/planning/losses.py:4-10 and the masked form of losses.py:12-24 in one entry point: arguments and results as
 * ag_chamfer_fwd_idx, except that x_mask / y_mask are both given or both NULL, idx_x / idx_y are both given or both NULL (NULL: the value only),
 * and 1 <= N, M <= 2^24.  ws: at least ag_chamfer_tiled_workspace_bytes(B, N, M) bytes (AG_ERR_WS otherwise), 4-byte aligned, free for reuse
 * once the stream has passed the call.  No host synchronisation, no memset: the call can be captured in a HIP graph. */
int ag_chamfer_tiled(const float *x, const uint8_t *x_mask, const float *y, const uint8_t *y_mask, int B, int N, int M, int y_batched, float *out,
                     int32_t *idx_x, int32_t *idx_y, void *ws, size_t ws_bytes, ag_stream_t stream);

/* Backward of ag_chamfer_tiled (losses.py:4-24 under autograd) with the indices that call wrote: arguments, formulas, the gy buffer of a
 * broadcast y and the results as ag_chamfer_backward, bit for bit where that applies; 1 <= N, M <= 2^24.  No atomics, no scratch. */
int ag_chamfer_tiled_backward(const float *x, const uint8_t *x_mask, const float *y, const uint8_t *y_mask, const int32_t *idx_x,
                              const int32_t *idx_y, const float *grad_out, int B, int N, int M, int y_batched, float *gx, float *gy,
                              ag_stream_t stream);

/* ---- the training losses of src/dynamics/gnn/loss.py that need no particle correspondence between prediction and label ---- */

/* Points a side of ag_emd (one wave per sample keeps the column side in registers): the largest size whose worst case stays well under a second
 * per launch on a shared device. */
#define AG_EMD_MAX_POINTS 1024

/* EarthMoverLoss.em_distance of src/dynamics/gnn/loss.py:29-55 without its host round trip (the (B,N,M) distance tensor of :32-34, the copy and
 * scipy.optimize.linear_sum_assignment per sample of :39-42, the gather of :46-51): the exact minimum-cost assignment of two clouds, one launch.
 *   x (B,N,3), y (B,M,3) if y_batched else (1,M,3); x_mask (B,N) / y_mask (B|1,M) u8, both given or both NULL; 1 <= N, M <= AG_EMD_MAX_POINTS.
 *   cost of a pair: c[n,m] = sqrtf((dx dx + dy dy) + dz dz) in fp32, products rounded separately, widened to fp64.
 *   With Nx / My the valid counts and K = min(Nx, My): an injection of the smaller valid set into the larger that minimises the fp64 sum of c
 *   (shortest augmenting paths with fp64 duals: exact, and where several assignments are optimal always the same one).
 *   col (B,N) int32: the partner of x[b,n] in y, -1 for a masked or unmatched point; row (B,M) int32: the inverse.
 *   out (B): float(S / K), S the fp64 sum of the matched c in ascending n (loss.py:54 per sample when N == M and nothing is masked).
 * K == 0, or a NaN / +-Inf among a sample's valid coordinates: out = NaN and every index -1 for that sample alone.
 * No atomics, no scratch, no host read, no memset: bit-reproducible and capturable in a HIP graph. */
int ag_emd(const float *x, const uint8_t *x_mask, const float *y, const uint8_t *y_mask, int B, int N, int M, int y_batched, float *out,
           int32_t *col, int32_t *row, ag_stream_t stream);

/* Backward of ag_emd for grad_out (B) = dL/dout with the assignment that call wrote (autograd through the gather and norm of loss.py:46-54):
 *   gx[b,n] = g_b u(x_n - y_col[n]) / K if col[n] >= 0 else 0;  gy[b,m] = g_b u(y_m - x_row[m]) / K if row[m] >= 0 else 0;  u(v) = v / ||v||, u(0) = 0,
 * K the number of matched pairs.  gx (B,N,3); gy may be NULL; for a broadcast y it is a (B,M,3) buffer as in ag_chamfer_backward: row 0 holds the
 * per-sample rows summed in ascending b on return.  Gather form, no atomics. */
int ag_emd_backward(const float *x, const float *y, const int32_t *col, const int32_t *row, const float *grad_out, int B, int N, int M, int y_batched,
                    float *gx, float *gy, ag_stream_t stream);

/* The per-sample directed maxima of HausdorffLoss.hausdorff_distance, src/dynamics/gnn/loss.py:70-75 (which then takes the maxima over the batch):
 * clouds and masks as ag_emd, sizes as ag_chamfer (N + M <= 12800).
 *   out (B,2) = [max_n min_m c, max_m min_n c] over the valid points, c as in ag_emd: max, min and sqrtf are exact, so these are the formula's bits.
 *   arg (B,4) int32 = n*, its nearest m, m*, its nearest n; ties go to the lowest index.  An empty side: NaN and -1. */
int ag_hausdorff(const float *x, const uint8_t *x_mask, const float *y, const uint8_t *y_mask, int B, int N, int M, int y_batched, float *out,
                 int32_t *arg, ag_stream_t stream);

/* ---- the planner's trajectory cost ("MPPI glue on device"): everything of running_cost, src/planning/plan.py:27-59, but the
 * error term's own kernel — the penalties rope_penalty / cloth_penalty / granular_penalty and box_loss of src/planning/losses.py:26-92, the
 * workspace-bounds term of plan.py:41-51 and the reward of plan.py:37 and 53 — in two launches that read every predicted cloud once.
 *   state_seqs (B, L, n, 3), action (B, L, 4) = (x_start, z_start, theta, length), state_init (n, 3), error_in (B*L) or NULL, all fp32.
 * Per cloud (b, l), in the x-z plane, every product and sum rounded separately, d(p, q) the distance of two points:
 *   extents    xlo, xhi, zlo, zhi = min / max over the n particles
 *   error      AG_ERROR_GIVEN: error_in[b L + l].  AG_ERROR_BOX: box_loss(state_seqs[b, l], box) = the mean over the particles (ascending
 *              per lane, then a butterfly: one fixed order) of sqrt(dx dx + dz dz), dx = max(box xmin - x, 0) + max(x - box xmax, 0)
 *   nearest    the particles of the cloud BEFORE push l (state_init for l = 0, state_seqs[b, l - 1] after; cloth: always state_init) against
 *              rope / cloth: the start point of action (b, l); granular: the nine points start + off (r sin theta, -r cos theta),
 *              off = -1, -0.75 ... 1, r = 0.05 sim_real_ratio.  The square root of the smallest squared distance (= the smallest distance)
 *   farthest   cloth: the largest such distance; else 0
 *   collision  rope, granular: exp(-100 max(nearest - 0.02 ratio, 0));  none: 0
 *              cloth: 1 - exp(-100 max(nearest - 0.005 ratio, 0)) - 0.2 f / max over all (b, l) of f,  f = min(farthest, 0.4 ratio)
 *   box        the largest of exp(-100 max(margin, 0)) over the margins xlo - bbox xmin, bbox xmax - xhi, zlo - bbox zmin, bbox zmax - zhi
 * and per sample, evaluated left to right, the means as ascending-l sums divided by L:
 *   reward[b] = -(2 / (max over all (b, l) of error + 1e-6)) error[b, L - 1] - 5 mean_l collision - 5 mean_l box.
 * A NaN goes where the reference's tensor ops carry it (min, max, mean and clamp propagate NaN there): a NaN x or z coordinate makes the
 * cloud's extents, box term, box_loss and the next push's nearest distance NaN, and a NaN error makes every reward NaN.  y is not read.
 * terms: NULL, or (B, L, AG_PLAN_TERMS): error, collision, box, nearest, farthest, xlo, xhi, zlo, zhi of every (b, l).
 * ws: ag_plan_cost_workspace_bytes(p) bytes (AG_ERR_WS otherwise), 4-byte aligned; holds the per-(b, l) terms of a call without `terms`; every
 * word is written before it is read.  No host synchronisation, no memset, no atomics: the call can be captured in a HIP graph and returns the
 * same bits every time. ---- */
enum { AG_PENALTY_NONE = 0, AG_PENALTY_ROPE = 1, AG_PENALTY_CLOTH = 2, AG_PENALTY_GRANULAR = 3 };
enum { AG_ERROR_GIVEN = 0, AG_ERROR_BOX = 1 };
#define AG_PLAN_TERMS 9
typedef struct ag_plan_cost_params {
    int B, L, n;
    int penalty;      /* AG_PENALTY_NONE / _ROPE / _CLOTH / _GRANULAR */
    int criterion;    /* AG_ERROR_GIVEN: error_in (B*L) is the error term (e.g. from ag_chamfer); AG_ERROR_BOX: box_loss against box[] */
    float sim_real_ratio;
    float bbox[4];    /* xmin, xmax, zmin, zmax of the workspace */
    float box[4];     /* target box of AG_ERROR_BOX */
} ag_plan_cost_params;

/* Scratch of ag_plan_cost: AG_PLAN_TERMS floats per (b, l), whatever n; 0 for parameters the call refuses. */
size_t ag_plan_cost_workspace_bytes(const ag_plan_cost_params *p);
int ag_plan_cost(const ag_plan_cost_params *p, const float *state_seqs, const float *action, const float *state_init,
                 const float *error_in, float *reward, float *terms, void *ws, size_t ws_bytes, ag_stream_t stream);

/* ---- a planning step of the reference's chunks in one pass: src/planning/plan.py:180-247 splits n_sample into n_chunk chunks of n_sample_chunk
 * samples and runs one Planner.trajectory_optimization (src/planning/real_world/planner.py:234-277) per chunk, each with its own cost
 * normalisers, softmax update and best sample, and merge_res (planner.py:312-323) keeps the best chunk.  The two calls below score and update
 * all chunks of one rollout of n_chunk S samples, chunk c being samples [c S, (c + 1) S).
 *
 * ag_plan_cost_chunked: ag_plan_cost with p->B = n_chunk S (S >= 1; AG_ERR_ARG otherwise), except that "max over all (b, l)" of the error and
 * of cloth's f is taken over the (b, l) of the sample's own chunk (plan.py:37 and losses.py:61 inside one chunk's call): reward[c S .. (c + 1) S)
 * holds the bits of ag_plan_cost on that slice of the inputs alone, a NaN error makes the rewards of its chunk NaN and of no other, and
 * n_chunk = 1 is ag_plan_cost.  Same terms table, same workspace (ag_plan_cost_workspace_bytes(p)), same two launches, the second with one
 * workgroup per chunk.  No host synchronisation, no memset, no atomics. ---- */
int ag_plan_cost_chunked(const ag_plan_cost_params *p, int n_chunk, const float *state_seqs, const float *action, const float *state_init,
                         const float *error_in, float *reward, float *terms, void *ws, size_t ws_bytes, ag_stream_t stream);

/* optimize_action_mppi and clip_actions of src/planning/plan_utils.py:31-39 and 80-101 for every chunk, and the arg-max of planner.py:259-265, in one
 * launch of one workgroup per chunk.  actions (n_chunk S, L, 4) = (x, z, theta, length), reward (n_chunk S), fp32.  Per chunk, every product and
 * sum rounded separately and every reduction in one fixed order (the same bits on every call):
 *   w = softmax(reward reward_weight) over the chunk's S samples, the largest exponent subtracted; S = 1 gives the weight 1 exactly
 *   per look-ahead index l the sums over the samples of w x, w z, w x_end, w z_end,
 *     x_end = x - (length push_length) cos theta,  z_end = z - (length push_length) sin theta
 *   theta' = atan2(z - z_end, x - x_end) of the sums, wrapped by ((theta' + pi) mod 2 pi) - pi with the divisor's sign (pi as a float)
 *   length' = sqrt(dx dx + dz dz) / push_length,  (dx, dz) = the summed end minus the summed start
 *   new_seq[c, l] = (x, z, theta', length') clamped to [lo, hi] per field: min with hi, then max with lo, a NaN kept
 *   best_idx[c] = the index inside the chunk of its largest reward: the lowest index on ties, and a NaN reward counts as the largest, the first
 *     NaN winning (torch.argmax, np.argmax); best_seq[c] = that sample's (L, 4) rows, best_reward[c] = its reward, both copied bit for bit
 * A NaN reward makes new_seq of its chunk NaN and of no other.  Out: new_seq (n_chunk, L, 4), best_idx (n_chunk) int32, best_seq (n_chunk, L, 4),
 * best_reward (n_chunk); any of them may be NULL.  n_chunk, S, L >= 1 and n_chunk S L <= 2^30 (AG_ERR_ARG otherwise).  No scratch, no host
 * synchronisation, no atomics: capturable in a HIP graph. */
typedef struct ag_mppi_params {
    int n_chunk, S, L;
    float reward_weight, push_length;
    float lo[4], hi[4];    /* action limits per field (x, z, theta, length) */
} ag_mppi_params;
int ag_mppi_update(const ag_mppi_params *p, const float *actions, const float *reward, float *new_seq, int32_t *best_idx, float *best_seq,
                   float *best_reward, ag_stream_t stream);

/* ---- farthest-point key-point sampling (SURVEY.md §8f row n3 data side): the two passes of fps() of src/dynamics/dataset/graph.py:8-36 — the
 * first is dgl.geometry.farthest_point_sampler, the second fps_rad_idx of src/dynamics/utils.py:10-24 — and with them the perception step of
 * the closed loop, src/planning/perception.py:266-279.  B clouds in one launch, one workgroup per cloud.
 *   pts (B,N,3) fp32; count (B) = number of valid LEADING points of each cloud, or NULL (all N); start (B) = index of the first pick.
 * Per cloud: pick start[b]; keep for every point the distance to its nearest pick; the next pick is the arg-max of the kept distances, the
 * LOWEST index on ties; stop after K picks, after count[b] picks, or — radius not NULL — as soon as the largest kept distance is <= radius[b]
 * (the float32 distance compared with the double as doubles).  A cloud with count[b] < 1 or start[b] outside [0, count[b]) gets no pick.
 * `metric` fixes the arithmetic (ties follow it), fp32 with every product and sum rounded separately, d = p - pick:
 *   AG_FPS_SQUARED  (d0 d0 + d1 d1) + d2 d2                                   (farthest_point_sampler; radius must be NULL)
 *   AG_FPS_NORM     the correctly rounded square root of that, per point      (fps_rad_idx: np.linalg.norm)
 * Out: idx (B,K) int32 picks in order, -1 past the cloud's last pick; n_out (B) picks made.
 * Clouds of up to AG_FPS_RESIDENT_POINTS points are held in registers for the whole call; larger ones stream the points from global memory
 * and keep the distances in `workspace` (ag_fps_workspace_bytes(B, N), asked of every call): there is no size limit.  Inputs are assumed
 * finite (a NaN or infinite coordinate gives unspecified picks, never an out-of-range index).  No host synchronisation: safe to capture. */
enum { AG_FPS_SQUARED = 0, AG_FPS_NORM = 1 };
#define AG_FPS_RESIDENT_POINTS 8192
size_t ag_fps_workspace_bytes(int B, int N);
int ag_fps(const float *pts, const int32_t *count, const int32_t *start, int B, int N, int K, int metric, const double *radius,
           int32_t *idx, int32_t *n_out, void *workspace, size_t workspace_bytes, ag_stream_t stream);

/* ---- the tabletop cloud from depth images (src/planning/perception.py:151-256, the geometry in front of get_state_cur): un-project + board
 * frame + crop, voxel merge, the statistical outlier filter and the height filter, each ending in one ORDERED compaction (input order, no
 * atomics decide a position).  The arithmetic is restated in adaptigraph_amd/perception.py (the host statement; the open3d details it lists
 * were written down from memory) and repeated here operation for operation: float64 on float32 inputs, products and sums rounded separately.
 * A cloud is pts (n_max, 3) fp32 plus a DEVICE count (its first *count rows are valid; launches are sized by n_max >= *count); 1 <= n_max <=
 * AG_TABLETOP_MAX_POINTS, larger clouds are refused (AG_ERR_ARG).  Every call takes ag_tabletop_workspace_bytes(n_max) bytes of scratch
 * (AG_ERR_WS otherwise; 0 = n_max out of range), free for reuse after the call's launches.  Output clouds have n_max rows and must not alias
 * the input.  No host synchronisation, counts are device words written by kernels: safe to capture.
 *
 * ag_depth_cloud: depth (C,H,W) fp32, mask (C,H,W) bytes or NULL, cams (C,21) doubles = Kinv (3x3 row-major, the inverse intrinsics computed by
 *   the caller), R (3x3), t (3); limits (8) doubles = depth lo, hi, then the box as min, max per axis.  Pixels (v, u) = (0, stride, ...): kept iff
 *   lo < d < hi (the float widened to double), the mask byte is non-zero and the board-frame point lies in the box (inclusive; a NaN fails);
 *   a = u d, b = v d, p_cam_r = (Kinv[r,0] a + Kinv[r,1] b) + Kinv[r,2] d, p_r = ((R[r,0] p_cam_0 + R[r,1] p_cam_1) + R[r,2] p_cam_2) + t_r, stored
 *   as fp32, camera-major then row-major.  pts has C ceil(H/stride) ceil(W/stride) rows (that product is the call's n_max).
 * ag_cloud_voxel_keys / ag_cloud_voxel_merge: keys[i] = the packed voxel key of point i, floor((p - origin) / voxel) per axis with origin =
 *   min - 0.5 voxel (AG_TABLETOP_VOXEL_KEY_LIMIT keys per axis; *status = 1 if the cloud is wider), INT64_MAX behind the count.  The caller sorts
 *   the keys STABLY (sorted_keys, perm = the source positions, int64); merge then writes one point per voxel — the sum of its members in
 *   ascending index / their number, as fp32 — ordered by lowest member index.  voxel_size is a HOST double.
 * ag_cloud_knn_mean: avg[i] = (sum of sqrt(d2) over the k' = min(k, *count) nearest points under the total order (d2, j), i itself included, in
 *   ascending order) / k', d2 = (dx dx + dy dy) + dz dz; 1 <= k <= AG_TABLETOP_MAX_NEIGHBORS.  Uniform grid, ring by ring; points still
 *   unresolved at the ring limit are finished by a brute-force pass.  info (2) = [points that took that pass, grid cells].
 * ag_cloud_outlier_filter: mean = (sum of the avg_i > 0) / n, std = sqrt(sum over avg_i > 0 of (avg_i - mean)^2 / (n - 1)), threshold = mean +
 *   *std_ratio std (a HOST double), sums in a fixed order; stats (3) = [mean, std, threshold]; keep[i] = 0 < avg_i < threshold (n <= 1: none);
 *   out = the kept points; count_out (2) = [their number, the same number bit-complemented (~) when nothing was removed].
 * ag_cloud_select: out = the points whose flags byte is non-zero, or — flags NULL — whose z is < *z_below (a device float); exactly one of them. */
#define AG_TABLETOP_MAX_POINTS (1 << 20)
#define AG_TABLETOP_MAX_NEIGHBORS 20
#define AG_TABLETOP_VOXEL_KEY_LIMIT (1 << 21)
size_t ag_tabletop_workspace_bytes(int n_max);
int ag_depth_cloud(const float *depth, const uint8_t *mask, const double *cams, const double *limits, int C, int H, int W, int stride, float *pts,
                   int32_t *count, void *workspace, size_t workspace_bytes, ag_stream_t stream);
int ag_cloud_voxel_keys(const float *pts, const int32_t *count, int n_max, const double *voxel_size, int64_t *keys, int32_t *status,
                        void *workspace, size_t workspace_bytes, ag_stream_t stream);
int ag_cloud_voxel_merge(const float *pts, const int32_t *count, int n_max, const int64_t *sorted_keys, const int64_t *perm, float *out,
                         int32_t *count_out, void *workspace, size_t workspace_bytes, ag_stream_t stream);
int ag_cloud_knn_mean(const float *pts, const int32_t *count, int n_max, int k, double *avg, int32_t *info, void *workspace,
                      size_t workspace_bytes, ag_stream_t stream);
int ag_cloud_outlier_filter(const float *pts, const int32_t *count, int n_max, const double *avg, const double *std_ratio, double *stats,
                            uint8_t *keep, float *out, int32_t *count_out, void *workspace, size_t workspace_bytes, ag_stream_t stream);
int ag_cloud_select(const float *pts, const int32_t *count, int n_max, const uint8_t *flags, const float *z_below, float *out, int32_t *count_out,
                    void *workspace, size_t workspace_bytes, ag_stream_t stream);

/* ---- rope push simulator (the data side; stands in for what src/sim/sim_env/flex_env.py:258-402 asks of its closed particle solver): ONE push
 * of E rope-on-table episodes in one launch, one 256-thread workgroup per episode, one particle per thread.  The model is this project's own
 *  and is stated operation for operation by adaptigraph_amd/sim.py:rope_push_host; the kernel gives the same bits.
 * Per-episode DEVICE arrays, (E) each: n particles in rope order (2 .. n_max), l0 rest spacing, w cluster width and kappa cluster gain (clusters
 * are skipped when w < 3 or w > n), n_push steps of the push (1 .. n_push_max), inv = float(1 / (n_push substeps)); push (E,4) = xs, zs, xe, ze.
 * State x, v (E,n_max,3) fp32, read and written in place (rows >= n untouched).  Per step `substeps` substeps of h seconds: predict under
 * gravity g, stretch (even pairs, then odd pairs), straight-segment shape matching, the cylindrical pusher of radius R against particles of radius
 * r (push steps only), the ground at height r, velocities with Coulomb friction mu on grounded particles; after the n_push steps `settle` steps
 * without the pusher.  Out: obj (E,F_max,n_max,3) and eef (E,F_max,3): frame f holds x and the pusher point (c.x, r, c.z) after push step
 * f record_every, the episode's last frame x after the settle with the pusher point (xe, r + lift, ze); n_frames (E) = (n_push - 1) /
 * record_every + 2 frames written, rows and frames behind them untouched.
 * AG_ERR_ARG, nothing launched: a null pointer, n_max outside 2 .. AG_SIM_ROPE_MAX_PARTICLES, F_max < (n_push_max - 1) / record_every + 2,
 * substeps or record_every < 1.  n_max and n_push_max are the host's bounds on the device arrays: an episode whose n or n_push lies outside
 * them writes n_frames = 0 and nothing else.  No host synchronisation, no atomics, the same bits on every call: safe to capture. */
#define AG_SIM_ROPE_MAX_PARTICLES 256
int ag_sim_rope_push(const int32_t *n, const float *l0, const int32_t *w, const float *kappa, const float *inv, const int32_t *n_push,
                     const float *push, float *x, float *v, float *obj, float *eef, int32_t *n_frames, int E, int n_max, int F_max,
                     int n_push_max, int substeps, int record_every, int settle, float h, float g, float r, float R, float mu, float lift,
                     ag_stream_t stream);

/* ---- granular push simulator (the data side for the granular material): ONE board push of E disc-pile episodes in one launch, one 256-thread
 * workgroup per episode, four grains per thread, contacts through a 64 x 64 cell grid in LDS that is rebuilt before every contact iteration.
 * The model is this project's own, stated operation for operation by adaptigraph_amd/sim.py:pile_push_host; the kernel gives
 * the same bits.  Per-episode DEVICE arrays, (E) each: n discs (1 .. n_max), rho their radius (0 < rho <= rho_max), n_push steps of the push
 * (1 .. n_push_max), inv = float(1 / (n_push substeps)); push (E,4) = xs, zs, xe, ze; lat (E,2) = the unit vector along the board (across the
 * push).  State x, v (E,n_max,3) fp32, read and written in place: components x and z of rows < n; y is carried, rows >= n are untouched.
 * Per step `substeps` substeps of h seconds: predict; `iters` Jacobi contact iterations between all discs nearer than 2 rho (integer sums of
 * the corrections scaled by 2^22, divided by the number of contacts); the board of half width W and half thickness T (push steps only), which
 * puts a disc nearer than rho + T to its segment at rho + T + slack from it; velocities with Coulomb friction mu under gravity g on every disc;
 * after the n_push steps `settle` steps without the board.  Out: obj (E,F_max,n_max,3) and eef (E,F_max,5,3): frame f holds x and the board's
 * key points c + (W o_k) lat, o = 1, -1, 0, 1/2, -1/2, at height tool_y after push step f record_every; the episode's last frame x after the
 * settle with the key points at the push end, at tool_y + lift; n_frames (E) = (n_push - 1) / record_every + 2, rows and frames behind untouched.
 * AG_ERR_ARG, nothing launched: a null pointer, n_max outside 1 .. AG_SIM_PILE_MAX_PARTICLES, F_max < (n_push_max - 1) / record_every + 2,
 * substeps, iters or record_every < 1, rho_max outside (0, 0.25] (the bound under which the integer sums cannot overflow).  n_max, n_push_max
 * and rho_max are the host's bounds on the device arrays: an episode whose n, n_push or rho lies outside them writes n_frames = 0 and nothing
 * else.  No host synchronisation, integer LDS atomics only, the same bits on every call: safe to capture. */
#define AG_SIM_PILE_MAX_PARTICLES 1024
int ag_sim_pile_push(const int32_t *n, const float *rho, const float *inv, const int32_t *n_push, const float *push, const float *lat, float *x,
                     float *v, float *obj, float *eef, int32_t *n_frames, int E, int n_max, int F_max, int n_push_max, int substeps, int iters,
                     int record_every, int settle, float h, float g, float mu, float W, float T, float slack, float tool_y, float lift,
                     float rho_max, ag_stream_t stream);

/* ---- cloth grasp-and-drag simulator (the data side for the cloth material): ONE grasp-and-drag of E mass-spring cloth episodes in one launch,
 * one 1024-thread workgroup per episode, four particles per thread, the predicted positions in LDS.  The model is this project's own (NOT
 * FleX, no self-collision), stated operation for operation by adaptigraph_amd/sim.py:cloth_push_host; the kernel gives the
 * same bits.  A cloth is a grid of nx x nz particles, i = iz nx + ix.  Per-episode DEVICE arrays: nx, nz (E) in 2 .. 64 with nx nz <= n_max;
 * rest (E,2) = l0, float(l0 sqrt 2); gains (E,4) = k_stretch, k_shear, k_bend, mu; steps (E,2) = n1, n2, the steps of the drag's two segments
 * (each >= 1, n1 + n2 <= n_push_max); inv (E,2) = float(1 / (n substeps)) of each; action (E,4) = xs, zs, xe, ze; lat (E,2) = the horizontal
 * unit vector across the drag.  State x, v (E,n_max,3) fp32, read and written in place (rows >= nx nz untouched).
 * The gripper moves from (xs, 0, zs) to (xe, lift, ze) in n1 steps, then down to (xe, 0, ze) in n2 steps (heights above the grasp height), then
 * lets go; `settle` steps follow.  The pick, on the x the call starts from: the up to AG_SIM_CLOTH_PICK_K particles of smallest
 * d2 = dx dx + dz dz to (xs, zs), equal d2 decided by the lower index, are grasped if the smallest d2 <= grasp2 (none otherwise); a grasped
 * particle keeps its offset from the gripper and is set to it every substep with inverse mass 0 until the release.
 * Per step `substeps` substeps of h seconds: predict under gravity g with v scaled by damp; the pins; `iters` sweeps of the distance
 * constraints -- stretch (ix, ix + 1), (iz, iz + 1) at l0, both diagonals of every cell at rest[1], bend (ix, ix + 2), (iz, iz + 2) at 2 l0 -- as
 * twelve conflict-free phases in place (coloured Gauss-Seidel; sim.py has the order), c = gain (len - rest) / (len (w_i + w_j)), skipped
 * when len == 0 or w_i + w_j == 0; the ground at height r; velocities with Coulomb friction mu on grounded, unpinned particles.
 * Out: obj (E,F_max,n_max,3) and eef (E,F_max,2,3): frame f holds x and the two finger points c +- finger lat at height tool_y + c.y after
 * step f record_every of the n1 + n2; the episode's last frame x after the settle with the finger points at (xe, lift, ze);
 * n_frames (E) = (n1 + n2 - 1) / record_every + 2, rows and frames behind untouched; picked (E,AG_SIM_CLOTH_PICK_K) the grasped particles in
 * the order of the pick, -1 where none.
 * AG_ERR_ARG, nothing launched: a null pointer, n_max outside 4 .. AG_SIM_CLOTH_MAX_PARTICLES, F_max < (n_push_max - 1) / record_every + 2,
 * substeps, iters or record_every < 1.  n_max and n_push_max are the host's bounds on the device arrays: an episode whose nx, nz or steps lie
 * outside them writes n_frames = 0 and nothing else.  No host synchronisation, no atomics, the same bits on every call: safe to capture. */
#define AG_SIM_CLOTH_MAX_PARTICLES 4096
#define AG_SIM_CLOTH_PICK_K 5
int ag_sim_cloth_push(const int32_t *nx, const int32_t *nz, const float *rest, const float *gains, const int32_t *steps, const float *inv,
                      const float *action, const float *lat, float *x, float *v, float *obj, float *eef, int32_t *n_frames, int32_t *picked,
                      int E, int n_max, int F_max, int n_push_max, int substeps, int iters, int record_every, int settle, float h, float g,
                      float r, float damp, float lift, float grasp2, float finger, float tool_y, ag_stream_t stream);

/* ---- box push simulator (the data side for the box material; stands in for src/sim/data_gen/data_gen_box.py over the 2-D rigid-body engine of
 * src/sim/sim_env/pymunk_env.py): ONE push of E rigid-box episodes in one launch, one 256-thread workgroup per episode, up to four particles
 * per thread.  The model is this project's own (NOT pymunk), stated operation for operation by
 * adaptigraph_amd/sim.py:box_push_host; the kernel gives the same bits.  A box is a rigid rectangle whose centre of mass is off its geometric
 * centre, sampled by n particles.  Per-episode DEVICE arrays: n (E) particles (4 .. n_max); q (E,n_max,2) their rest coordinates relative to
 * the centre of mass and m (E,n_max) their masses (0 <= m <= 1, sum 1), rows >= n never read; body (E,6) = the footprint x_lo, x_hi, z_lo,
 * z_hi relative to the centre of mass, the inertia I = sum m |q|^2 (> 0), rho_max >= max |q| (0 < rho_max <= 8); n_push steps of the push
 * (1 .. n_push_max), inv = float(1 / (n_push substeps)); push (E,4) = xs, zs, xe, ze.  State pose (E,4) = X, Z, co, si of the centre of mass
 * ((co, si) a unit vector) and vel (E,3) = VX, VZ, Omega, read and written in place.
 * Per step `substeps` substeps of h seconds: predict (the rotation in Cayley form, renormalised); `iters` rigid positional corrections against
 * the frictionless cylindrical pusher of radius R (push steps only; a pusher centre inside the footprint leaves through the nearest face; the
 * part of a penetration beyond `cap` moves the box and the pose the substep started from alike, so that no velocity comes of it);
 * velocities from the change of pose; Coulomb friction mu under gravity g of every particle on the table, implicit: k_i = m_i mu g /
 * max(|u_i|, eps), four sums over the particles (integers scaled by 2^22, exact in any order) and a 3 x 3 solve; at rest (exactly zero) once
 * |V| + |Omega| rho_max < v_rest.  After the n_push steps `settle` steps without the pusher.
 * Out: obj (E,F_max,n_max,3), eef (E,F_max,3) and pose_frames (E,F_max,4): frame f holds the particles (X + Rot q at height r), the pusher
 * point (c.x, r, c.z) and the pose after push step f record_every; the episode's last frame those after the settle with the pusher point
 * (xe, r + lift, ze); n_frames (E) = (n_push - 1) / record_every + 2, rows and frames behind untouched.
 * AG_ERR_ARG, nothing launched: a null pointer, n_max outside 4 .. AG_SIM_BOX_MAX_PARTICLES, F_max < (n_push_max - 1) / record_every + 2,
 * substeps, iters or record_every < 1, (mu g) / eps outside (0, 8192] (with rho_max <= 8 the bound under which the integer sums stay inside
 * 2^51).  n_max and n_push_max are the host's bounds on the device arrays: an episode whose n, n_push, inertia or rho_max lies outside the
 * bounds writes n_frames = 0 and nothing else.  No host synchronisation, no atomics, the same bits on every call: safe to capture. */
#define AG_SIM_BOX_MAX_PARTICLES 1024
int ag_sim_box_push(const int32_t *n, const float *q, const float *m, const float *body, const float *inv, const int32_t *n_push,
                    const float *push, float *pose, float *vel, float *obj, float *eef, float *pose_frames, int32_t *n_frames, int E, int n_max,
                    int F_max, int n_push_max, int substeps, int iters, int record_every, int settle, float h, float g, float mu, float r, float R,
                    float eps, float v_rest, float cap, float lift, ag_stream_t stream);

/* ---- simulated depth cameras (what the reference takes from its simulator's renderer, src/sim/sim_env/flex_env.py:151-189, :404-409): depth and
 * id images of E particle scenes from C calibrated pinhole cameras in ONE launch, every particle a sphere, the table a plane.  No tool (colour: ag_draw),
 * no sensor noise.  The arithmetic is stated by adaptigraph_amd/render.py:render_depth_host and repeated here operation for
 * operation -- float64 on float32 inputs, products and sums rounded separately, only + - * / sqrt -- so the kernel gives the statement's bits.
 * DEVICE arrays: pts (E,n_max,3) fp32 sphere centres in the cameras' world frame; n (E) int32 spheres per episode (an n outside 0 .. n_max renders
 * as 0; rows >= n are never read); radius (E) fp32; cams (C,25) doubles = Kinv (3x3 row-major, the inverse intrinsics computed by the caller),
 * R (3x3), t (3) with p_world = R p_cam + t as ag_depth_cloud reads them, then fx, fy, cx, cy of the pinhole (zero skew; they only bound a
 * sphere's pixels); plane (4) doubles (nx, ny, nz, o), the table nx x + ny y + nz z = o in the world frame, or NULL for none; limits (2) doubles =
 * near, far with 0 <= near < far.
 * Sphere i in camera c: d = float64(p) - t, c_r = (R[0,r] d_0 + R[1,r] d_1) + R[2,r] d_2, rr = float64(radius); it takes part iff c_2 - rr > near.
 * Pixel (u, v): qx = (Kinv[0,0] u + Kinv[0,1] v) + Kinv[0,2], qy from row 1, A = (qx qx + qy qy) + 1, B = (qx c_0 + qy c_1) + c_2,
 * Cc = ((c_0 c_0 + c_1 c_1) + c_2 c_2) - rr rr, disc = B B - A Cc; a hit iff disc >= 0, at d = (B - sqrt(disc)) / A, counted iff near < d < far.
 * Plane: w_r = (R[r,0] qx + R[r,1] qy) + R[r,2], den = (nx w_0 + ny w_1) + nz w_2, num = o - ((nx t_0 + ny t_1) + nz t_2); den != 0: dp = num / den,
 * counted iff near < dp < far.  The smallest double wins: spheres in ascending index with strict <, the plane only if strictly smaller than
 * every sphere hit.  Out: depth (E,C,H,W) fp32 = float(winner), 0 where nothing counts; id (E,C,H,W) int32 = the particle, -1 the plane, -2 nothing.
 * One 256-thread workgroup per (episode, camera, AG_RENDER_TILE x AG_RENDER_TILE pixels), the particles staged through LDS in chunks of
 * AG_RENDER_CHUNK and compacted in index order; every pixel written once.
 * AG_ERR_ARG, nothing launched: a null pts / n / radius / cams / limits / depth / id, E or C < 1, H or W outside 1 .. AG_RENDER_MAX_SIDE, n_max
 * outside 1 .. AG_RENDER_MAX_PARTICLES.  No host synchronisation, no atomics, the same bits on every call: safe to capture. */
#define AG_RENDER_TILE 32
#define AG_RENDER_CHUNK 256
#define AG_RENDER_MAX_SIDE 4096
#define AG_RENDER_MAX_PARTICLES 4096
int ag_render_depth(const float *pts, const int32_t *n, const float *radius, const double *cams, const double *plane, const double *limits, int E,
                    int n_max, int C, int H, int W, float *depth, int32_t *id, ag_stream_t stream);

/* ---- rollout and planning records drawn as images (what the reference draws with cv2: src/dynamics/rollout/graph.py:44-230 `visualize_graph`,
 * src/planning/plan_utils.py:104-300 `visualize_img`): F frames of H x W RGBA pixels from a display list -- discs and thick segments between
 * projected points, in paint order over a background -- in TWO launches.  The arithmetic is stated by
 * adaptigraph_amd/viz.py:draw_host and repeated here operation for operation, so the kernel gives the statement's bits.  Our coverage rule, not
 * cv2's Bresenham lines or its anti-aliasing; no text; spheres for particles (the background of mode 2 is ag_render_depth's id image).
 * DEVICE arrays: pts (n_pts,3) fp32 points in the cameras' world frame; prims (n_prim,4) int32 = point a, point b, style, 0; styles (n_style,4)
 * int32 = kind (0 disc about a, 1 segment a -> b), size (disc radius / segment width in pixels, 0 .. AG_DRAW_MAX_SIZE), layer (0 opaque,
 * 1 overlay), colour 0xRRGGBB; frames (F,4) int32 = camera, first primitive, primitive count, background index; cams (C,25) doubles as
 * ag_render_depth reads them; near (1) HOST double.  Background: mode 0 the colour color0; mode 1 bg = (n_bg,H,W,4) uint8 images (4-byte
 * aligned; the alpha byte is ignored); mode 2 bg = (n_bg,H,W) int32 id images and palette (n_pal) int32 colours: palette[id % n_pal] for
 * id >= 0, color0 for -1 (the table), color1 otherwise (nothing).  A background index outside 0 .. n_bg - 1 gives color0.
 * Point i in camera c: d = float64(p) - t, c_r = (R[0,r] d_0 + R[1,r] d_1) + R[2,r] d_2; valid iff c_2 > near; x = trunc(fx (c_0 / c_2) + cx),
 * y likewise; invalid if either is not finite or exceeds AG_DRAW_MAX_COORD in magnitude.  A primitive is dropped if a point or style index
 * is out of range (never dereferenced), its kind, size or layer is none of the above, or an endpoint it uses is invalid; a frame's range is
 * clipped to 0 .. n_prim and is empty for a camera outside 0 .. C - 1.
 * Coverage of pixel p, int64: disc (p - a)^2 <= size^2; segment with d = b - a, L2 = d.d, q = p - a, s = q.d, X = q_x d_y - q_y d_x:
 * L2 == 0 or s < 0: 4 |p - a|^2 <= size^2; s > L2: 4 |p - b|^2 <= size^2; otherwise 4 X^2 <= size^2 L2.
 * Paint: base = background; every covering layer-0 primitive in ascending index sets base; top = base; every covering layer-1 primitive in
 * ascending index sets top; per channel out = (top alpha + base (256 - alpha) + 128) >> 8, alpha in 0 .. 256; the alpha byte of out is 255.
 * Out: out (F,H,W,4) uint8.  scratch: ag_draw_scratch_bytes(n_pts, C) bytes, the projected points.
 * One 256-thread workgroup per (frame, AG_RENDER_TILE x AG_RENDER_TILE pixels), the primitives staged through LDS in chunks of AG_RENDER_CHUNK
 * and compacted in index order; every pixel written once.
 * AG_ERR_ARG, nothing launched: a null pts / prims / styles / frames / cams / near / scratch / out, F or C < 1, a negative count, H or W outside
 * 1 .. AG_RENDER_MAX_SIDE, alpha outside 0 .. 256, a mode outside 0 .. 2, a mode 1 or 2 without images, a mode 2 without a palette, a scratch
 * that is too small, F x tiles beyond one launch.  No host synchronisation, no atomics, no allocation: safe to capture. */
#define AG_DRAW_MAX_SIZE 64
#define AG_DRAW_MAX_COORD 16383
size_t ag_draw_scratch_bytes(int n_pts, int C);
int ag_draw(const float *pts, int n_pts, const int32_t *prims, int n_prim, const int32_t *styles, int n_style, const int32_t *frames, int F,
            const double *cams, int C, const double *near /*host*/, int H, int W, int alpha, int bg_mode, const void *bg, int n_bg,
            const int32_t *palette, int n_pal, int color0, int color1, void *scratch, size_t scratch_bytes, uint8_t *out, ag_stream_t stream);

/* ---- records as baseline JPEG scans (what the reference writes with cv2 and merges into videos: src/dynamics/rollout/graph.py:163-225,
 * rollout.py:194-203, src/planning/plan.py:328-339): the entropy-coded scans of F frames of H x W pixels in FIVE launches.  The
 * arithmetic is stated by adaptigraph_amd/jpeg.py:jpeg_scan_host, all integers, and repeated here operation for operation, so the call gives the
 * statement's bytes; the headers (SOI .. SOS), EOI and the AVI container of a Motion-JPEG video are host code there.  Not: mp4, inter-frame
 * coding, optimised or progressive Huffman tables.
 * DEVICE arrays: images (F,H,W,channels) uint8, channels 4 as ag_draw writes them (R, G, B, alpha; 4-byte aligned; alpha is ignored) or 3.
 * Colour: JFIF YCbCr in 16-bit fixed point, clamped to 0 .. 255.  subsampling AG_JPEG_444: an MCU is 8 x 8 pixels = the blocks Y, Cb, Cr;
 * AG_JPEG_420: 16 x 16 = Y00, Y01, Y10, Y11, Cb, Cr with chroma (a + b + c + d + 2) >> 2; the image is extended to whole MCUs by repeating its
 * last column and row.  Integer 8 x 8 DCT of sample - 128 in two matrix passes (13-bit coefficients; every intermediate inside int32), the Annex K
 * quantisation tables scaled by quality 1 .. 100 with the IJG rule, division to nearest and symmetric in sign, the four Annex K Huffman tables,
 * one restart interval every `restart` MCUs: the DC predictors reset, the segment is padded with 1-bits to a byte, every 0xFF byte is followed
 * by 0x00, RSTm (m mod 8) stands between segments and not after the last.
 * Out: out = the frames' scans back to back, offsets (F + 1) int64: frame f is out[offsets[f] .. offsets[f + 1]).
 * A segment is at most 2 * AG_JPEG_BLOCK_BYTES * blocks-per-MCU (3 or 6) * restart + 2 bytes = its SLOT (a block's bits, 11 + 11 of DC and
 * 63 * (16 + 10) of AC, are under AG_JPEG_BLOCK_BYTES bytes; stuffing at most doubles them; 2 for the marker).  With M = MCUs per frame,
 * S = ceil(M / restart) segments per frame and G = F S:  ag_jpeg_out_bytes = G * slot;  ag_jpeg_scratch_bytes = the sum, each part rounded up
 * to 256 bytes, of the coefficients (F M blocks-per-MCU * 64 int16), a slot per segment (G * slot), two int32 per segment (4 G + 4 G) and the
 * scan's sums (4 (G / 256 + 2)).  Both queries return 0 for arguments the call refuses.
 * One workgroup codes one segment, its unstuffed bits in LDS: AG_JPEG_MAX_RESTART * 6 * AG_JPEG_BLOCK_BYTES = 19 968 bytes.
 * AG_ERR_ARG, nothing launched: a null images / scratch / out / offsets, F < 1, H or W outside 1 .. AG_RENDER_MAX_SIDE, channels not 3 or 4,
 * quality outside 1 .. 100, an unknown subsampling, restart outside 1 .. AG_JPEG_MAX_RESTART, unaligned RGBA images, a scratch or an out that is
 * smaller than its query, a worst case beyond 2^31 - 1 bytes (hand in fewer frames).  No host synchronisation, no allocation, no memset, every
 * scratch word written before it is read, integer atomics in LDS only (exact in any order): the same bytes on every call, safe to capture. */
#define AG_JPEG_444 0
#define AG_JPEG_420 1
#define AG_JPEG_MAX_RESTART 16
#define AG_JPEG_BLOCK_BYTES 208
size_t ag_jpeg_scratch_bytes(int F, int H, int W, int subsampling, int restart);
size_t ag_jpeg_out_bytes(int F, int H, int W, int subsampling, int restart);
int ag_jpeg_encode(const uint8_t *images, int F, int H, int W, int channels, int quality, int subsampling, int restart, void *scratch,
                   size_t scratch_bytes, uint8_t *out, size_t out_bytes, int64_t *offsets, ag_stream_t stream);

/* ---- object masks from colour images (what the reference does with the masks of its detection and segmentation models,
 * src/planning/perception.py:176-209: join the "table" / "sheet" masks and the object masks, mask_table & ~mask_obj, keep every pixel that is NOT
 * table), with classical stages in the models' place: colour keys, square morphology, connected components, selection by area, hole filling
 * (DESIGN.md 8.18).  The arithmetic is stated by adaptigraph_amd/segment.py in numpy integers and repeated here operation for operation: every
 * result equals the statement's bit for bit.  Not: a learned model, text prompts, instances mapped to p_instance, watershed / grab-cut.
 * DEVICE arrays: images (C,H,W,channels) uint8, channels 4 (R, G, B, alpha; 4-byte aligned; alpha is ignored) or 3; masks (C,H,W) uint8, non-zero =
 * set, written as 0 / 1; labels (C,H,W) int32; count (C) int32.  Every image of a call is treated alone.
 * Shapes: 1 <= C <= 65535, H, W >= 1, H W <= 2^31 - 257 (a pixel's index is an int32), H <= 65535 AG_SEGMENT_TILE_H.  ag_segment_scratch_bytes
 * = the sum, each part rounded up to 256 bytes, of three int32 images (12 C H W), the scan's sums (4 C (H W / 256 + 2)), the selection's candidates
 * (64 C ceil(H W / 256) + 8 C) and two masks (2 C H W); 0 for a shape the calls refuse.  The calls that take scratch share it: calls on one stream
 * may use the same buffer.
 * ag_segment_color_mask (the models' part): integer HSV of a pixel, with mx, mn the channel maximum and minimum and d = mx - mn: V = mx;
 *   S = 0 if mx = 0, else (255 d + mx / 2) / mx; H = 0 if d = 0, else by the maximum channel, r before g before b: floor((60 (g - b) + d / 2) / d)
 *   mod 360, floor((60 (b - r) + d / 2) / d) + 120 mod 360, floor((60 (r - g) + d / 2) / d) + 240 mod 360 (floor toward minus infinity).  keys:
 *   HOST, n_keys <= AG_SEGMENT_MAX_KEYS rows of h_lo, h_hi, s_lo, s_hi, v_lo, v_hi, inclusive; h_lo > h_hi wraps through 359 -> 0; they travel as
 *   kernel arguments.  mask = a pixel lies in any key's box.  One launch.
 * ag_segment_morph: op AG_SEGMENT_ERODE / _DILATE / _OPEN / _CLOSE with the (2 radius + 1) square, 0 <= radius <= AG_SEGMENT_MAX_RADIUS; pixels
 *   outside the image are background for every operation.  A row pass and a column pass per erosion or dilation: two or four launches.  out
 *   may be mask.
 * ag_segment_label: the connected components of the set pixels under connectivity 4 or 8 (perception.py:176-190 receives them as instance masks).
 *   labels: 0 for background, else 1 .. count[c] in ascending order of a component's lowest row-major pixel index, restarting in every image;
 *   complete for any number of components.  Five launches: tile-local union-find in LDS over row runs, unions across the tile borders in global
 *   memory (agent-scope atomics only), flatten, the two-pass scan over the roots, relabel.  A root is its component's lowest index, whatever
 *   the order of the unions.
 * ag_segment_components: table (C,max_labels,8) int64 rows area, x_min, y_min, x_max, y_max, sum_x, sum_y, touches_border of labels
 *   1 .. min(count[c], max_labels); the other rows zero.  Integer atomics, one set per row run.  Two launches.
 * ag_segment_select: out = the components of mask with at least min_area pixels and, with keep_largest = k in 1 .. AG_SEGMENT_MAX_KEEP, of
 *   those the k largest, equal areas by the lower label (perception.py:191-202 picks masks by label; here by size); keep_largest 0 keeps all.
 *   Areas live at the root pixels: any number of components.  Five launches, seven with keep_largest.  out may be mask (the last launch writes it).
 * ag_segment_fill_holes: out = mask and every background component that no pixel of the image border belongs to, the background under the dual
 *   connectivity (4 where the foreground's is 8).  Five launches.  out may be mask.
 * ag_segment_keep: out = ~(table & ~objects), perception.py:203-209; objects may be NULL (no object mask: out = ~table).  One launch.
 * AG_ERR_ARG, nothing launched: a null pointer, a shape outside the ranges above, channels not 3 or 4, more than AG_SEGMENT_MAX_KEYS keys,
 * unaligned RGBA images, an unknown op, a radius, connectivity or keep_largest out of range, max_labels < 1; AG_ERR_WS: a scratch smaller than
 * ag_segment_scratch_bytes.  No host synchronisation, no allocation, no memset (every per-call word is written by a kernel of the call before it
 * is read), launch counts that depend on the arguments and never on the images, integer arithmetic only: the same bits on every call, safe to
 * capture. */
#define AG_SEGMENT_TILE_H 16
#define AG_SEGMENT_TILE_W 64
#define AG_SEGMENT_MAX_KEYS 8
#define AG_SEGMENT_MAX_KEEP 8
#define AG_SEGMENT_MAX_RADIUS 8
#define AG_SEGMENT_ERODE 0
#define AG_SEGMENT_DILATE 1
#define AG_SEGMENT_OPEN 2
#define AG_SEGMENT_CLOSE 3
void ag_segment_tile_sizes(int *tile_h, int *tile_w);
size_t ag_segment_scratch_bytes(int C, int H, int W);
int ag_segment_color_mask(const uint8_t *images, int C, int H, int W, int channels, const int32_t *keys /*host*/, int n_keys, uint8_t *mask,
                          ag_stream_t stream);
int ag_segment_morph(const uint8_t *mask, int C, int H, int W, int op, int radius, void *scratch, size_t scratch_bytes, uint8_t *out,
                     ag_stream_t stream);
int ag_segment_label(const uint8_t *mask, int C, int H, int W, int connectivity, void *scratch, size_t scratch_bytes, int32_t *labels,
                     int32_t *count, ag_stream_t stream);
int ag_segment_components(const int32_t *labels, const int32_t *count, int C, int H, int W, int max_labels, int64_t *table, ag_stream_t stream);
int ag_segment_select(const uint8_t *mask, int C, int H, int W, int connectivity, int min_area, int keep_largest, void *scratch,
                      size_t scratch_bytes, uint8_t *out, ag_stream_t stream);
int ag_segment_fill_holes(const uint8_t *mask, int C, int H, int W, int connectivity, void *scratch, size_t scratch_bytes, uint8_t *out,
                          ag_stream_t stream);
int ag_segment_keep(const uint8_t *table, const uint8_t *objects, int C, int H, int W, uint8_t *out, ag_stream_t stream);

/* ---- training batches assembled on the device (SURVEY.md §8f row n4 data side): DynDataset.__getitem__ for B samples at once plus their
 * collation, src/dynamics/dataset/dataset.py:10-252, with the dataset resident in HBM:
 *   obj_store   fp32: every episode's object positions (T_e, N_e, 3), one after the other
 *   tool_store  the tool positions (T_e, n_eef, 3) likewise, fp32 or — dims.tool_f64 — float64 (the dataset's own dtype: the actions are
 *               differences taken in that dtype and rounded to fp32 afterwards)
 *   episodes    (n_episodes, 4) int64: first point of the episode in obj_store, first point in tool_store, T_e, N_e
 *   epi (B) int32 episode of every sample; all of these are DEVICE arrays, nothing is read back.
 *
 * ag_gather_clouds: pts[b, :N, :] = frame frame[b] of episode epi[b], zeros behind, N = min(N_e, Nmax); count[b] = N: the padded clouds
 *   ag_fps pass 1 takes.  A sample whose episode or frame is out of range gets count 0.
 *
 * ag_assemble_batch: every per-item tensor of the collated batch in one launch, ns = no + n_eef nodes per sample (objects first):
 *   frames (B, H + Fu) int32 frame of every history / future slot; picks (B, K + 1) int32 as sampling.two_pass_tensors returns them: the
 *   key-point indices into the cloud, -1 behind the last, their number n_kp in column K (read on the device).
 *   state (B,H,ns,3): rows < n_kp the picked points, rows >= no the tool points, zeros between;  state_future (B,Fu,no,3) likewise (objects);
 *   eef_future (B,Fu-1,ns,3) the tool rows of future slot f;  action (B,ns,3) = tool[H] - tool[H-1], action_future (B,Fu-1,ns,3) =
 *   tool[H+f+1] - tool[H+f] (tool rows; object rows zero);  attrs (B,ns,2) = [row < n_kp, row >= no];  p_instance (B,no,1), obj_mask (B,no)
 *   = row < n_kp;  state_mask (B,ns) = row < n_kp or row >= no;  eef_mask (B,ns) = row >= no (masks: one byte, 0 / 1);
 *   material_index (B,no,n_mat) int64 = 1 at column mat_col of rows < n_kp.  With Fu == 1 eef_future / action_future are empty and may be NULL.
 *   noise (B,H,ns,3) float64 and rot (B,3,3) fp32, both or neither (dataset.py:184-195, randomness.use): state = fp32(double(state) + noise),
 *   one rounding, on every row; then every position tensor (state, state_future, eef_future, action, action_future) becomes a @ rot[b],
 *   out_j = fmaf(a2, r2j, fmaf(a1, r1j, a0 * r0j)).
 * An index outside its table (episode, frame, pick) yields zeros, never an out-of-range read.  No host synchronisation: safe to capture. */
typedef struct ag_batch_dims {
    int32_t B, H, Fu;         /* samples, n_his, n_future */
    int32_t no, n_eef;        /* max_nobj, tool points */
    int32_t K;                /* picks has K + 1 columns */
    int32_t n_mat, mat_col;   /* material_index width and the column set */
    int32_t n_episodes;
    int32_t tool_f64;         /* tool_store holds doubles */
} ag_batch_dims;
typedef struct ag_batch_out {
    float *state, *action, *eef_future, *action_future, *state_future, *attrs, *p_instance;
    uint8_t *obj_mask, *state_mask, *eef_mask;
    int64_t *material_index;
} ag_batch_out;
int ag_gather_clouds(const float *obj_store, const int64_t *episodes, int n_episodes, const int32_t *epi, const int32_t *frame, int B, int Nmax,
                     float *pts, int32_t *count, ag_stream_t stream);
int ag_assemble_batch(const ag_batch_dims *dims, const float *obj_store, const void *tool_store, const int64_t *episodes, const int32_t *epi,
                      const int32_t *frames, const int32_t *picks, const double *noise, const float *rot, const ag_batch_out *out,
                      ag_stream_t stream);

/* ---- training path: graph pieces of DynamicsPredictor.forward and their adjoints on the CSR adjacency.
 * Plain row-major fp32 tensors of arbitrary feature width D; every reduction runs in a fixed order (no atomics).
 *
 * ag_gather_rows:  out[e,:] = x[idx[e],:]                    — replaces Rr.bmm(X) / Rs.bmm(X), model.py:224-249,283-284
 * ag_segment_sum:  out[n,:] = sum_{k in [ptr[n],ptr[n+1])} vals[perm ? perm[k] : k, :]
 *                  — replaces Rr_t.bmm (model.py:295) with perm = NULL over the receiver-sorted edges, and is the adjoint of
 *                  a gather by any index given that index's (pointer, permutation) view (receivers: row_ptr/NULL;
 *                  senders: col_ptr/stable argsort of send)
 * ag_message_forward:  agg[n,:] = sum_{e in row n} relu((eterm[e,:] + hr[n,:]) + hs[send[e],:])
 *                  — relation_propagator + Rr_t.bmm of one round (model.py:283-295) after the W_rp column split
 * ag_message_backward: grad_edge[e,:] = grad_agg[recv(e),:] * [pre-activation > 0]  (= d loss / d eterm[e]),
 *                  grad_hr[n,:] = sum_{e in row n} grad_edge[e,:];  d loss / d hs = ag_segment_sum(grad_edge, col_ptr, perm) */
int ag_gather_rows(const float *x, const int32_t *idx, float *out, int64_t n_out, int D, ag_stream_t stream);
int ag_segment_sum(const float *vals, const int32_t *ptr, const int32_t *perm, float *out, int64_t n_seg, int D, ag_stream_t stream);
int ag_message_forward(const float *eterm, const float *hr, const float *hs, const int32_t *row_ptr, const int32_t *send, float *agg,
                       int64_t n_nodes, int D, ag_stream_t stream);
int ag_message_backward(const float *eterm, const float *hr, const float *hs, const int32_t *row_ptr, const int32_t *send,
                        const float *grad_agg, float *grad_edge, float *grad_hr, int64_t n_nodes, int D, ag_stream_t stream);

/* ag_edge_views: the SENDER-side view of a receiver-sorted edge list, on the device in one launch — what the autograd of the one-hot Rs.bmm
 * gathers (model.py:224-249, 283-284: their backward is Rs^T.bmm) needs as (pointer, permutation), and what torch.sort(stable) + bincount +
 * cumsum built before:
 *   send_perm (n_edges) = the edges in ascending sender order, equal senders in ascending edge order (a stable argsort of edge_send),
 *   col_ptr (B*N + 1)   = exclusive prefix of the per-sender edge counts, col_ptr[B*N] = n_edges = row_ptr[B*N].
 * row_ptr (B*N + 1) and edge_send are those of ag_build_edges: sample b's edges are [row_ptr[bN], row_ptr[(b+1)N]) and their senders lie in
 * [bN, (b+1)N) (an edge whose sender does not is skipped, and its slot of send_perm left unwritten).  One workgroup per sample: a counting
 * sort with integer counters only, so the result does not depend on any order of execution.  No memset, no host synchronisation, no
 * allocation: capturable.  `workspace`: ag_edge_views_workspace_bytes(B, N) bytes (the counters of samples too large for LDS; may be 0). */
size_t ag_edge_views_workspace_bytes(int B, int N);
int ag_edge_views(const int32_t *row_ptr, const int32_t *edge_send, int B, int N, int32_t *col_ptr, int32_t *send_perm, void *workspace,
                  ag_stream_t stream);

/* ag_step_update_forward / ag_step_update_backward: the tail of a model step of the DIFFERENTIABLE rollouts, out of place, and its adjoint —
 * one launch each (forward_dynamics.py:160-176 of dynamics / :356-372 of dynamics_masked under autograd; ag_rollout's in-place step update
 * is the no-grad form):
 *   rec_out[b]          = repeat[b] == step ? pred[b] : rec[b]                                   record-on-repeat      (rec may be NULL: zeros)
 *   y[b]                = min_i pred[b,i,1] (AG_HEIGHT_MIN) | sum_i pred[b,i,1] m[b,i] / sum_i m[b,i] (AG_HEIGHT_MASKED_MEAN, m = obj_mask) ; + raise
 *   state_out[b,h]      = state[b,h+1] (h < H-1);  state_out[b,H-1] = [pred[b] | tool rows: (state[b,H-1].x + delta.x, y[b], state[b,H-1].z + delta.z)]
 * pred (B,n_p,3), state / state_out (B,H,N,3), delta (B,N,3), rec / rec_out (B,n_p,3), repeat (B), obj_mask (B,n_p) bytes; the tool rows are
 * the last N - n_p of a sample.  The sums run in ag_rollout's order (thread-strided partials, xor butterfly, (w0 + w1) + (w2 + w3)).
 * Backward, given grad_state_out and grad_rec_out:
 *   grad_rec   = repeat[b] == step ? 0 : grad_rec_out
 *   grad_state[b,h] = grad_state_out[b,h-1] (h >= 1; the oldest frame's gradient is dropped by the shift) + the tool rows' x / z of
 *                     grad_state_out[b,H-1] at h = H-1;  grad_delta = those tool x / z, zero elsewhere
 *   grad_pred  = (grad_state_out[b,H-1,:n_p] + [repeat[b] == step] grad_rec_out[b]) + the height's share in y: with G[b] the sum of the tool
 *                rows' y gradients, G to the FIRST particle that attains the minimum (AG_HEIGHT_MIN), G / count to every masked-in particle
 *                (AG_HEIGHT_MASKED_MEAN).
 * One fixed summation order per output, no atomics: the same bits on every call. */
int ag_step_update_forward(const float *pred, const float *state, const float *delta, const float *rec, const int32_t *repeat, const uint8_t *obj_mask,
                           int B, int H, int N, int n_p, int step, int height_mode, float raise, float *state_out, float *rec_out, ag_stream_t stream);
int ag_step_update_backward(const float *pred, const int32_t *repeat, const uint8_t *obj_mask, int B, int H, int N, int n_p, int step, int height_mode,
                            const float *grad_state_out, const float *grad_rec_out, float *grad_pred, float *grad_state, float *grad_delta,
                            float *grad_rec, ag_stream_t stream);

/* ---- training path, dense stacks (row n4): the Linear(+ReLU) chains of DynamicsPredictor.forward and their backward as fused
 * MFMA kernels (activations stay in registers between layers, in both directions; arithmetic per call: `precision` below — the
 * Python training path defaults to split-bf16).  Replaces the forward/backward of
 *   AG_CHAIN_EDGE     relation_encoder.model.{0,2,4} (+ReLU each) and relation_propagator.linear[:, :nf] (no ReLU)   model.py:274,289
 *   AG_CHAIN_NODE     particle_encoder.model.{0,2,4} (+ReLU each)                                                    model.py:268
 *   AG_CHAIN_DECODER  non_rigid_predictor.linear_{0,1} (+ReLU), linear_2                                             model.py:306
 * in src/dynamics/train/train.py:90-112 (forward + loss.backward()).
 *
 * ag_train_pack: device-side packing of one layer into the kernels' chunk-image format (weights change every optimiser step):
 *   op(W)[o][k] = transposed ? W[k*ld + col0 + o] : W[o*ld + col0 + k] (o < n_out, k < n_in), bias (nullable) as column n_in;
 *   `compact` = the single-chunk first-layer image (n_in + 1 <= 32), else `n_tiles` 32-row images; dst gets
 *   (compact ? 1 : n_tiles) * 5120 floats.  Forward streams hold the layers in order (first layer compact for EDGE/NODE);
 *   backward streams hold W_{L-1}^T .. W_1^T (5 images each, no bias) then W_0^T (1 image for EDGE/NODE, 5 for DECODER).
 * ag_train_chain: forward (backward = 0): x ([rows][d_in] dense for EDGE/NODE, [rows_pad][160] for DECODER) -> y[l], l < L, each
 *   [rows_pad][160] fp32 (rows_pad = rows rounded up to 128; columns >= 150 and padding rows are scratch).  backward = 1:
 *   dy ([rows_pad][160], gradient w.r.t. y[L-1]) + the saved y[l] -> dz[l] (pre-activation gradients, [rows_pad][160]) and
 *   dx (same shape as x; nullable for EDGE/NODE).  Weight gradients are dz[l]^T y[l-1] — plain library GEMMs left to the caller.
 *   `y` / `dz` are HOST arrays of L device pointers.
 * `precision`: 0 = exact fp32 MFMA, non-zero = split-bf16 (as the inference engine's mode 1); the packed stream and the chain call
 *   must use the same value. */
enum { AG_CHAIN_EDGE = 0, AG_CHAIN_NODE = 1, AG_CHAIN_DECODER = 2 };
int ag_train_pack(const float *W, const float *bias, int n_out, int n_in, int ld, int col0, int transposed, int compact, int n_tiles,
                  int precision, float *dst, ag_stream_t stream);
int ag_train_chain(int kind, int backward, int precision, const float *x, const float *packed, float *const *y, const float *dy,
                   float *const *dz, float *dx, int64_t rows, int d_in, ag_stream_t stream);

/* rel_inputs of DynamicsPredictor.forward (model.py:220-253) and its adjoint, from one per-node table
 *   tab (n_nodes, D) = [attrs (attr_dim) | group = cat(p_instance, 0) (group_dim) | state_norm (D - attr_dim - group_dim)]:
 *   out[e] = [tab[r][:A] | tab[s][:A] | sum |tab[r][A:A+G] - tab[s][A:A+G]| | tab[r][A+G:] - tab[s][A+G:]], width 2A + 1 + (D - A - G),
 * with r = recv[e], s = send[e] (global node ids).  Backward: grad_tab[n] = sum over the edges n receives (row_ptr order) and
 * sends (col_ptr / send_perm order) of the per-edge gradients; scratch_r / scratch_s are (n_edges, D) each. */
int ag_edge_inputs_forward(const float *tab, int D, int attr_dim, int group_dim, const int32_t *recv, const int32_t *send, float *out, int64_t n_edges,
                           ag_stream_t stream);
int ag_edge_inputs_backward(const float *tab, int D, int attr_dim, int group_dim, const int32_t *recv, const int32_t *send, const int32_t *row_ptr,
                            const int32_t *col_ptr, const int32_t *send_perm, const float *grad_out, float *scratch_r, float *scratch_s, float *grad_tab,
                            int64_t n_edges, int64_t n_nodes, ag_stream_t stream);

/* The node update's residual, Propagator.forward with res (model.py:36-40): y = relu((a + b) + c) over n contiguous floats
 * (n % 4 == 0, 16-byte aligned), and its adjoint out = g * [y > 0] (the same for all three inputs). */
int ag_add3_relu(const float *a, const float *b, const float *c, float *y, int64_t n, ag_stream_t stream);
int ag_relu_mask(const float *g, const float *y, float *out, int64_t n, ag_stream_t stream);

/* Weight and bias gradients of up to 4 dense layers in two launches: for layer l,
 *   out[l][o][k] = sum_rows dz[l][row][o] * prev[l][row][k]   (k < n_in[l])      = d loss / d W_l[o][k]
 *   out[l][o][n_in[l]] = sum_rows dz[l][row][o]                                   = d loss / d b_l[o]
 * dz[l] has row stride dz_ld[l] <= 160 (160 for the tables of ag_train_chain backward; n_out for a dense (rows, n_out) gradient),
 * prev[l] is the layer's input with row stride prev_ld[l] (>= n_in[l]); out is [n_layers][160][160] fp32.  Rows are split into slabs, partial sums meet in a fixed order: bit-reproducible.
 * dz / dz_ld / prev / prev_ld / n_in are HOST arrays. */
size_t ag_train_weight_grads_workspace_bytes(int64_t rows, int n_layers);
int ag_train_weight_grads(int n_layers, const float *const *dz, const int32_t *dz_ld, const float *const *prev, const int32_t *prev_ld, const int32_t *n_in,
                          int64_t rows, float *out, void *workspace, size_t workspace_bytes, ag_stream_t stream);

/* The same, ACCUMULATING layer l's gradients straight into caller storage (a parameter's .grad): w_grad[l][o * w_grad_ld[l] + k] +=
 * dW_l[o][k] for o < n_out[l], k < n_in[l], and b_grad[l][o] += db_l[o] (b_grad or b_grad[l] may be NULL).  A layer whose w_grad[l]
 * is NULL goes to `out` as above.  This is what removes autograd's per-parameter slice / clone / accumulate kernels from the
 * training step (train.py:110-112 loss.backward() accumulates into .grad the same way). */
int ag_train_weight_grads_into(int n_layers, const float *const *dz, const int32_t *dz_ld, const float *const *prev, const int32_t *prev_ld,
                               const int32_t *n_in, int64_t rows, float *out, float *const *w_grad, const int32_t *w_grad_ld, float *const *b_grad,
                               const int32_t *n_out, void *workspace, size_t workspace_bytes, ag_stream_t stream);

/* Optional per-kernel timing with HIP events recorded on the caller's stream around every launch of each
 * kernel class (used by bench.py for the roofline line; off by default, costs two event records per launch).
 * ag_profile_read synchronises on the recorded events and returns, per class, the summed milliseconds, the
 * launch count, and for AG_K_EDGE_ENCODE the summed number of edges processed (units for the roofline). */
enum { AG_K_EDGES = 0, AG_K_NODE_ENCODE = 1, AG_K_EDGE_ENCODE = 2, AG_K_AGGREGATE = 3, AG_K_NODE_UPDATE = 4,
       AG_K_ROLLOUT_STEP = 5, AG_K_COUNT = 6 };
int ag_profile_enable(ag_model *m, int enable);
int ag_profile_read(ag_model *m, double *ms /*AG_K_COUNT*/, int64_t *launches /*AG_K_COUNT*/, int64_t *edges);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* ADAPTIGRAPH_HIP_H */
