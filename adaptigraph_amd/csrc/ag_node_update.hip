// ag_node_update.hip — streaming node update, and the launch of either node update (shared device layer: ag_mlp_dev.h)
#include "ag_mlp_dev.h"

namespace {

// `agg` as q16 rows, as this kernel reads them (format and decoding: ag_mlp_dev.h)
struct AggRowQ16 { int4 v[AG_NT][2]; uint2 ex; };
__device__ __forceinline__ void load_rowmajor_q16(const unsigned char *row, AggRowQ16 &r, int h)
{
#pragma unroll
    for (int t = 0; t < AG_NT; ++t) {
        r.v[t][0] = *reinterpret_cast<const int4 *>(row + 64 * t + 32 * h);
        r.v[t][1] = *reinterpret_cast<const int4 *>(row + 64 * t + 32 * h + 16);
    }
    r.ex = *reinterpret_cast<const uint2 *>(row + 280);
}
__device__ __forceinline__ void agg_q16_tile(const AggRowQ16 &r, int t, int h, f32x16 &v)
{
    const float sc = agg_q16_tile_scale(r.ex, t);
    float lo[8], hi[8];
    agg_q16_decode8(r.v[t][0], sc, lo);
    agg_q16_decode8(r.v[t][1], sc, hi);
#pragma unroll
    for (int k = 0; k < 8; ++k) { v[k] = lo[k]; v[8 + k] = hi[k]; }
    if (t == 4) {      // features 150..159 do not exist: their positions hold the exponent bytes (and zeros)
        if (h) { v[10] = 0.0f; v[11] = 0.0f; }
        v[12] = 0.0f; v[13] = 0.0f; v[14] = 0.0f; v[15] = 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------
// One propagation round at node level: fused segment reduce (aggregate_rows) or a pre-computed `agg` table,
// then the node update (model.py:299-301), then either the next round's node-level relation terms (Hr, Hs)
// or — after the last round — the decoder + clamp + integrate (model.py:306-309).
// ---------------------------------------------------------------------------------------------
// FUSE (precision mode 2 only): the round's segment reduce runs INSIDE this kernel, so the `agg` table never exists in HBM
// (-328 MB of the 2.3 GB a round moves) and the aggregate launch disappears.  The reduce keeps the standalone kernel's memory
// pattern — 20 adjacent lanes stream one node's 320-byte Eterm rows, 12 nodes per pass of the workgroup — because that pattern,
// not the MFMA lane layout, is what coalesces (the r01 fusion gathered row-per-lane in the MFMA layout: 0.52 ms vs 0.30 + 0.20).
// Its sums cross to the owning wave's B-operand registers through a 32-row LDS stage (row stride 164 floats: conflict-free
// ds_read_b128), one wave's 32 rows at a time.  The two workgroups of a CU are in different phases, so one's latency-bound
// gather overlaps the other's MFMA chain; row tiles are dealt XCD-contiguously so a graph's sender rows stay in one L2.
// Measured (C2, r02): 0.474 ms per round vs 0.292 + 0.196 separate (-3 %), 1.97 GB at 4.2 TB/s instead of 2.3 GB at 4.7: the
// bytes saved are paid back in bandwidth, and in the two-stream rollout the separate kernels co-run better (99 k vs 103 k
// graph-steps/s), so this is ag_set_option("fuse_aggregate", 2), not the default.  Keeping 8 edges or three nodes per lane in
// flight changed nothing (0.473 / 0.475 ms): the round is bandwidth-bound at what this access mix reaches, not latency-bound.
#define AG_STAGE_LD 164
template <class Prec, bool LAST, bool FUSE, bool HSQ = false, bool AQ = false>      // HSQ: the next round's sender table is written as q16 rows (mode 2); AQ: `agg` is read as q16 rows
__global__ __launch_bounds__(AG_MLP_THREADS, AG_MLP_WG_PER_CU) void node_update_kernel(AgWeights w, AgFwdArgs a)
{
    AG_LDS_DECL
    __shared__ __attribute__((aligned(16))) float stage[FUSE ? 32 * AG_STAGE_LD : 4];
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5, wave = tid >> 6;
    const int Mn = ag_rows(a);
    const int ntiles = (Mn + AG_ROWS_PER_BLOCK - 1) / AG_ROWS_PER_BLOCK;
    ChunkPipe P{LAST ? pick<Prec>(w.node_last, w.node_last_b3) : pick<Prec>(w.node_mid, w.node_mid_b3), LAST ? 16 : 15, 0, 0, lds};
    pipe_start(P);
    TileQueue q(nullptr, s_next_tile);   // ~4 row tiles per workgroup: nothing to balance, static stride
    if (FUSE) {   // XCD-contiguous deal: block b sits on XCD b % 8; give XCD x the logical ids [x*nb/8, (x+1)*nb/8) so that in every
                  // round of the grid stride one XCD works on ~nb/8 CONSECUTIVE row tiles (whole graphs)
        const int nb = gridDim.x, bid = blockIdx.x, qq = nb >> 3, rr = nb & 7, xcd = bid & 7, idx = bid >> 3;
        q.tile = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + idx;
    }
    const bool ovf = a.ovf && *a.ovf != 0;      // de-duplicated call that overflowed the compact tables: Pn / h come from the packed tables
    const float *pn_rows = ovf ? nullptr : a.pn_rows, *h_rows = ovf ? nullptr : a.h_rows;
    f32x16 agg_next[AQ ? 1 : AG_NT];      // (!FUSE) the agg rows of the row tile about to start
    AggRowQ16 aggq_next;                  // (AQ: as loaded, decoded where the operand image is built)
    const unsigned char *aggq = reinterpret_cast<const unsigned char *>(a.agg);
    bool have_next = false;
#pragma unroll 1
    while (q.tile < ntiles) {
        const int tile = q.tile;
        q.claim();
        const int g = tile * AG_ROWS_PER_BLOCK + wave * 32 + j;
        const bool valid = g < Mn;
        const int gc = valid ? g : 0;

        typename Prec::Act x, y;
        if constexpr (FUSE) {
            AgFwdArgs ar = a;
            ag_overflow_view(ar);
            const int ng = lane / AG_AGG_GROUP, c = lane - ng * AG_AGG_GROUP, f0 = ag_half_lane_feature(c);      // twenty lanes of one wave per node
            const int slot = wave * AG_AGG_NODES_PER_WAVE + ng;                                                      // 12 node slots per pass
#pragma unroll 1
            for (int grp = 0; grp < AG_MLP_WAVES; ++grp) {
#pragma unroll 1
                for (int pass = 0; pass < 3; ++pass) {                   // 3 x 12 node slots >= 32 rows
                    const int r = pass * 12 + slot;
                    if (ng < AG_AGG_NODES_PER_WAVE && r < 32) {
                        const int gn = tile * AG_ROWS_PER_BLOCK + grp * 32 + r;
                        float4 acc0 = make_float4(0.f, 0.f, 0.f, 0.f), acc1 = acc0;
                        if (gn < Mn) {
                            const int E_ = ar.self_info ? ag_edges(ar) : 0;
                            if (ar.self_info) {
                                if (a.hs_q16) ag_reduce_node_q16<AG_AGG_IN_FLIGHT, true, true>(ar, gn, c, ng * AG_AGG_GROUP, acc0, acc1, E_);
                                else ag_reduce_node_q16<AG_AGG_IN_FLIGHT, false, true>(ar, gn, c, ng * AG_AGG_GROUP, acc0, acc1, E_);
                            } else {
                                if (a.hs_q16) ag_reduce_node_q16<AG_AGG_IN_FLIGHT, true, false>(ar, gn, c, ng * AG_AGG_GROUP, acc0, acc1);
                                else ag_reduce_node_q16<AG_AGG_IN_FLIGHT, false, false>(ar, gn, c, ng * AG_AGG_GROUP, acc0, acc1);
                            }
                        }
                        if (a.agg_q16) ag_q16_roundtrip_segment(acc0, acc1);      // (the 16-bit rounding the `agg` rows of the separate kernels go through: same bits)
                        *reinterpret_cast<float4 *>(stage + r * AG_STAGE_LD + f0) = acc0;
                        *reinterpret_cast<float4 *>(stage + r * AG_STAGE_LD + f0 + 8) = acc1;
                    }
                }
                __syncthreads();
                if (wave == grp) {
#pragma unroll
                    for (int t = 0; t < AG_NT; ++t) {
                        f32x16 v;
#pragma unroll
                        for (int qd = 0; qd < 4; ++qd) {
                            const float4 u = *reinterpret_cast<const float4 *>(stage + j * AG_STAGE_LD + 32 * t + 8 * qd + 4 * h);
                            v[4 * qd] = u.x; v[4 * qd + 1] = u.y; v[4 * qd + 2] = u.z; v[4 * qd + 3] = u.w;
                        }
                        Prec::set_tile(x, t, v);
                    }
                }
                __syncthreads();
            }
        } else {
            // this row tile's agg rows: loaded during the PREVIOUS row tile's last two layers (below), except for a workgroup's first tile
            if (!have_next) {
                if constexpr (AQ) load_rowmajor_q16(aggq + (size_t)gc * (2 * AG_FP), aggq_next, h);
                else load_rowmajor(a.agg + (size_t)gc * AG_FP, agg_next, h);
            }
        }
        const size_t blk = (size_t)(tile * AG_MLP_WAVES + wave) * AG_PACK_BLOCK + h * 128 + j * 4;
        const size_t rowoff = (size_t)g * AG_FP + 4 * h;   // own row even when past Mn (padding rows)
        // Pn (+ h in round 0) come from the compact rows of the de-duplicated node encoder when it is on
        const size_t crow = pn_rows ? (size_t)a.node_row[gc] * AG_FP + 4 * h : 0;
        const ResidInit resid{pn_rows ? pn_rows + crow : a.pn + blk, h_rows ? h_rows + crow : a.h + blk, pn_rows != nullptr, h_rows != nullptr};
        resid.prefetch();      // issued before the operand split of agg below, whose ~250 VALU instructions cover part of the latency
        if constexpr (!FUSE) {
#pragma unroll
            for (int t = 0; t < AG_NT; ++t) {
                if constexpr (AQ) { f32x16 v; agg_q16_tile(aggq_next, t, h, v); Prec::set_tile(x, t, v); }
                else Prec::set_tile(x, t, agg_next[t]);
            }
        }
        // The next row tile of this workgroup (static grid stride: TileQueue without a counter): its agg rows are fetched while this tile's second
        // and third layers run, into the registers the first layer's input image has just left.
        const int tile_n = tile + (int)gridDim.x;
        auto prefetch_agg = [&]() {
            if constexpr (!FUSE) {
                have_next = tile_n < ntiles;       // workgroup-uniform
                if (have_next) {
                    const int gn = tile_n * AG_ROWS_PER_BLOCK + wave * 32 + j;
                    if constexpr (AQ) load_rowmajor_q16(aggq + (size_t)(gn < Mn ? gn : 0) * (2 * AG_FP), aggq_next, h);
                    else load_rowmajor(a.agg + (size_t)(gn < Mn ? gn : 0) * AG_FP, agg_next, h);
                } else {      // (a defined value on this path too: otherwise the previous tile's rows stay live through the whole first layer)
                    if constexpr (AQ) {
#pragma unroll
                        for (int t = 0; t < AG_NT; ++t) { aggq_next.v[t][0] = make_int4(0, 0, 0, 0); aggq_next.v[t][1] = make_int4(0, 0, 0, 0); }
                        aggq_next.ex = make_uint2(0u, 0u);
                    } else {
#pragma unroll
                        for (int t = 0; t < AG_NT; ++t)
#pragma unroll
                            for (int r = 0; r < 16; ++r) agg_next[t][r] = 0.0f;
                    }
                }
            }
        };
        if (!LAST) {
            dense<Prec, AG_F, true, false>(P, x, y, resid, PackStoreEpi{a.h + blk});   // h'
            q.publish();
            prefetch_agg();
            // Hr/Hs of the NEXT round go to the alternate tables: other workgroups of this launch may still be
            // gathering this round's Hs rows (fused aggregation reads them inside this kernel).
            dense_store<Prec, AG_F, false, false>(P, y, ZeroInit{}, RowStoreEpi{a.hr_out + rowoff});
            if constexpr (HSQ) dense_store<Prec, AG_F, false, false>(P, y, ZeroInit{}, RowStoreQ16Epi{reinterpret_cast<unsigned char *>(a.hs_out) + (size_t)g * (2 * AG_FP), h, a.status});
            else dense_store<Prec, AG_F, false, false>(P, y, ZeroInit{}, RowStoreEpi{a.hs_out + rowoff});
        } else {
            dense<Prec, AG_F, true, false>(P, x, y, resid);   // particle_effect'
            q.publish();
            dense<Prec, AG_F, true, true>(P, y, x, ZeroInit{});    // linear_0 + ReLU
            dense<Prec, AG_F, true, true>(P, x, y, ZeroInit{});    // linear_1 + ReLU
            prefetch_agg();                                        // (both activation images are live until here: the decoder ping-pongs them)
            f32x16 m;
            Prec::template layer<AG_F, 1, false, true>(P, y, ZeroInit{}, NoEpi{},      // linear_2 -> rows 0..2 of tile 0
                                                       [&](int, const f32x16 &v) { m = v; });
            const int go = a.row_orig ? a.row_orig[gc] : gc;      // (shared-state rollout: the node this compact row stands for; predictions are stored by row)
            const int b = go / a.N, i = go - b * a.N;
            if (valid && h == 0 && i < a.n_p) {
                const float *cur = a.state + (((size_t)b * AG_NHIS + (AG_NHIS - 1)) * a.N + i) * 3;
                float *pm = a.pred_motion + (a.row_orig ? (size_t)gc : (size_t)b * a.n_p + i) * 3;
                float *pp = a.pred_pos + (a.row_orig ? (size_t)gc : (size_t)b * a.n_p + i) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float mv = m[c];
                    pm[c] = mv;
                    pp[c] = cur[c] + fminf(fmaxf(mv, -a.clamp), a.clamp);   // model.py:309
                }
            }
        }
        q.next();
    }
}

}  // namespace

void ag_launch_node_update(const AgWeights &w, const AgFwdArgs &a, const AgPath &p, int last, hipStream_t s)
{
    const AgNodeUpdate &v = last ? p.last : p.mid;
    const dim3 grid(grid_for(a.B * a.N, a.max_blocks)), block(AG_MLP_THREADS);
    if (v.ws) { ag_launch_node_update_ws(w, a, v, s); return; }
    if (!p.b3) {
        if (last) hipLaunchKernelGGL((node_update_kernel<PrecF32, true, false>), grid, block, 0, s, w, a);
        else hipLaunchKernelGGL((node_update_kernel<PrecF32, false, false>), grid, block, 0, s, w, a);
    } else if (v.fused) {      // cooperative LDS-staged reduce inside the kernel (no aggregate launch, no agg table)
        if (last) hipLaunchKernelGGL((node_update_kernel<PrecB3, true, true>), grid, block, 0, s, w, a);
        else if (v.hs_q16) hipLaunchKernelGGL((node_update_kernel<PrecB3, false, true, true>), grid, block, 0, s, w, a);
        else hipLaunchKernelGGL((node_update_kernel<PrecB3, false, true>), grid, block, 0, s, w, a);
    } else if (v.agg_q16) {    // (mode 2 only: `agg` arrives as q16 rows; its rounds before the last write Hs as q16 rows)
        if (last) hipLaunchKernelGGL((node_update_kernel<PrecB3, true, false, false, true>), grid, block, 0, s, w, a);
        else hipLaunchKernelGGL((node_update_kernel<PrecB3, false, false, true, true>), grid, block, 0, s, w, a);
    } else if (last) hipLaunchKernelGGL((node_update_kernel<PrecB3, true, false>), grid, block, 0, s, w, a);
    else if (v.hs_q16) hipLaunchKernelGGL((node_update_kernel<PrecB3, false, false, true>), grid, block, 0, s, w, a);
    else hipLaunchKernelGGL((node_update_kernel<PrecB3, false, false>), grid, block, 0, s, w, a);
}
