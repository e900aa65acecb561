// ag_edge_encode.hip — streaming edge encoder, and the launch of either edge encoder (shared device layer: ag_mlp_dev.h)
#include "ag_mlp_dev.h"

namespace {

#ifndef AG_H3_WG_PER_CU
#define AG_H3_WG_PER_CU 2    // edge_encode_kernel<PrecH3>: two activation images (fp16 + expanded residual) per Act, 40 KB LDS per workgroup
#endif

// ---------------------------------------------------------------------------------------------
// Edge encoder + pstep-invariant edge term.
//   rel_inputs = [attrs_r | attrs_s | sum|g_r - g_s| | state_norm_r - state_norm_s]   model.py:220-253
//   enc_e      = Encoder(rel_inputs)                                                   model.py:274
//   Eterm      = W_rp[:, :F] . enc_e + b_rp      (first column block of relation_propagator, model.py:289)
// The one-hot gathers Rr.bmm / Rs.bmm become indexed reads of the (L2-resident) raw node inputs.
// ---------------------------------------------------------------------------------------------
template <class Prec> constexpr int kEdgeWgPerCu = AG_MLP_WG_PER_CU;
template <> constexpr int kEdgeWgPerCu<PrecH3> = AG_H3_WG_PER_CU;
// weight stream of the edge stack per arithmetic, and whether its first-layer image carries the residual columns (f16_residual)
template <class Prec> constexpr bool kEdgeResidualSlots = false;
template <> constexpr bool kEdgeResidualSlots<PrecH3> = true;
template <class Prec> __device__ __forceinline__ const float4 *edge_stream(const AgWeights &w) { return pick<Prec>(w.edge_encode, std::is_same_v<Prec, PrecH3> ? w.edge_encode_h2 : w.edge_encode_b3); }
template <class Prec>
__global__ __launch_bounds__(AG_MLP_THREADS, (kEdgeWgPerCu<Prec>)) void edge_encode_kernel(AgWeights w, AgFwdArgs a)
{
    AG_LDS_DECL
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5, wave = tid >> 6;
    const int E = ag_edges(a) + a.self_rows;      // (+ the class rows of elided self-loops, AgFwdArgs::self_info: synthetic edges behind the list)
    if (a.edge_counter && blockIdx.x == 0 && tid == 0) atomicAdd(a.edge_counter, (unsigned long long)E);
    const int ntiles = (E + AG_ROWS_PER_BLOCK - 1) / AG_ROWS_PER_BLOCK;
    if ((int)blockIdx.x >= ntiles) return;
    ChunkPipe P{edge_stream<Prec>(w), 16, 0, 0, lds, w.edge_scale_h3};
    pipe_start(P);
    TileQueue q(a.tile_ctr, s_next_tile);   // ~38 row tiles per workgroup at C2
#pragma unroll 1
    while (q.tile < ntiles) {
        const int tile = q.tile;
        q.claim();
        const int e = tile * AG_ROWS_PER_BLOCK + wave * 32 + j;
        const bool valid = e < E;
        int r = valid ? a.edge_recv[e] : 0, s = valid ? a.edge_send[e] : 0;
        // synthetic self-edge of attribute class r - class_row0 (self-edge elision): [a, a, 0, 0 ...] — a real self-loop's inputs (x - x = +0)
        const int cls = (a.self_rows && r >= a.self_class_row0) ? r - a.self_class_row0 : -1;      // (every copy of a class row carries the class's node-table row)
        if (cls >= 0) r = s = 0;
        const int b = r / a.N, ri = r - b * a.N, si = s - b * a.N;

        float feat[24];
#pragma unroll
        for (int k = 0; k < 24; ++k) feat[k] = 0.0f;
        feat[0] = a.attrs[(size_t)r * 2]; feat[1] = a.attrs[(size_t)r * 2 + 1];
        feat[2] = a.attrs[(size_t)s * 2]; feat[3] = a.attrs[(size_t)s * 2 + 1];
        if (cls >= 0) { feat[0] = feat[2] = cls == 0 ? 1.0f : 0.0f; feat[1] = feat[3] = cls == 0 ? 0.0f : 1.0f; }
        {
            float gd = 0.0f;   // g = cat([p_instance, 0]) (model.py:235), group_diff = sum |g_r - g_s| (:238)
            for (int ii = 0; ii < a.n_inst; ++ii) {
                const float gr = ri < a.n_p ? a.p_instance[((size_t)b * a.n_p + ri) * a.n_inst + ii] : 0.0f;
                const float gs = si < a.n_p ? a.p_instance[((size_t)b * a.n_p + si) * a.n_inst + ii] : 0.0f;
                gd += fabsf(gr - gs);
            }
            feat[4] = gd;
        }
        feat[AG_EDGE_IN] = 1.0f;   // bias column of relation_encoder.model.0
        {
            const float *st = a.state + (size_t)b * AG_NHIS * a.N * 3;
            float pr[AG_NHIS][3], ps[AG_NHIS][3];
#pragma unroll
            for (int hh = 0; hh < AG_NHIS; ++hh)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    pr[hh][c] = st[((size_t)hh * a.N + ri) * 3 + c];
                    ps[hh][c] = st[((size_t)hh * a.N + si) * 3 + c];
                }
#pragma unroll
            for (int hh = 0; hh + 1 < AG_NHIS; ++hh)   // state_res = state[:,1:] - state[:,:-1]  (model.py:155)
#pragma unroll
                for (int c = 0; c < 3; ++c) feat[5 + hh * 3 + c] = (pr[hh + 1][c] - pr[hh][c]) - (ps[hh + 1][c] - ps[hh][c]);
#pragma unroll
            for (int c = 0; c < 3; ++c) feat[5 + (AG_NHIS - 1) * 3 + c] = pr[AG_NHIS - 1][c] - ps[AG_NHIS - 1][c];
            if (cls >= 0)      // (node 0 stood in for the class row's endpoints: its differences with itself are +0 unless it is non-finite)
#pragma unroll
                for (int k = 5; k < AG_EDGE_IN; ++k) feat[k] = 0.0f;
        }
        f32x16 in0;
#pragma unroll
        for (int r16 = 0; r16 < 16; ++r16) in0[r16] = 0.0f;
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int p = 0; p < 4; ++p) in0[4 * q + p] = h ? feat[8 * q + 4 + p] : feat[8 * q + p];
        if constexpr (kEdgeResidualSlots<Prec>) {      // fp16 residuals of the state differences in the spare K slots 18..29 (see f16_residual)
#pragma unroll
            for (int q = 2; q < 4; ++q)
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int k0 = 8 * q + p, k1 = k0 + 4;      // this lane half's slot: k0 (h = 0) or k1 (h = 1)
                    const bool l0 = k0 >= AG_EDGE_LO_SLOT0 && k0 < AG_EDGE_LO_SLOT0 + AG_EDGE_LO_COUNT;
                    const bool l1 = k1 >= AG_EDGE_LO_SLOT0 && k1 < AG_EDGE_LO_SLOT0 + AG_EDGE_LO_COUNT;
                    const float v0 = l0 ? f16_residual(feat[k0 - AG_EDGE_LO_SLOT0 + AG_EDGE_LO_FEAT0]) : (k0 < 18 ? feat[k0] : 0.0f);
                    const float v1 = l1 ? f16_residual(feat[k1 - AG_EDGE_LO_SLOT0 + AG_EDGE_LO_FEAT0]) : (k1 < 18 ? feat[k1] : 0.0f);
                    in0[4 * q + p] = h ? v1 : v0;
                }
        }

        typename Prec::Act x, y;
        Prec::set_tile(x, 0, in0);
        dense_first<Prec, AG_EDGE_IN + 1>(P, x, y);
        q.publish();
        dense<Prec, AG_F, true, true>(P, y, x, ZeroInit{});
        dense<Prec, AG_F, true, true>(P, x, y, ZeroInit{});    // relation_encode
        if (a.eterm_half)    // Eterm (q16 table in precision mode 2)
            dense_store<Prec, AG_F, false, true>(P, y, ZeroInit{}, RowStoreQ16Epi{reinterpret_cast<unsigned char *>(a.eterm) + (size_t)e * (2 * AG_FP), h, a.status});
        else
            dense_store<Prec, AG_F, false, true>(P, y, ZeroInit{}, RowStoreEpi{a.eterm + (size_t)e * AG_FP + 4 * h});
        if constexpr (std::is_same_v<Prec, PrecH3>) { h3_report(x.bad, a.status); h3_report(y.bad, a.status); }      // a hidden activation left fp16's range
        q.next();
    }
}

struct EdgeRaw {           // raw gathered inputs of one edge (receiver r, sender s), model.py:220-253
    float ar[2], as[2], gr, gs;
    float pr[AG_NHIS][3], ps[AG_NHIS][3];
    int ri, si, b;
};

__device__ __forceinline__ void edge_gather(const AgFwdArgs &a, int r, int s, EdgeRaw &g)
{
    const int b = r / a.N, ri = r - b * a.N, si = s - b * a.N;
    g.ri = ri; g.si = si; g.b = b;
    g.ar[0] = a.attrs[(size_t)r * 2]; g.ar[1] = a.attrs[(size_t)r * 2 + 1];
    g.as[0] = a.attrs[(size_t)s * 2]; g.as[1] = a.attrs[(size_t)s * 2 + 1];
    // instance 0 of g = cat([p_instance, 0]) (model.py:235); further instances are read in edge_features
    g.gr = (a.n_inst > 0 && ri < a.n_p) ? a.p_instance[((size_t)b * a.n_p + ri) * a.n_inst] : 0.0f;
    g.gs = (a.n_inst > 0 && si < a.n_p) ? a.p_instance[((size_t)b * a.n_p + si) * a.n_inst] : 0.0f;
    const float *st = a.state + (size_t)b * AG_NHIS * a.N * 3;
#pragma unroll
    for (int hh = 0; hh < AG_NHIS; ++hh)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            g.pr[hh][c] = st[((size_t)hh * a.N + ri) * 3 + c];
            g.ps[hh][c] = st[((size_t)hh * a.N + si) * 3 + c];
        }
}

// rel_inputs = [attrs_r | attrs_s | sum|g_r - g_s| | state_res_r - state_res_s | cur_r - cur_s | 1]; lane half h keeps
// features 8q + 4h + p (the B-operand image of k16-steps 0 and 1)
__device__ __forceinline__ void edge_features(const AgFwdArgs &a, const EdgeRaw &g, int h, f32x16 &in0)
{
    float feat[24];
#pragma unroll
    for (int k = 0; k < 24; ++k) feat[k] = 0.0f;
    feat[0] = g.ar[0]; feat[1] = g.ar[1]; feat[2] = g.as[0]; feat[3] = g.as[1];
    float gd = fabsf(g.gr - g.gs);
    for (int ii = 1; ii < a.n_inst; ++ii) {
        const float gr = g.ri < a.n_p ? a.p_instance[((size_t)g.b * a.n_p + g.ri) * a.n_inst + ii] : 0.0f;
        const float gs = g.si < a.n_p ? a.p_instance[((size_t)g.b * a.n_p + g.si) * a.n_inst + ii] : 0.0f;
        gd += fabsf(gr - gs);
    }
    feat[4] = gd;
    feat[AG_EDGE_IN] = 1.0f;   // bias column of relation_encoder.model.0
#pragma unroll
    for (int hh = 0; hh + 1 < AG_NHIS; ++hh)   // state_res = state[:,1:] - state[:,:-1]  (model.py:155)
#pragma unroll
        for (int c = 0; c < 3; ++c) feat[5 + hh * 3 + c] = (g.pr[hh + 1][c] - g.pr[hh][c]) - (g.ps[hh + 1][c] - g.ps[hh][c]);
#pragma unroll
    for (int c = 0; c < 3; ++c) feat[5 + (AG_NHIS - 1) * 3 + c] = g.pr[AG_NHIS - 1][c] - g.ps[AG_NHIS - 1][c];
#pragma unroll
    for (int r16 = 0; r16 < 16; ++r16) in0[r16] = 0.0f;
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int p = 0; p < 4; ++p) in0[4 * q + p] = h ? feat[8 * q + 4 + p] : feat[8 * q + p];
}

}  // namespace

void ag_launch_edge_encode(const AgWeights &w, const AgFwdArgs &a, const AgPath &p, hipStream_t s)
{
    if (a.e_cap <= 0) return;
    const dim3 block(AG_MLP_THREADS);
    const int e_max = a.e_cap + a.self_rows;      // upper bound of the rows this launch encodes (the true count is on the device)
    const int h3_cus = a.max_blocks / AG_MLP_WG_PER_CU > 0 ? a.max_blocks / AG_MLP_WG_PER_CU : 1;      // (max_blocks 1: one CU's worth, not an empty grid)
    switch (p.edge) {
    case AG_EDGE_H3_WS: ag_launch_edge_encode_ws(w, a, p, s); return;
    case AG_EDGE_H3: hipLaunchKernelGGL(edge_encode_kernel<PrecH3>, dim3(grid_for(e_max, h3_cus * AG_H3_WG_PER_CU)), block, 0, s, w, a); return;
    case AG_EDGE_B3: hipLaunchKernelGGL(edge_encode_kernel<PrecB3>, dim3(grid_for(e_max, a.max_blocks)), block, 0, s, w, a); return;
    case AG_EDGE_F32: hipLaunchKernelGGL(edge_encode_kernel<PrecF32>, dim3(grid_for(e_max, a.max_blocks)), block, 0, s, w, a); return;
    }
}
