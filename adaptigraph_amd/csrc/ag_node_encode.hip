// ag_node_encode.hip — node encoder and its de-duplication passes (shared device layer: ag_mlp_dev.h)
#include "ag_block_dev.h"
#include "ag_mlp_dev.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Node encoder + pstep-invariant node terms.
//   enc = Encoder([attrs | phys | action])                      model.py:168-195, 268
//   h0  = enc                                                     model.py:269
//   Pn  = W_pp[:, :F] . enc + b_pp     (first column block of particle_propagator, model.py:300)
//   Hr  = W_rp[:, F:2F] . h0,  Hs = W_rp[:, 2F:3F] . h0   (receiver / sender column blocks of
//          relation_propagator applied at NODE level instead of per edge, model.py:283-289)
// ---------------------------------------------------------------------------------------------
// Node-encoder de-duplication, step 1: one WAVE per sample walks the sample's nodes in index order and maps every node to a compact
// table row: the first AG_DEDUP_REPS distinct input rows [attrs | phys (0 for tool slots) | action] (bitwise comparison) become shared
// rows, a node that matches none of them gets a private row.  New rows are appended to the encoder's work list (global counter: the
// ORDER of the list does not matter, a row's MFMA chain does not depend on its position in a row tile).
__global__ __launch_bounds__(256) void node_classify_kernel(AgFwdArgs a)
{
    __shared__ unsigned rep[4][AG_DEDUP_REPS][AG_NODE_IN_MAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + wave;
    if (b >= a.B) return;                                  // wave-uniform; the kernel has no workgroup-level synchronisation
    const int N = a.N, A = AG_ATTR, Pd = a.phys_dim, D = A + Pd + 3;
    const int base = b * AG_DEDUP_REPS;          // this sample's shared rows
    int nrep = 0;
    constexpr int kPre = 8;                                // 64-node slices whose inputs are fetched together (one memory round trip per 512 nodes)
    for (int s0 = 0; s0 < N; s0 += 64 * kPre) {
        unsigned vv[kPre][AG_NODE_IN_MAX];
#pragma unroll
        for (int u = 0; u < kPre; ++u) {
            const int i = s0 + 64 * u + lane;
            const bool valid = i < N;
            const size_t g = (size_t)b * N + (valid ? i : 0);
#pragma unroll
            for (int k = 0; k < AG_NODE_IN_MAX; ++k) {
                float x = 0.0f;
                if (k < A) x = a.attrs[g * A + k];
                else if (k < A + Pd) x = (valid && i < a.n_p) ? a.phys[(size_t)b * Pd + (k - A)] : 0.0f;
                else if (k < D) x = a.action[g * 3 + (k - A - Pd)];
                vv[u][k] = __float_as_uint(x);
            }
        }
#pragma unroll
        for (int u = 0; u < kPre; ++u) {
            const int i = s0 + 64 * u + lane;
            if (s0 + 64 * u >= N) break;                       // wave-uniform
            const bool valid = i < N;
            const size_t g = (size_t)b * N + (valid ? i : 0);
            unsigned (&v)[AG_NODE_IN_MAX] = vv[u];
            int match = -1;
            for (int r = 0; r < nrep; ++r) {
                bool eq = true;
#pragma unroll
                for (int k = 0; k < AG_NODE_IN_MAX; ++k) eq = eq && v[k] == rep[wave][r][k];
                if (eq && match < 0) match = r;
            }
            while (nrep < AG_DEDUP_REPS) {
                const unsigned long long un = __ballot(valid && match < 0);
                if (!un) break;
                const int leader = __ffsll((long long)un) - 1;
                bool eq = true;
#pragma unroll
                for (int k = 0; k < AG_NODE_IN_MAX; ++k) {
                    const unsigned lv = (unsigned)__shfl((int)v[k], leader);
                    if (lane == 0) rep[wave][nrep][k] = lv;
                    eq = eq && v[k] == lv;
                }
                if (valid && match < 0 && eq) match = nrep;
                if (lane == leader) {
                    const int slot = atomicAdd(a.enc_count, 1);
                    if (slot < a.rows_c) { a.enc_row[slot] = base + nrep; a.enc_src[slot] = (int)g; }
                    else *a.ovf = 1;
                }
                ++nrep;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();
            }
            int row = base + match;
            const unsigned long long priv = __ballot(valid && match < 0);       // rows of their own: one pair of atomics per wave, not per lane
            if (priv) {
                const int first = __ffsll((long long)priv) - 1;
                int slot0 = 0, prow0 = 0;
                if (lane == first) { slot0 = atomicAdd(a.enc_count, __popcll(priv)); prow0 = atomicAdd(a.priv_count, __popcll(priv)); }
                slot0 = __shfl(slot0, first);
                prow0 = __shfl(prow0, first);
                if (valid && match < 0) {
                    const int rank = ballot_rank(priv, lane);
                    row = a.shared_rows + prow0 + rank;                      // private rows follow the B x AG_DEDUP_REPS shared ones
                    const bool fits = row < a.rows_c && slot0 + rank < a.rows_c;
                    if (!fits) { *a.ovf = 1; row = a.rows_c - 1; }           // budget exhausted: this call runs without de-duplication (every consumer tests ovf)
                    else { a.enc_row[slot0 + rank] = row; a.enc_src[slot0 + rank] = (int)g; }
                }
            }
            if (valid) a.node_row[g] = row;
        }
    }
}

// step 2 (independent of the encoders): the first round's sender gathers go to compact rows, so the sender column is mapped once
// (send_remap_body: ag_mlp_dev.h)
__global__ __launch_bounds__(256) void send_remap_kernel(AgFwdArgs a) { send_remap_body(a, blockIdx.x, gridDim.x); }

template <class Prec, bool DEDUP>
__global__ __launch_bounds__(AG_MLP_THREADS, AG_MLP_WG_PER_CU) void node_encode_kernel(AgWeights w, AgFwdArgs a)
{
    AG_LDS_DECL
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5, wave = tid >> 6;
    // compact encoder: nothing to do when the call overflowed the compact tables; per-node encoder of a de-duplicated call (a.ovf set): only then
    if (a.ovf && (*a.ovf != 0) == DEDUP) return;
    const int Mn = DEDUP ? *a.enc_count : a.B * a.N;      // rows to encode: the work list of node_classify_kernel, or every node
    const int ntiles = (Mn + AG_ROWS_PER_BLOCK - 1) / AG_ROWS_PER_BLOCK;
    if ((int)blockIdx.x >= ntiles) return;                // (de-duplicated: a handful of row tiles)
    ChunkPipe P{pick<Prec>(w.node_encode, w.node_encode_b3), 26, 0, 0, lds};
    pipe_start(P);
    TileQueue q(nullptr, s_next_tile);   // ~4 row tiles per workgroup: nothing to balance, static stride
#pragma unroll 1
    while (q.tile < ntiles) {
        const int tile = q.tile;
        q.claim();
        const int g = tile * AG_ROWS_PER_BLOCK + wave * 32 + j;
        const bool valid = g < Mn;
        const int gc = valid ? (DEDUP ? a.enc_src[g] : g) : 0;        // a node that carries this row's inputs
        const int b = gc / a.N, i = gc - b * a.N;

        // p_inputs = [attrs(2) | physics_param (0 for tool slots) | action(3) | 1 (bias column)], feature k = 4h + p
        f32x16 in0;
#pragma unroll
        for (int r = 0; r < 16; ++r) in0[r] = 0.0f;
        {
            const int A = AG_ATTR, Pd = a.phys_dim;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int k = 4 * h + p;
                float v = 0.0f;
                if (k < A) v = a.attrs[(size_t)gc * A + k];
                else if (k < A + Pd) v = i < a.n_p ? a.phys[(size_t)b * Pd + (k - A)] : 0.0f;
                else if (k < A + Pd + 3) v = a.action[(size_t)gc * 3 + (k - A - Pd)];
                else if (k == A + Pd + 3) v = 1.0f;   // bias column of particle_encoder.model.0
                in0[p] = v;
            }
        }
        typename Prec::Act x, y;
        Prec::set_tile(x, 0, in0);
        dense_first<Prec, AG_NODE_IN_MAX>(P, x, y);
        q.publish();
        dense<Prec, AG_F, true, true>(P, y, x, ZeroInit{});
        if constexpr (DEDUP) {
            // compact row-major tables at the row the work item names; lanes past the list write dump rows [rows_c, rows_c + 128)
            const size_t row = valid ? (size_t)a.enc_row[g] : (size_t)a.rows_c + wave * 32 + j;
            const size_t rowoff = row * AG_FP + 4 * h;
            dense<Prec, AG_F, true, true>(P, x, y, ZeroInit{}, RowStoreEpi{a.h0c + rowoff});                 // y = particle_encode = h0
            dense_store<Prec, AG_F, false, true>(P, y, ZeroInit{}, RowStoreEpi{a.pnc + rowoff});             // Pn
            dense_store<Prec, AG_F, false, false>(P, y, ZeroInit{}, RowStoreEpi{a.hrc + rowoff});            // Hr (round 0 reads it through node_row)
            dense_store<Prec, AG_F, false, false>(P, y, ZeroInit{}, RowStoreEpi{a.hsc + rowoff});            // Hs (round 0 gathers it through send_c)
        } else {
            const size_t blk = (size_t)(tile * AG_MLP_WAVES + wave) * AG_PACK_BLOCK + h * 128 + j * 4;
            const size_t rowoff = (size_t)g * AG_FP + 4 * h;   // own row even when past Mn (padding rows)
            dense<Prec, AG_F, true, true>(P, x, y, ZeroInit{}, PackStoreEpi{a.h + blk});               // y = particle_encode = h0
            dense_store<Prec, AG_F, false, true>(P, y, ZeroInit{}, PackStoreEpi{a.pn + blk});           // Pn
            dense_store<Prec, AG_F, false, false>(P, y, ZeroInit{}, RowStoreEpi{a.hr + rowoff});  // Hr
            dense_store<Prec, AG_F, false, false>(P, y, ZeroInit{}, RowStoreEpi{a.hs + rowoff});  // Hs
        }
        q.next();
    }
}

}  // namespace

void ag_launch_send_remap(const AgFwdArgs &a, hipStream_t s)
{
    if (a.e_cap <= 0) return;
    const int blocks = (a.e_cap + 255) / 256;
    hipLaunchKernelGGL(send_remap_kernel, dim3(blocks < 4096 ? blocks : 4096), dim3(256), 0, s, a);
}

void ag_launch_node_encode(const AgWeights &w, const AgFwdArgs &a, hipStream_t s)
{
    if (a.dedup) {
        hipLaunchKernelGGL(node_classify_kernel, dim3((a.B + 3) / 4), dim3(256), 0, s, a);
        const dim3 gridc(grid_for(a.rows_c, a.max_blocks)), blockc(AG_MLP_THREADS);      // worst case every row is private; workgroups past the list exit
        if (a.precision == AG_PREC_B3) hipLaunchKernelGGL((node_encode_kernel<PrecB3, true>), gridc, blockc, 0, s, w, a);
        else hipLaunchKernelGGL((node_encode_kernel<PrecF32, true>), gridc, blockc, 0, s, w, a);
        return;
    }
    ag_launch_node_encode_fallback(w, a, s);      // (the per-node encoder)
}

void ag_launch_node_encode_fallback(const AgWeights &w, const AgFwdArgs &a, hipStream_t s)
{
    const dim3 grid(grid_for(a.B * a.N, a.max_blocks)), block(AG_MLP_THREADS);
    if (a.precision == AG_PREC_B3) hipLaunchKernelGGL((node_encode_kernel<PrecB3, false>), grid, block, 0, s, w, a);
    else hipLaunchKernelGGL((node_encode_kernel<PrecF32, false>), grid, block, 0, s, w, a);
}
