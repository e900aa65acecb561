// ag_edge_encode_ws.hip — weight-stationary edge encoder (shared device layer: ag_mlp_dev.h)
#include "ag_mlp_dev.h"

namespace {

// =====================================================================================================================
// Weight-STATIONARY edge encoder (precision mode 2, arithmetic PrecH3; the default there, ag_set_option("edge_stationary", 0) selects the streaming kernel).
//
// The streaming kernels (ag_edge_encode.hip) re-read the whole 320 KB weight image from L2 through LDS for every 128 edges: 2 560 B of
// L2->LDS traffic and 2 560 B of LDS fragment reads per edge, against 388 B of HBM traffic.  Here the dataflow is turned around:
//  * ONE 512-thread workgroup per CU, two waves per SIMD, 256 registers per lane.  The four layers are cut into 15 "units" of one
//    32-feature out-tile (30 matrix instructions per 32 edges) plus the narrow first layer (5 tiles x 4): a wave owns TWO units and keeps
//    their A operands (fp16 hi fragments + the scaled MFMA's [e4m3 lo | e4m3 hi] operands: 80 registers per unit) in REGISTERS for the
//    whole launch — the compiler splits a 256-register wave 128 + 128, so a wave's first unit and the fp16 half of its second sit in
//    accumulation registers (the MFMA reads its A operand from there directly), the rest and all accumulators in architectural ones:
//        wave 0, 1: RE1 tiles {0,1}, {2,3} + first-layer tile 0 / 1       wave 2, 3: RE2 tiles {0,1}, {2,3} + first-layer tile 2 / 3
//        wave 4, 5: We tiles {0,1}, {2,3}                                  wave 6: RE1 tile 4, RE2 tile 4
//        wave 7: We tile 4, per-edge input gather, first-layer tile 4          (waves w and w + 4 share a SIMD)
//  * 32-edge blocks flow through the waves as a software pipeline; a layer's 160 x 32 activation block is handed over through LDS
//    as a SET of two images already in the B-operand layout of the next layer (lane (j, h) writes exactly the bytes lane (j, h) of
//    the consumer reads): 10 KB of fp16 values and 5 KB of e5m2 residual bytes (PrecH3: x = x16 + r8).  One barrier per ROUND.  Block i:
//    indices / node rows / features in rounds i .. i + 2 (wave 7), first layer in round i + 3, RE1 i + 4, RE2 i + 5 (its pairs hand the
//    block over at the start of round i + 6), We i + 7 (its pairs store the rows at the start of round i + 8).  Rings: RE1 and RE2 inputs
//    two blocks, We input three; LDS 131 KB.
//  * What a second wave per SIMD buys (tools/ubench/mx_lone.hip, valu_beside_mfma.hip; profiles/r04_edge_ws8_trace.txt): a wave does not
//    overlap its own VALU work with its own matrix instructions, and while one wave of a SIMD issues MFMAs back to back the other's
//    instructions take ~10 cycles each (packed fp32 VALU 39: none are used here).  So a wave runs its 30 MFMAs, then its epilogues as plain
//    code, and the two waves of a SIMD are kept in OPPOSITE halves of their rounds: waves 2-5 start a round with the epilogue of the
//    accumulators they computed in the previous round, their partners start with their MFMAs.  Until r04 the kernel ran four waves of 512
//    registers with every epilogue cut into micro-chores pinned into MFMA shadows: 0.72 ms against 0.61 for this one.
//  * A dependent MFMA issued straight after its predecessor uses the pipe's accumulate path; results of asm MFMAs are not interlocked against
//    compiler-placed readers (ws_settle), a VALU-written B operand needs two wait states (s_nop 1), and the scaled MFMA reads its eight B
//    registers over several passes after issue (two register sets by tile parity).
//  * Each accumulator sees hi.x16 of k16-steps 2t, 2t + 1 and the scaled correction product by ascending input tile t, so results equal
//    edge_encode_kernel<PrecH3> bit for bit.
// =====================================================================================================================
#define AG_WS_IMG 10240          // bytes of one fp16 activation image: [10 k16-steps][64 lanes][8 fp16]
#define AG_WS_RES 5120           // bytes of its residual image: [10 k16-steps][64 lanes][8 e5m2]
#define AG_WS_SET (AG_WS_IMG + AG_WS_RES)
#define AG_WS_IN0 2048           // first-layer input image: 2 k16-steps
#define AG_WS_SLOTS 3

// A (layer, out-tile) unit's A operands: fp16 hi fragments by k16-step, the block-scaled MFMA's operands [e4m3 lo | e4m3 hi] by input tile, and
// the unit's block scales (lane (i, h): h = 0 the lo scales, h = 1 the hi scales; sc0 = tiles 0..3 by byte, sc1 byte 0 = tile 4)
struct WsUnit { f16x8 hi[10]; h3_i32x8 mx[AG_NT]; unsigned sc0, sc1; };
typedef h3_u32x4 ws_u32x4;
typedef int ws_i32x2 __attribute__((ext_vector_type(2)));

// ACC: keep the unit in the accumulation-register half of the file; a wave holds three units (240 registers) there.
template <bool ACC, bool ACC_MX = ACC>
__device__ __forceinline__ void ws_load_unit(WsUnit &W, const float4 *chunk, const uint32_t *scales, int lane)
{
    typedef int i32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int u = 0; u < 10; ++u) W.hi[u] = *reinterpret_cast<const f16x8 *>(chunk + u * 64 + lane);
#pragma unroll
    for (int t = 0; t < AG_NT; ++t) {
        const i32x4 a = *reinterpret_cast<const i32x4 *>(chunk + AG_H3_HI_BYTES / 16 + (t * 64 + lane) * 2);
        const i32x4 b = *reinterpret_cast<const i32x4 *>(chunk + AG_H3_HI_BYTES / 16 + (t * 64 + lane) * 2 + 1);
        W.mx[t] = h3_i32x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    }
    W.sc0 = scales[lane];
    W.sc1 = scales[64 + lane];
    // opaque values (after ALL the loads: the asm is a use, and a use waits for its load): they must live in registers and cannot be re-loaded
    // inside the persistent loop
#pragma unroll
    for (int u = 0; u < 10; ++u) { if (ACC) asm volatile("" : "+a"(W.hi[u])); else asm volatile("" : "+v"(W.hi[u])); }
#pragma unroll
    for (int t = 0; t < AG_NT; ++t) { if (ACC_MX) asm volatile("" : "+a"(W.mx[t])); else asm volatile("" : "+v"(W.mx[t])); }
    asm volatile("" : "+v"(W.sc0), "+v"(W.sc1));
}
__device__ __forceinline__ unsigned lds_addr3(const __attribute__((address_space(3))) void *p) { return (unsigned)(uintptr_t)p; }
template <int N>
__device__ __forceinline__ void ws_wait2(bf16x8 &a, bf16x8 &b) { asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N)); }
template <int N>
__device__ __forceinline__ void ws_wait3(bf16x8 &a, bf16x8 &b, bf16x8 &c)
{
    static_assert(N >= 0 && N <= 15, "lgkmcnt is 4 bits");
    asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(a), "+v"(b), "+v"(c) : "n"(N));
}

// acc (+)= W . x from inline asm: accumulator and B operand in architectural registers, A operand where the unit lives
template <bool ACC, bool FIRST>
__device__ __forceinline__ void ws_mfma(f32x16 &acc, const f16x8 &w, const bf16x8 &x)
{
    if constexpr (FIRST) {
        if constexpr (ACC) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=&v"(acc) : "a"(w), "v"(x));
        else asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=&v"(acc) : "v"(w), "v"(x));
    } else {
        if constexpr (ACC) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "a"(w), "v"(x));
        else asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(x));
    }
}
// the two fp16 MFMAs of an input tile on one accumulator, back to back (the second takes the pipe's accumulate path), as ONE statement: hipcc pads
// every asm statement whose outputs the next instruction reads with a wait state of its own
template <bool ACC, bool FIRST>
__device__ __forceinline__ void ws_mfma2(f32x16 &acc, const f16x8 &w0, const f16x8 &w1, const bf16x8 &x0, const bf16x8 &x1)
{
    if constexpr (FIRST) {
        if constexpr (ACC) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %3, 0\n\tv_mfma_f32_32x32x16_f16 %0, %2, %4, %0" : "=&v"(acc) : "a"(w0), "a"(w1), "v"(x0), "v"(x1));
        else asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %3, 0\n\tv_mfma_f32_32x32x16_f16 %0, %2, %4, %0" : "=&v"(acc) : "v"(w0), "v"(w1), "v"(x0), "v"(x1));
    } else {
        if constexpr (ACC) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %3, %0\n\tv_mfma_f32_32x32x16_f16 %0, %2, %4, %0" : "+v"(acc) : "a"(w0), "a"(w1), "v"(x0), "v"(x1));
        else asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %3, %0\n\tv_mfma_f32_32x32x16_f16 %0, %2, %4, %0" : "+v"(acc) : "v"(w0), "v"(w1), "v"(x0), "v"(x1));
    }
}
// acc += 2^(sa - 127) 2^(sb - 127) A8 . B8 over two 32-element K blocks: A e4m3 (cbsz 0), B e5m2 (blgp 1); the A scale is byte SEL of `sa` in the
// lanes of the half with the block's number, the B scale byte 0 of `sb`
// (the statement opens with the two wait states a VALU-written B operand needs before an MFMA reads it: the byte permutes that build it may be
// scheduled anywhere above)
template <bool ACC, int SEL>
__device__ __forceinline__ void ws_mfma_mx(f32x16 &acc, const h3_i32x8 &a, const h3_i32x8 &b, unsigned sa, unsigned sb)
{
#define AG_MX(OPS) \
    do { if constexpr (ACC) asm volatile("s_nop 1\n\tv_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 " OPS " cbsz:0 blgp:1" : "+v"(acc) : "a"(a), "v"(b), "v"(sa), "v"(sb)); \
         else asm volatile("s_nop 1\n\tv_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 " OPS " cbsz:0 blgp:1" : "+v"(acc) : "v"(a), "v"(b), "v"(sa), "v"(sb)); } while (0)
    if constexpr (SEL == 0) AG_MX("op_sel:[0,0,0] op_sel_hi:[0,0,0]");
    else if constexpr (SEL == 1) AG_MX("op_sel:[1,0,0] op_sel_hi:[0,0,0]");
    else if constexpr (SEL == 2) AG_MX("op_sel:[0,0,0] op_sel_hi:[1,0,0]");
    else AG_MX("op_sel:[1,0,0] op_sel_hi:[1,0,0]");
#undef AG_MX
}

// Epilogue of the hidden layers in eight pieces.  M = 0..7 of out-tile T: half S = M >> 2, output dword M & 3 (two accumulator values):
// ReLU, packed fp16 convert, largest-pattern tracking, the two residual bytes (h3_pair); the fourth dword stores the consumer's 16 bytes
// of k16-step 2T + S (bias column: feature 150 := 1.0) and its 8 residual bytes (residual image: [5 input tiles][64 lanes][16 bytes]).
struct WsEpi { ws_u32x4 H; int R[4]; unsigned bad; };
typedef __attribute__((address_space(3))) unsigned char lds_u8;      // LDS pointers stay in their address space: a store is one ds_write with an
                                                                     // immediate offset (through a generic pointer: two address instructions each)
template <int T, int M>
__device__ __forceinline__ void ws_act_micro(const f32x16 &acc, WsEpi &E, lds_u8 *set_lane, int h)
{
    constexpr int S = M >> 2, w = M & 3;
    unsigned untracked = 0;
    E.H[w] = h3_pair<false>(relu1(acc[8 * S + 2 * w]), relu1(acc[8 * S + 2 * w + 1]), E.R[2 * S + (w >> 1)], (w & 1) != 0, untracked);
    // largest fp16 pattern so far (inf / NaN = an overflow of this layer): the values are >= 0, so the float maximum is the integer one; NaN propagates
    if constexpr ((w & 1) == 1) asm("v_pk_maximum3_f16 %0, %0, %1, %2" : "+v"(E.bad) : "v"(E.H[w - 1]), "v"(E.H[w]));
    if constexpr (w == 3) {
        if constexpr (T == 4 && S == 1) {           // feature 150 = 16*9 + 6: element e = 2 of the h = 1 half (its residual byte is 0: the feature is padding)
            if (h == 1) E.H[1] = (E.H[1] & 0xffff0000u) | 0x3c00u;
        }
        *reinterpret_cast<__attribute__((address_space(3))) ws_u32x4 *>(set_lane + (2 * T + S) * 1024) = E.H;
        if constexpr (S == 1)
            *reinterpret_cast<__attribute__((address_space(3))) ws_u32x4 *>(set_lane + AG_WS_IMG + T * 1024) = ws_u32x4{(unsigned)E.R[0], (unsigned)E.R[1], (unsigned)E.R[2], (unsigned)E.R[3]};
    }
}
// We: one out-tile of the q16 table in seven chores (format and helpers: RowStoreQ16Epi, ag_mlp_dev.h): 0, 1 the lane's maximum over its 16 values,
// 2 the tile exponent (partner half by v_permlane32_swap) and its byte, 3..6 two packed converts each, 4 and 6 store 16 (8) bytes.
// Branch-free on purpose: a store under `if (block is valid)` made the compiler sink the whole tile's converts into the conditional block.
// Rows of blocks outside the launch go to 32 dump rows behind the table (the 16-bit table uses half of its fp32-sized allocation).
struct WsQ16 { unsigned m; int eb; int inv; unsigned w[4]; unsigned nonfinite; };
template <int T, int C>
__device__ __forceinline__ void ws_q16_chore(const f32x16 &acc, WsQ16 &Q, unsigned char *row, int h)
{
    static_assert(C >= 0 && C < 7, "seven chores per out-tile");
    if constexpr (C == 0) {
        Q.m = 0;
#pragma unroll
        for (int r = 0; r < 8; r += 2) Q.m = q16_max2<false>(Q.m, acc[r], acc[r + 1]);
    } else if constexpr (C == 1) {
#pragma unroll
        for (int r = 8; r < 16; r += 2) Q.m = q16_max2<false>(Q.m, acc[r], acc[r + 1]);
    } else if constexpr (C == 2) {
        bool nf;
        Q.eb = q16_tile_exp(Q.m, nf);
        Q.inv = q16_inv_scale(Q.eb);
        Q.nonfinite |= nf ? 1u : 0u;
        q16_store_exp(row, T, h, Q.eb);
    } else {
        constexpr int s = (C - 3) >> 1, k0 = 2 * ((C - 3) & 1);
        Q.w[k0] = q16_pack(acc[8 * s + 2 * k0], acc[8 * s + 2 * k0 + 1], Q.inv);
        Q.w[k0 + 1] = q16_pack(acc[8 * s + 2 * k0 + 2], acc[8 * s + 2 * k0 + 3], Q.inv);
        if constexpr (((C - 3) & 1) == 1) q16_store_half(row, T, h, s, Q.w);
    }
}

// Per-node inputs of the edge features: ag_edge_node_tab_row (ag_common.h), one thread per node.
// Workgroups past the node range (de-duplicated calls) map the sender column to compact rows for round 0's reduce (send_remap_body): one small
// launch per model step instead of two.  (In ag_rollout both ride the edge builder's launches instead — AgEdgeArgs riders — and this kernel is
// launched for what they did not cover: ag_forward, the brute-force edge path, the CU-partitioned rollout.)
__global__ __launch_bounds__(256) void edge_node_tab_kernel(AgFwdArgs a, int nb_tab)
{
    if ((int)blockIdx.x >= nb_tab) { send_remap_body(a, (int)blockIdx.x - nb_tab, (int)gridDim.x - nb_tab); return; }
    ag_edge_node_tab_row(a.state, a.attrs, a.p_instance, a.n_inst, a.n_p, a.B, a.N, a.edge_node_tab, a.status, blockIdx.x * 256 + threadIdx.x,
                         a.self_rows ? (long long)a.self_class_row0 : -1);
}

// First layer of one 32-edge block for out-tiles [T0, T0 + NT): per tile 2 k16-steps x (lo, hi) fp16 MFMAs with the A fragments read from the
// LDS image `wf` (this lane's 16 bytes of fragment 0; [5 tiles][2 steps][hi | lo][64 lanes][8 fp16]) and the block's input image at `lin` — NT
// independent chains, two plain products (the inputs carry their own residuals in spare K slots).  slot(IC<m>) runs after MFMA m = g * NT + t
// (g = 0..3: (step 0, lo), (step 0, hi), (step 1, lo), (step 1, hi)), m = 0 .. 4 NT - 1.
template <int T0, int NT, class Slot>
__device__ __forceinline__ void ws_first_layer(f32x16 (&accF)[NT], unsigned lin, unsigned wf, Slot &&slot)
{
    bf16x8 xq[2], fq[2][NT];
    __builtin_amdgcn_s_setprio(3);      // as in ws_phase
    lds_read16<0>(xq[0], lin);
    lds_read16<1024>(xq[1], lin);
    static_for<0, NT>([&](auto T) { constexpr int t = decltype(T)::value; lds_read16<(((T0 + t) * 2 + 0) * 2 + 1) * 1024>(fq[0][t], wf); });
    static_for<0, 4>([&](auto GG) {
        constexpr int g = decltype(GG)::value, u = g >> 1;
        if constexpr (g < 3) {
            constexpr int nu = (g + 1) >> 1, nhl = 1 - ((g + 1) & 1);
            static_for<0, NT>([&](auto T) { constexpr int t = decltype(T)::value; lds_read16<(((T0 + t) * 2 + nu) * 2 + nhl) * 1024>(fq[(g + 1) & 1][t], wf); });
        }
        static_for<0, NT>([&](auto T) {
            constexpr int t = decltype(T)::value;
            constexpr int later = (NT - 1 - t) + (g < 3 ? NT : 0);
            ws_wait2<later>(fq[g & 1][t], xq[u]);
            ws_mfma<false, (g == 0)>(accF[t], __builtin_bit_cast(f16x8, fq[g & 1][t]), xq[u]);
            slot(std::integral_constant<int, g * NT + t>{});
            __builtin_amdgcn_sched_barrier(0);
        });
    });
    __builtin_amdgcn_s_setprio(0);
}

#define AG_WS_LAG_F 3
#define AG_WS_LAG_1 4
#define AG_WS_LAG_2 5
#define AG_WS_LAG_3 7      // the RE2 pairs hand their block over at the start of the NEXT round
// An asm MFMA's result is not interlocked against the VALU instructions the compiler places after it: 16 passes + 4 states for the scaled one
__device__ __forceinline__ void ws_settle(f32x16 &a) { asm volatile("s_nop 15\n\ts_nop 7" : "+v"(a)); }
__device__ __forceinline__ void ws_settle(f32x16 &a, f32x16 &b) { asm volatile("s_nop 15\n\ts_nop 7" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ void ws_settle(f32x16 &a, f32x16 &b, f32x16 &c) { asm volatile("s_nop 15\n\ts_nop 7" : "+v"(a), "+v"(b), "+v"(c)); }
// One MFMA phase of the eight-wave kernel: accumulators 0 .. NA-1 run units W[0 .. NA-1] on ONE input set (la: this lane's 16 bytes of k16-step 0).
// The compiler splits a 256-register wave into 128 + 128: a wave's first unit and the fp16 half of its second live in accumulation registers
// (NACC2 half-units: fp16 fragments of unit k = half-unit 2k, its scaled-MFMA operands = half-unit 2k + 1), the rest in architectural ones.
// No operand ring: the partner wave's matrix work covers the LDS latency.  The next tile's reads are issued after the fp16 MFMAs that read the
// current fragments and land during the scaled MFMAs; the scaled MFMA's B operand (read over several passes after issue) alternates between two
// register sets by tile parity.
template <int NA, int NACC2, int U0 = 0, int NW, int NACCS>
__device__ __forceinline__ void ws_phase(const WsUnit (&W)[NW], f32x16 (&acc)[NACCS], unsigned la)
{
    bf16x8 xa, xb, r;
    // The instruction arbiter serves the OLDER wave of a SIMD first: without a raised priority the younger wave's MFMAs wait behind every VALU
    // instruction of the older wave's epilogue (kernel 0.676 -> 0.615 ms with it)
    __builtin_amdgcn_s_setprio(3);
    lds_read16<0>(xa, la);
    lds_read16<1024>(xb, la);
    lds_read16<AG_WS_IMG>(r, la);
    const unsigned one = 0x7f7f7f7fu;      // E8M0 127 = 2^0: the activations' bytes are plain e5m2 numbers
    h3_i32x8 Bq[2];
    static_for<0, AG_NT>([&](auto TT) {
        constexpr int t = decltype(TT)::value;
        ws_wait3<0>(xa, xb, r);
        h3_i32x8 &B = Bq[t & 1];
        B = h3_b_operand(h3_top_bytes(__builtin_bit_cast(h3_u32x4, xa), __builtin_bit_cast(h3_u32x4, xb)), __builtin_bit_cast(h3_u32x4, r));
        static_for<0, NA>([&](auto KK) {
            constexpr int k = decltype(KK)::value;
            ws_mfma2<(2 * (U0 + k) < NACC2), (t == 0)>(acc[U0 + k], W[U0 + k].hi[2 * t], W[U0 + k].hi[2 * t + 1], xa, xb);
        });
        if constexpr (t + 1 < AG_NT) {
            lds_read16<(2 * t + 2) * 1024>(xa, la);
            lds_read16<(2 * t + 3) * 1024>(xb, la);
            lds_read16<AG_WS_IMG + (t + 1) * 1024>(r, la);
        }
        static_for<0, NA>([&](auto KK) {
            constexpr int k = decltype(KK)::value;
            ws_mfma_mx<(2 * (U0 + k) + 1 < NACC2), (t & 3)>(acc[U0 + k], W[U0 + k].mx[t], B, t < 4 ? W[U0 + k].sc0 : W[U0 + k].sc1, one);
        });
        if constexpr (t > 0) asm volatile("" :: "v"(Bq[(t - 1) & 1]));      // the previous tile's operand is released only now
    });
    asm volatile("" :: "v"(Bq[(AG_NT - 1) & 1]));
    __builtin_amdgcn_s_setprio(0);
}
template <int T>
__device__ __forceinline__ void ws_hidden_tile(const f32x16 &acc, WsEpi &E, lds_u8 *set_lane, int h)
{
    static_for<0, 8>([&](auto MM) { ws_act_micro<T, decltype(MM)::value>(acc, E, set_lane, h); });
}
template <int T>
__device__ __forceinline__ void ws_table_tile(const f32x16 &acc, WsQ16 &Q, unsigned char *row, int h)
{
    static_for<0, 7>([&](auto CC) { ws_q16_chore<T, decltype(CC)::value>(acc, Q, row, h); });
}

__global__ __launch_bounds__(512, 1) void edge_encode_ws_kernel(AgWeights w, AgFwdArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_act[7][AG_WS_SET];                // input sets of RE1, RE2 (rings of two blocks), We (ring of three)
    __shared__ __attribute__((aligned(16))) unsigned char s_in0[AG_WS_SLOTS][AG_WS_IN0];      // first-layer inputs
    __shared__ __attribute__((aligned(16))) float4 s_wf[AG_CHUNK_F4];                         // first-layer fragments [5 tiles][2 steps][hi|lo][64][8]
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int E = ag_edges(a) + a.self_rows;      // (+ the class rows of elided self-loops: their endpoints are the class rows of the per-node table)
    if (a.edge_counter && blockIdx.x == 0 && tid == 0) atomicAdd(a.edge_counter, (unsigned long long)E);
    const int nblk = (E + 31) / 32;
    if ((int)blockIdx.x >= nblk) return;
    const int n_i = (nblk - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;      // blocks of this workgroup: blockIdx + i * gridDim
    const int rounds = n_i + AG_WS_LAG_3 + 1;      // + 1: the We pairs store a block's rows at the start of the next round
    const float4 *ws = w.edge_encode_h2;
    for (int i = tid; i < AG_CHUNK_F4; i += 512) s_wf[i] = ws[i];
    for (int i = tid; i < (int)(sizeof(s_act) / 16); i += 512) reinterpret_cast<float4 *>(&s_act[0][0])[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = tid; i < (int)(sizeof(s_in0) / 16); i += 512) reinterpret_cast<float4 *>(&s_in0[0][0])[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const size_t e_pad = ag_edge_rows_pad(a.e_cap);        // rows of the table (fwd_layout); dump rows start here
    auto gblock = [&](int i) { return (int)blockIdx.x + i * (int)gridDim.x; };
    auto slot_of = [](int i) { return (i + 4 * AG_WS_SLOTS) % AG_WS_SLOTS; };                 // i >= -12
    // this lane's 16 bytes of k16-step 0 of the fp16 image of input set `layer` (0: RE1, 1: RE2, 2: We), block i (i >= -8)
    auto img = [&](int layer, int i) -> lds_u8 * { return (lds_u8 *)&s_act[layer < 2 ? 2 * layer + ((i + 8) & 1) : 4 + (i + 9) % 3][lane * 16]; };
    auto eterm_row = [&](int i) {
        const size_t e = ((i >= 0 && i < n_i) ? (size_t)gblock(i) * 32 : e_pad) + j;
        return reinterpret_cast<unsigned char *>(a.eterm) + e * (2 * AG_FP);
    };
    WsEpi Ep{{0u, 0u, 0u, 0u}, {0, 0, 0, 0}, 0u};
    const uint32_t *wsc = w.edge_scale_h3;      // block scales of unit k (stream chunk 1 + k): wsc + 128 k
    auto load_unit = [&](WsUnit &U, int chunk) { ws_load_unit<true, true>(U, ws + (size_t)chunk * AG_CHUNK_F4, wsc + (size_t)(chunk - 1) * 128, lane); };
    auto load_unit2 = [&](WsUnit &U, int chunk) { ws_load_unit<true, false>(U, ws + (size_t)chunk * AG_CHUNK_F4, wsc + (size_t)(chunk - 1) * 128, lane); };
    auto noop = [](auto) {};
    const unsigned wf = lds_addr_of(s_wf) + lane * 16;

    // hidden layer L (1: RE1, 2: RE2), out-tiles T0 and T0 + 1; then first-layer tile TF (-1: none)
    auto hidden_pair = [&](auto LL, auto TT, auto FF, auto DD) {
        constexpr int L = decltype(LL)::value, T0 = decltype(TT)::value, TF = decltype(FF)::value;
        constexpr bool DEFER = decltype(DD)::value;      // the round starts with the PREVIOUS round's epilogue (the SIMD partner starts with its MFMAs)
        WsUnit W[2];
        load_unit(W[0], 1 + 5 * (L - 1) + T0);
        load_unit2(W[1], 2 + 5 * (L - 1) + T0);
        __syncthreads();
        f32x16 acc[2];
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[0][q] = acc[1][q] = 0.0f;
#pragma unroll 1
        for (int r = 0; r < rounds; ++r) {
            const int i = r - (AG_WS_LAG_F + L);
            if constexpr (DEFER) {
                lds_u8 *outp = img(L, i - 1);
                ws_hidden_tile<T0>(acc[0], Ep, outp, h);
                ws_hidden_tile<T0 + 1>(acc[1], Ep, outp, h);
            }
            const unsigned la = lds_addr3(img(L - 1, i));
            ws_phase<2, 3>(W, acc, la);
            ws_settle(acc[0], acc[1]);
            if constexpr (!DEFER) {
                lds_u8 *out = img(L, i);
                ws_hidden_tile<T0>(acc[0], Ep, out, h);
                ws_hidden_tile<T0 + 1>(acc[1], Ep, out, h);
            }
            if constexpr (TF >= 0) {
                const int i0 = r - AG_WS_LAG_F;
                f32x16 accF[1];
                ws_first_layer<TF, 1>(accF, lds_addr_of(&s_in0[slot_of(i0)][lane * 16]), wf, noop);
                ws_settle(accF[0]);
                ws_hidden_tile<TF>(accF[0], Ep, img(0, i0), h);
            }
            ws_round_barrier();
        }
    };
    // We tiles T0 and T0 + 1 and first-layer tile TF.  The round STARTS with the previous round's table epilogue (the SIMD partner starts with its
    // MFMAs: the two waves stay in opposite halves of their rounds), then the first-layer tile, then this round's MFMAs.
    auto table_pair = [&](auto FF, auto TT) {
        constexpr int TF = decltype(FF)::value, T0 = decltype(TT)::value;
        WsUnit W[2];
        load_unit(W[0], 11 + T0);
        load_unit2(W[1], 12 + T0);
        __syncthreads();
        f32x16 acc[2], accF[1];
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[0][q] = acc[1][q] = 0.0f;
        WsQ16 Q{0u, AG_Q16_EB_MIN, 0, {0u, 0u, 0u, 0u}, 0u};
#pragma unroll 1
        for (int r = 0; r < rounds; ++r) {
            const int i0 = r - AG_WS_LAG_F, i3 = r - AG_WS_LAG_3;
            unsigned char *rowp = eterm_row(i3 - 1);
            ws_table_tile<T0>(acc[0], Q, rowp, h);
            ws_table_tile<T0 + 1>(acc[1], Q, rowp, h);
            if constexpr (TF >= 0) {
                ws_first_layer<TF, 1>(accF, lds_addr_of(&s_in0[slot_of(i0)][lane * 16]), wf, noop);
                ws_settle(accF[0]);
                ws_hidden_tile<TF>(accF[0], Ep, img(0, i0), h);
            }
            const unsigned la = lds_addr3(img(2, i3));
            ws_phase<2, 3>(W, acc, la);
            ws_settle(acc[0], acc[1]);
            ws_round_barrier();
        }
        if (Q.nonfinite && a.status) atomicOr(a.status, 1);
    };

    if (wave == 0) hidden_pair(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, std::false_type{});
    else if (wave == 1) hidden_pair(std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{}, std::integral_constant<int, 1>{}, std::false_type{});
    else if (wave == 2) hidden_pair(std::integral_constant<int, 2>{}, std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{}, std::true_type{});
    else if (wave == 3) hidden_pair(std::integral_constant<int, 2>{}, std::integral_constant<int, 2>{}, std::integral_constant<int, 3>{}, std::true_type{});
    else if (wave == 4) table_pair(std::integral_constant<int, -1>{}, std::integral_constant<int, 0>{});
    else if (wave == 5) table_pair(std::integral_constant<int, -1>{}, std::integral_constant<int, 2>{});
    else if (wave == 6) {
        // ---------------------------------------------------------------- RE1 tile 4 and RE2 tile 4: two input sets, one after the other
        WsUnit W[1], W1[1];
        load_unit(W[0], 1 + 4);
        load_unit2(W1[0], 6 + 4);
        __syncthreads();
        f32x16 accA[1], accB[1];
#pragma unroll 1
        for (int r = 0; r < rounds; ++r) {
            const int i1 = r - AG_WS_LAG_1, i2 = r - AG_WS_LAG_2;
            const unsigned la1 = lds_addr3(img(0, i1)), la2 = lds_addr3(img(1, i2));
            ws_phase<1, 2>(W, accA, la1);
            ws_settle(accA[0]);
            ws_hidden_tile<4>(accA[0], Ep, img(1, i1), h);
            ws_phase<1, 1>(W1, accB, la2);
            ws_settle(accB[0]);
            ws_hidden_tile<4>(accB[0], Ep, img(2, i2), h);
            ws_round_barrier();
        }
    } else {
        // ---------------------------------------------------------------- per-edge input gather, first-layer tiles 2-4, We tile 4
        WsUnit W[1];
        load_unit(W[0], 11 + 4);
        __syncthreads();
        f32x16 accF[1], acc[1];
        WsQ16 Q{0u, AG_Q16_EB_MIN, 0, {0u, 0u, 0u, 0u}, 0u};
        // three blocks in flight: edge indices (this round) -> the two 64-byte node rows (next round) -> features (the round after)
        int er = 0, es = 0;                // indices of block r (loaded in round r, used in round r + 1)
        float4 R[4], S[4];                 // receiver / sender rows of block r - 1 (loaded in round r, used in round r + 1)
#pragma unroll
        for (int q = 0; q < 4; ++q) R[q] = S[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
        auto pk = [](float x0, float x1) { const f32x2 v = {x0, x1}; return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2)); };
        const float4 *tab = reinterpret_cast<const float4 *>(a.edge_node_tab);
        static_assert(AG_NHIS == 4 && AG_EDGE_IN == 17, "edge_node_tab rows and the feature pieces are laid out for four history frames");
#pragma unroll 1
        for (int r = 0; r < rounds; ++r) {
            const int i0 = r - AG_WS_LAG_F, i3 = r - AG_WS_LAG_3;
            {   // We tile 4 first: the SIMD partner (an RE2 pair) starts its round with an epilogue
                const unsigned la = lds_addr3(img(2, i3));
                ws_phase<1, 2>(W, acc, la);
                ws_settle(acc[0]);
                ws_table_tile<4>(acc[0], Q, eterm_row(i3), h);
            }
            {   // features of block r - 2 from the rows loaded last round: [attrs_r | attrs_s | |g_r - g_s| | row_r[4:16] - row_s[4:16] | 1];
                // lane half h keeps slots 8q + 4h + c -> B-operand image of k16-step 0 (features 0..15) and 1 (slot 16: feature 16, 17: the bias
                // 1.0, 18..29: the fp16 residuals of features 5..16, f16_residual; the same values in the same slots as edge_encode_kernel<PrecH3>)
                float feat[24];
#pragma unroll
                for (int k = 0; k < 24; ++k) feat[k] = 0.0f;
                feat[0] = R[0].x; feat[1] = R[0].y; feat[2] = S[0].x; feat[3] = S[0].y; feat[4] = fabsf(R[0].z - S[0].z); feat[AG_EDGE_IN] = 1.0f;
                feat[5] = R[1].x - S[1].x; feat[6] = R[1].y - S[1].y; feat[7] = R[1].z - S[1].z; feat[8] = R[1].w - S[1].w;
                feat[9] = R[2].x - S[2].x; feat[10] = R[2].y - S[2].y; feat[11] = R[2].z - S[2].z; feat[12] = R[2].w - S[2].w;
                feat[13] = R[3].x - S[3].x; feat[14] = R[3].y - S[3].y; feat[15] = R[3].z - S[3].z; feat[16] = R[3].w - S[3].w;
                ws_u32x4 X, X1;
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int c2 = 0; c2 < 2; ++c2)
                        X[2 * q + c2] = pk(h ? feat[8 * q + 4 + 2 * c2] : feat[8 * q + 2 * c2], h ? feat[8 * q + 5 + 2 * c2] : feat[8 * q + 1 + 2 * c2]);
                // slots 16, 17 | 20, 21 and 18, 19 | 22, 23, then 24, 25 | 28, 29 and 26, 27 | 30, 31   (h = 0 | h = 1; slots 30, 31 stay zero)
                X1[0] = h ? pk(f16_residual(feat[7]), f16_residual(feat[8])) : pk(feat[16], feat[AG_EDGE_IN]);
                X1[1] = h ? pk(f16_residual(feat[9]), f16_residual(feat[10])) : pk(f16_residual(feat[5]), f16_residual(feat[6]));
                X1[2] = h ? pk(f16_residual(feat[15]), f16_residual(feat[16])) : pk(f16_residual(feat[11]), f16_residual(feat[12]));
                X1[3] = h ? 0u : pk(f16_residual(feat[13]), f16_residual(feat[14]));
                *reinterpret_cast<ws_u32x4 *>(&s_in0[slot_of(r - 2)][lane * 16]) = X;
                *reinterpret_cast<ws_u32x4 *>(&s_in0[slot_of(r - 2)][lane * 16 + 1024]) = X1;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) { R[q] = tab[(unsigned)er * 4u + q]; S[q] = tab[(unsigned)es * 4u + q]; }      // node rows of block r - 1
            {                                                                                                          // edge indices of block r
                const int e = (r < n_i ? gblock(r) : 0) * 32 + j;
                const bool valid = r < n_i && e < E;
                er = valid ? a.edge_recv[e] : 0;
                es = valid ? a.edge_send[e] : 0;
            }
            ws_first_layer<4, 1>(accF, lds_addr_of(&s_in0[slot_of(i0)][lane * 16]), wf, noop);
            ws_settle(accF[0]);
            ws_hidden_tile<4>(accF[0], Ep, img(0, i0), h);
            ws_round_barrier();
        }
        if (Q.nonfinite && a.status) atomicOr(a.status, 1);
    }
    h3_report(Ep.bad, a.status);
}

}  // namespace

// AgPath::edge == AG_EDGE_H3_WS of ag_launch_edge_encode (ag_edge_encode.hip): one workgroup per CU, 32-edge blocks
void ag_launch_edge_encode_ws(const AgWeights &w, const AgFwdArgs &a, const AgPath &p, hipStream_t s)
{
    const int blocks = (a.e_cap + a.self_rows + 31) / 32, slots = a.ws_blocks;      // (row bound as in ag_launch_edge_encode)
    const int nb_tab = a.tab_done ? 0 : (a.B * a.N + 255) / 256;
    const int nb_map = p.dedup && !a.remap_done ? ((a.e_cap + 1023) / 1024 < 4096 ? (a.e_cap + 1023) / 1024 : 4096) : 0;      // four edges per thread
    if (nb_tab + nb_map > 0) hipLaunchKernelGGL(edge_node_tab_kernel, dim3(nb_tab + nb_map), dim3(256), 0, s, a, nb_tab);
    hipLaunchKernelGGL(edge_encode_ws_kernel, dim3(blocks < slots ? blocks : (slots > 0 ? slots : 1)), dim3(512), 0, s, w, a);   // (always eight waves, whatever AG_MLP_THREADS is)
}
