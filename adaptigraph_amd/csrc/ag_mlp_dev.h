// ag_mlp_dev.h — shared device layer of the fused dense-MLP kernels on the gfx950 matrix cores, three arithmetics:
//   F32 : v_mfma_f32_32x32x2_f32   — exact fp32 (a k-ordered fmaf chain), 157 TFLOP/s class
//   B3  : v_mfma_f32_32x32x16_bf16 — every fp32 operand split x = hi + lo (two bf16), products
//         lo*hi + hi*lo + hi*hi accumulated in fp32 ("bf16x3"): ~2^-17 relative operand error, measured
//         1e-6..6e-6 max-abs on the reference forwards (gate 1e-4), 16/3 = 5.3x the fp32 MFMA rate.
//   H2  : v_mfma_f32_32x32x16_f16  — EDGE stack of precision mode 2 only: activations rounded to one fp16, weights split
//         hi + lo (two fp16), lo*x + hi*x ("fp16x2", struct PrecH3); streaming kernel edge_encode_kernel<PrecH3> and the
//         weight-stationary edge_encode_ws_kernel (the default: weights in registers, activations through LDS).
//
// Replaces the reference's Encoder / Propagator / ParticlePredictor stacks
// (src/dynamics/gnn/model.py:4-60) and the one-hot gathers feeding them (model.py:214-253, 283-295).
//
// Design (CDNA4-first):
//  * One wave owns 32 rows (edges or nodes).  The product is computed TRANSPOSED, D^T = W . X^T: the weight
//    matrix is the MFMA A operand (32 out-features x k), the activations are the B operand (k x 32 rows).
//    The 32x32 accumulator layout then gives lane (j = lane&31, h = lane>>5) the features
//    {32t + 8q + 4h + p} of row j — exactly the B-operand image the NEXT layer needs if its k-loop visits k
//    in that order (the k order of a dot product is free as long as A and B agree; the host packs the
//    weights to match).  So activations never leave registers between layers: bias, ReLU, the bf16 split
//    and the layer-to-layer hand-off are register-only.  No LDS round trip, no transposes.
//  * Weights stream through LDS in 20 KB chunk images (one 32-feature out-tile; bias stored as input column
//    150 against a constant-1 activation so it rides the MFMA chain), double-buffered by LDS-DMA
//    (global_load_lds_dwordx4) issued a full tile ahead, one barrier per tile.
//      F32 image: [32 out][160] floats, 16-byte XOR swizzle (col16 ^= (row>>1)&7) -> conflict-free ds_read_b128
//      B3  image: [10 k16-steps][hi|lo][64 lanes][8 bf16] fragment-major -> every ds_read_b128 is lane-linear
//  * All kernels are persistent (<= 2 workgroups per CU walk the 128-row tiles with a grid stride); the weight
//    ring keeps turning across row tiles.  256-thread workgroups, one wave per SIMD, 2 workgroups per CU.
//
// The kernels live one family per source, each with its launcher: ag_node_encode.hip, ag_edge_encode.hip, ag_edge_encode_ws.hip,
// ag_node_update.hip, ag_node_update_ws.hip, ag_chain.hip.  Everything here is used by at least two of them (PrecH3 is kept beside the
// other two arithmetics); a helper of one family lives in that family's source.
#pragma once
#include "ag_common.h"
#include <type_traits>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

namespace {

// max(x, 0) as ONE op: fp32 bit patterns order like int32 for x >= 0 and every negative float is a negative int, so
// relu(x) = as_float(max(as_int(x), 0)) (v_max_i32).  Through fmaxf / fmed3 the compiler adds a canonicalising
// `v_max_f32 x, x, x` per value.  (Not inline asm: the MFMA -> VALU read hazard is software-managed and the hazard
// recogniser does not look inside asm.)
__device__ __forceinline__ float relu1(float x)
{
    const int b = __float_as_int(x);
    return __int_as_float(b > 0 ? b : 0);
}
// two fp32 -> packed bf16, round-to-nearest-even (v_cvt_pk_bf16_f32), low half = a
__device__ __forceinline__ unsigned cvt_pk_bf16(float a, float b)
{
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

// compile-time loop: f(std::integral_constant<int, I>) for I in [I0, N) — inline-asm immediates need constant expressions
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// Weight-fragment reads of the split-bf16 kernels, issued from inline asm with hand-counted waits.  Left to the
// compiler, the software-pipelined reads of a tile are re-serialised by the machine scheduler in most tiles (one
// register, `s_waitcnt lgkmcnt(0)` after every ds_read: each k16-step then eats a full LDS round trip).  LDS returns
// data in order, so `lgkmcnt(n)` with n = number of fragment reads issued AFTER the wanted pair is exact for them;
// compiler-issued LDS/SMEM traffic in between can only make the wait stricter.  The wait is tied to the fragment
// registers ("+v") so their MFMAs cannot be scheduled above it.
template <int OFF>
__device__ __forceinline__ void lds_read16(bf16x8 &d, unsigned lds_byte_addr)
{
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(lds_byte_addr), "n"(OFF));
}
template <int PENDING>
__device__ __forceinline__ void lds_wait_pair(bf16x8 &a, bf16x8 &b)
{
    static_assert(PENDING >= 0 && PENDING <= 15, "lgkmcnt is 4 bits");
    asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(PENDING));
}
__device__ __forceinline__ unsigned lds_addr_of(const void *p)
{
    return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const void *)p;
}

struct ChunkPipe {
    const float4 *g;   // weight stream (global), chunk k at g + k*AG_CHUNK_F4; the stream is walked cyclically
    int total;         // chunks in the stream (= chunks per row tile)
    int fetch;         // next stream chunk to fetch (wraps at total)
    int buf;           // LDS buffer holding the current chunk (0/1)
    float *lds;        // 2 * AG_CHUNK_FLOATS
    const uint32_t *scales = nullptr;   // PrecH3 only: block scales of the stream's wide units (128 dwords per chunk after the first)
};

// Asynchronous global -> LDS copy of the next weight chunk (global_load_lds_dwordx4: LDS-DMA, no VGPR staging,
// no ds_write in the wave's LDS queue).  Each wave-instruction lands 64 x 16 B at a wave-uniform LDS base (M0), so
// the chunk image is copied linearly: thread t moves float4 t + 256u, u = 0..4.
// Issued from inline asm on purpose: through the builtin, hipcc (ROCm 7.2) treats the DMA as a pending LDS write
// and puts s_waitcnt vmcnt(0) in front of the very next ds_read, i.e. it waits ~1 us for the copy at the top of
// every tile.  With asm the copy stays in flight under the tile's MFMAs and is drained by pipe_wait() right
// before the tile's barrier (cdna_hip_programming.md §5 "Pipelining across barriers").  vmcnt retires in order,
// so compiler-counted waits for its own loads can only over-wait because of these extra entries, never under-wait.
__device__ __forceinline__ void dma16(const void *gsrc, unsigned lds_byte_addr)
{
    asm volatile("s_mov_b32 m0, %0\n\t"
                 "s_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, off"
                 :: "s"(lds_byte_addr), "v"(gsrc) : "memory", "m0");
}

__device__ __forceinline__ void pipe_dma(ChunkPipe &P, int buf)
{
    // The chunk index is laundered through an SGPR so the optimiser cannot prove the (cyclic) address sequence
    // loop-invariant: otherwise LICM hoists ~100 64-bit addresses out of the persistent loop and spills them.
    int f = P.fetch;
    asm volatile("" : "+s"(f));
    const float4 *g = P.g + (size_t)f * AG_CHUNK_F4 + threadIdx.x;
    const unsigned base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void *)P.lds;
    const unsigned dst = __builtin_amdgcn_readfirstlane(base + (buf * AG_CHUNK_FLOATS + (threadIdx.x >> 6) * 256) * 4);
#pragma unroll
    for (int u = 0; u * AG_MLP_THREADS < AG_CHUNK_F4; ++u)        // 1280 float4 per chunk: 5 pieces per wave at 256 threads, 3 / 2 at 512
        if ((u + 1) * AG_MLP_THREADS <= AG_CHUNK_F4 || (int)threadIdx.x + u * AG_MLP_THREADS < AG_CHUNK_F4)   // wave-uniform (64 | 1280)
            dma16(g + AG_MLP_THREADS * u, dst + 16 * AG_MLP_THREADS * u);
    P.fetch = P.fetch + 1 == P.total ? 0 : P.fetch + 1;
}

// Drain the LDS-DMA of the next chunk before the tile's barrier: a full `vmcnt(0)`.  A counted wait that leaves the
// tile's own epilogue stores in flight (vmcnt(S)) measured the same in the split-bf16 kernels (their epilogue is deferred
// by a tile, so the stores are ~1 us old here) and 1.5 % faster in one exact-fp32 kernel, but it is only correct if a
// younger store can never retire before an older load; LLVM's own waitcnt pass does not assume that on gfx9-class
// targets (mixed load/store events make the counter "out of order"), so neither does this code.
__device__ __forceinline__ void pipe_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

__device__ __forceinline__ void pipe_start(ChunkPipe &P)
{
    pipe_dma(P, 0);         // chunk 0
    pipe_wait();
    __syncthreads();
}

// ---- per-tile epilogues (run right after a 32-feature out-tile is finished, so its stores overlap the next
//      tile's MFMAs instead of piling up behind the layer) -------------------------------------------------
struct NoEpi {
    __device__ __forceinline__ void operator()(int, const f32x16 &) const {}
};
// Epilogue stores are unconditional: a row past the valid range writes into the table's padding rows (every table is
// allocated in whole row tiles), which keeps the epilogue branch-free.
struct RowStoreEpi {        // one tile of the row-major [rows][160] table; row = table + row*160 + 4h
    float *row;
    __device__ __forceinline__ void operator()(int ti, const f32x16 &v) const
    {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<float4 *>(row + 32 * ti + 8 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    }
};

// ---- q16: the 16-bit per-edge table of precision mode 2 (format: ag_common.h).  The pieces below are shared by the streaming kernels'
//      epilogue (RowStoreQ16Epi) and the weight-stationary kernel's epilogue pieces, so both write the same bits. ------------------------------
// largest |v| of two values against a running maximum (as a bit pattern; m >= 0).  NANSAFE: compared as unsigned integers — |x| orders
// like one, and inf / NaN sort above every finite value, so a non-finite accumulator ends up in the block exponent and raises the
// status bit (the split-bf16 edge stack has no other check).  Otherwise ONE v_maximum3_f32 with |.| source modifiers (the IEEE-754-2019
// maximum of gfx950: a NaN operand PROPAGATES, inf is kept; until r04 this was v_max3_f32, which drops a NaN — a NaN accumulator that no
// activation check had caught was then stored as 0 with status 0): both flag the same tiles and give the same maximum for finite ones.
// (Inline asm on accumulators: callers read them >= 4 MFMAs after their last write.)
template <bool NANSAFE>
__device__ __forceinline__ unsigned q16_max2(unsigned m, float a, float b)
{
    if constexpr (NANSAFE) {
        const unsigned ua = __float_as_uint(a) & 0x7fffffffu, ub = __float_as_uint(b) & 0x7fffffffu;
        return max(m, max(ua, ub));
    } else {
        unsigned r;
        asm("v_maximum3_f32 %0, %1, |%2|, |%3|" : "=v"(r) : "v"(m), "v"(a), "v"(b));
        return r;
    }
}
// block exponent of an out-tile from the lane's own maximum: the other half of the tile's rows sits in lane j + 32 (v_permlane32_swap)
__device__ __forceinline__ int q16_tile_exp(unsigned m, bool &nonfinite)
{
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 sw = __builtin_amdgcn_permlane32_swap(m, m, false, false);
    m = max(sw.x, sw.y);
    nonfinite = m >= 0x7e800000u;               // biased exponent > AG_Q16_EB_MAX (|v| >= 2^126), inf or NaN: the clamped scale would saturate the tile
    const int eb = (int)(m >> 23);
    return eb < AG_Q16_EB_MIN ? AG_Q16_EB_MIN : (eb > AG_Q16_EB_MAX ? AG_Q16_EB_MAX : eb);
}
__device__ __forceinline__ int q16_inv_scale(int eb) { return 126 - eb; }          // the tile's values are scaled by 2^(126 - eb)
// two values -> packed snorm16 (round to nearest).  The scaling is v_ldexp_f32, one per value, NOT one v_pk_mul_f32 per pair: the packed fp32
// instructions take ~39 cycles beside a busy matrix pipe against ~10 for an ordinary VALU instruction (tools/ubench/valu_beside_mfma.hip), and
// this runs in the shadow of MFMAs in every edge kernel.  (ldexp by 2^k and the multiplication by 2^k round identically: same bits.)
__device__ __forceinline__ unsigned q16_pack(float a, float b, int inv)
{
    typedef short s16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(unsigned, (s16x2)__builtin_amdgcn_cvt_pknorm_i16(__builtin_ldexpf(a, inv), __builtin_ldexpf(b, inv)));
}
// stores of one out-tile of lane (j, h): `row` = table + e * 320 bytes; the lane's 32 bytes start at 64 ti + 32 h.  In tile 4 the last eight
// bytes of the lane's chunk are padding that holds exponent bytes written by OTHER lanes / waves: they are not touched.
__device__ __forceinline__ void q16_store_half(unsigned char *row, int ti, int h, int s, const unsigned (&w)[4])
{
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    unsigned char *p = row + 64 * ti + 32 * h + 16 * s;
    if (ti == 4 && s == 1) *reinterpret_cast<u32x2 *>(p) = u32x2{w[0], w[1]};       // (plain stores: `nt` here costs the edge encoder 4 %, ag_common.h)
    else *reinterpret_cast<u32x4 *>(p) = u32x4{w[0], w[1], w[2], w[3]};
}
__device__ __forceinline__ void q16_store_exp(unsigned char *row, int ti, int h, int eb) { row[ag_q16_exp_byte_offset(ti, h)] = (unsigned char)eb; }

struct RowStoreQ16Epi {     // Eterm as q16 (precision mode 2).  The maximum runs on compiler-visible integer instructions here: `v` comes straight
                            // from builtin MFMAs, and an inline-asm reader gets no MFMA -> VALU wait states from the compiler (the asm version,
                            // hoisted above the tile barrier, read accumulators the last scaled MFMA had not written yet: a block exponent off by
                            // one in 1e-4 of the tiles).  Same result as the float maximum of the weight-stationary kernel for finite tiles.
    unsigned char *row;     // table + e * 320
    int h;
    int *status = nullptr;  // model status word: bit 0 is raised when a tile holds a non-finite value (or one beyond 2^127)
    __device__ __forceinline__ void operator()(int ti, const f32x16 &v) const
    {
        unsigned m = 0;
#pragma unroll
        for (int r = 0; r < 16; r += 2) m = q16_max2<true>(m, v[r], v[r + 1]);
        bool bad;
        const int eb = q16_tile_exp(m, bad);
        const int inv = q16_inv_scale(eb);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            unsigned w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = q16_pack(v[8 * s + 2 * k], v[8 * s + 2 * k + 1], inv);
            q16_store_half(row, ti, h, s, w);
        }
        q16_store_exp(row, ti, h, eb);
        if (bad && status) atomicOr(status, 1);     // AG_STATUS_NONFINITE
    }
};
struct PackStoreEpi {       // same for the fragment-image tables (h, Pn); blk_lane = table + block*5120 + h*128 + j*4
    float *blk_lane;
    __device__ __forceinline__ void operator()(int ti, const f32x16 &v) const
    {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            ag_st_nt(reinterpret_cast<float4 *>(blk_lane + ((ti * 4 + q) * 2) * 128), make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]));
    }
};

// ---- accumulator initialisers ------------------------------------------------------------------------------
struct ZeroInit {
    __device__ __forceinline__ f32x16 operator()(int /*ti*/) const
    {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        return acc;
    }
};
struct ResidInit {  // accumulator := Pn + h, i.e. W_pp[:, :F].enc + b_pp + residual (model.py:36-40,299-301).  Each source is either a
                    // packed (fragment-image) table, pointer already offset to this wave's 32-row block and this lane's (h, j), or — node
                    // de-duplication — a row-major row of a compact table, pointer = row + 4h.
                    // The loads run ahead of their use (r05; loaded where a tile needs them, each of the layer's five tiles waited a full memory
                    // latency two MFMAs into its chain): prefetch() issues h of ALL five out-tiles and Pn of tile 0 at the row tile's top (h's
                    // registers are the ones the layer's output image occupies tile by tile: disjoint live ranges), operator()(ti) adds what
                    // has arrived and issues Pn of tile ti + 1.  Measured -2.6 % (node_update is bound by bytes through L2, not by these
                    // latencies: docs/NEGATIVE_RESULTS.md R5.2).
    const float *pn, *hh;
    bool pn_rowmajor, h_rowmajor;
    mutable f32x16 hraw[AG_NT];       // h of all five out-tiles, issued at the row tile's top
    mutable f32x16 pnext;             // Pn of the NEXT out-tile
    template <bool NT = false>
    __device__ __forceinline__ static void load_tile(const float *p, bool rowmajor, int ti, f32x16 &d)
    {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            // ONE unconditional 16-byte load per quad (address by select; a load under `if (rowmajor)` is split into predicated dword loads)
            const int off = ((ti * 4 + q) * 2) * 128, offr = 32 * ti + 8 * q;
            const bool pad = offr >= 152;                             // row-major rows: columns >= 152 + 4h are not read (zero)
            const float4 *src = reinterpret_cast<const float4 *>(p + (rowmajor ? (pad ? 0 : offr) : off));
            const float4 a = NT ? ag_ld_nt(src) : *src;
            d[4 * q + 0] = a.x; d[4 * q + 1] = a.y; d[4 * q + 2] = a.z; d[4 * q + 3] = a.w;      // (padding quad: zeroed where the tile is consumed, zero_pad)
        }
    }
    __device__ __forceinline__ static void zero_pad(bool rowmajor, int ti, f32x16 &d)      // a VALU op on a loaded value waits for the load: not in load_tile
    {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (32 * ti + 8 * q >= 152 && rowmajor) { d[4 * q + 0] = 0.f; d[4 * q + 1] = 0.f; d[4 * q + 2] = 0.f; d[4 * q + 3] = 0.f; }
    }
    __device__ __forceinline__ void prefetch() const
    {
#pragma unroll
        for (int t = 0; t < AG_NT; ++t) load_tile<true>(hh, h_rowmajor, t, hraw[t]);
        load_tile(pn, pn_rowmajor, 0, pnext);
    }
    __device__ __forceinline__ f32x16 operator()(int ti) const
    {
        f32x16 acc;
        // opaque: without it the scheduler pulls this add up into the PREVIOUS out-tile, right behind the load (to free the register), where it
        // waits for the load — and, vmcnt being in order, for whatever else was issued before it
        asm volatile("" : "+v"(pnext));
        zero_pad(pn_rowmajor, ti, pnext);
        zero_pad(h_rowmajor, ti, hraw[ti]);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = pnext[r] + hraw[ti][r];
        if (ti + 1 < AG_NT) load_tile(pn, pn_rowmajor, ti + 1, pnext);
        return acc;
    }
};

// =====================================================================================================
// Precision policies.  Both expose
//   Act                      register image of a 160-wide activation row block (the MFMA B operands)
//   from_tiles(f32 tiles)    build an Act from fp32 accumulator tiles
//   layer<K,NT,RELU,BIAS>    out-tile loop: acc = init(ti); acc += W_chunk . in; relu; epi(ti, acc);
//                            the finished tile is handed to `sink(ti, acc)` (next layer's Act, or raw tiles)
// K = number of input columns visited (k >= K is zero padding).  With BIAS the layer's bias is input column K of
// the packed weights and the matching activation "feature K" is forced to 1.0, so the bias rides the MFMA chain
// (columns >= AG_F of every activation table are padding, nothing else reads them).
// =====================================================================================================
struct PrecF32 {
    struct Act { f32x16 t[AG_NT]; };
    __device__ __forceinline__ static void set_tile(Act &a, int ti, const f32x16 &v) { a.t[ti] = v; }

    template <int K, int NT, bool RELU, bool BIAS, class Init, class Epi, class Sink>
    __device__ __forceinline__ static void layer(ChunkPipe &P, const Act &in, const Init &init, const Epi &epi, Sink &&sink)
    {
        constexpr int KE = K + (BIAS ? 1 : 0);
        constexpr int PT = (KE + 7) / 8;      // quads (= 4 k-steps = one ds_read_b128 per lane) per tile
        const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
        // per-lane fragment addresses: row i, 16-byte column (8t + 2q + h) ^ ((i >> 1) & 7) (host pre-swizzled)
        const int sw = (i >> 1) & 7;
        int qoff[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) qoff[q] = i * AG_WSTRIDE + 4 * ((2 * q + h) ^ sw);
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
            const float *buf = P.lds + P.buf * AG_CHUNK_FLOATS;
            f32x16 acc = init(ti);      // BEFORE the chunk DMA: vmcnt retires in order, so a wait for a load issued behind the DMA waits for the DMA too
            pipe_dma(P, P.buf ^ 1);
#pragma unroll
            for (int m = 0; m < PT; ++m) {
                const int t = m / 4, q = m % 4;
                const float4 w = *reinterpret_cast<const float4 *>(buf + qoff[q] + 32 * t);
                const float wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int k0 = 32 * t + 8 * q + p;        // column seen by the h = 0 half (h = 1: k0 + 4)
                    if (k0 < KE) {
                        float x = in.t[t][4 * q + p];
                        if (BIAS && (k0 == K || k0 + 4 == K)) x = (h == (k0 == K ? 0 : 1)) ? 1.0f : x;
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[p], x, acc, 0, 0, 0);
                    }
                }
            }
            if (RELU) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = relu1(acc[r]);
            }
            epi(ti, acc);
            sink(ti, acc);
            pipe_wait();
            __syncthreads();
            P.buf ^= 1;
        }
    }

    // First layers (fan-in <= 24): all five out-tiles are packed into ONE chunk ([5][32 rows][32 floats], same
    // 16-byte swizzle), so the layer costs one DMA and one barrier instead of five.
    template <int K, class Sink>
    __device__ __forceinline__ static void layer_first(ChunkPipe &P, const Act &in, Sink &&sink)
    {
        constexpr int PT = (K + 7) / 8;
        static_assert(K <= 32, "compact first layer");
        const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
        const int sw = (i >> 1) & 7;
        const float *buf = P.lds + P.buf * AG_CHUNK_FLOATS;
        pipe_dma(P, P.buf ^ 1);
#pragma unroll
        for (int ti = 0; ti < AG_NT; ++ti) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
            for (int q = 0; q < PT; ++q) {
                const float4 w = *reinterpret_cast<const float4 *>(buf + ti * 1024 + i * 32 + 4 * ((2 * q + h) ^ sw));
                const float wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    if (8 * q + p < K) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[p], in.t[0][4 * q + p], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = relu1(acc[r]);
            sink(ti, acc);
        }
        pipe_wait();
        __syncthreads();
        P.buf ^= 1;
    }
};



struct PrecB3 {
    // step u = 2t + s covers features [16u, 16u+16): lane (j,h) slot e holds feature 16u + 8(e>>2) + 4h + (e&3),
    // which is accumulator register 8s + e of out-tile t — so a finished tile converts in place, no shuffles.
    struct Act { bf16x8 hi[2 * AG_NT], lo[2 * AG_NT]; };
    // hi = bf16(x) (RNE), lo = bf16(x - hi), two values per packed convert: 6 VALU ops per value pair.  (Written on pairs
    // with explicit converts: from per-element `(__bf16)x` the compiler emitted ~3x as many ops, and the relu+split
    // epilogues were co-limiting the kernels with the MFMAs.)
    __device__ __forceinline__ static void set_tile(Act &a, int ti, const f32x16 &v)
    {
#pragma unroll
        for (int s = 0; s < 2; ++s) set_half(a, ti, s, v);
    }
    // k16-step 2ti + s of the next layer's operand = accumulator registers 8s..8s+7 of out-tile ti
    __device__ __forceinline__ static void set_half(Act &a, int ti, int s, const f32x16 &v)
    {
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        u32x4 H, L;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float x0 = v[8 * s + 2 * w], x1 = v[8 * s + 2 * w + 1];
            const unsigned hp = cvt_pk_bf16(x0, x1);
            const float h0 = __uint_as_float(hp << 16), h1 = __uint_as_float(hp & 0xffff0000u);
            H[w] = hp;
            L[w] = cvt_pk_bf16(x0 - h0, x1 - h1);
        }
        a.hi[2 * ti + s] = __builtin_bit_cast(bf16x8, H);
        a.lo[2 * ti + s] = __builtin_bit_cast(bf16x8, L);
    }

    template <int K, int NT, bool RELU, bool BIAS, class Init, class Epi, class Sink>
    __device__ __forceinline__ static void layer(ChunkPipe &P, const Act &in, const Init &init, const Epi &epi, Sink &&sink)
    {
        constexpr int KE = K + (BIAS ? 1 : 0);
        constexpr int NU = (KE + 15) / 16;    // k16-steps per tile
        constexpr int PF = 2;                 // weight fragments are read PF steps ahead of their MFMAs
        const int lane = threadIdx.x & 63, h = lane >> 5;
        // The epilogue of tile ti (ReLU, hi/lo split for the next layer, stores) is DEFERRED into tile ti+1, behind
        // that tile's barrier and fragment prefetch: its ~100 VALU ops then issue in the shadow of tile ti+1's MFMAs
        // instead of sitting between the last MFMA of a tile and the barrier.
        f32x16 prev;
        auto finish = [&](int ti, f32x16 &v) {
            if (RELU) {
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] = relu1(v[r]);
            }
            epi(ti, v);
            sink(ti, v);
        };
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
            const unsigned la = lds_addr_of(P.lds) + (unsigned)(P.buf * AG_CHUNK_FLOATS * 4 + lane * 16);
            f32x16 acc = init(ti);      // BEFORE the chunk DMA: vmcnt retires in order, so a wait for a load issued behind the DMA waits for the DMA too
            pipe_dma(P, P.buf ^ 1);
            bf16x8 wq[PF + 1][2];
            static_for<0, (PF < NU ? PF : NU)>([&](auto U) {
                constexpr int u = decltype(U)::value;
                lds_read16<(2 * u) * 1024>(wq[u][0], la);
                lds_read16<(2 * u + 1) * 1024>(wq[u][1], la);
            });
            if (ti > 0) finish(ti - 1, prev);
            static_for<0, NU>([&](auto U) {
                constexpr int u = decltype(U)::value;
                if constexpr (u + PF < NU) {
                    lds_read16<(2 * (u + PF)) * 1024>(wq[(u + PF) % (PF + 1)][0], la);
                    lds_read16<(2 * (u + PF) + 1) * 1024>(wq[(u + PF) % (PF + 1)][1], la);
                }
                constexpr int ahead = (NU - 1 - u) < PF ? (NU - 1 - u) : PF;     // k16-steps whose reads were issued after step u's
                lds_wait_pair<2 * ahead>(wq[u % (PF + 1)][0], wq[u % (PF + 1)][1]);
                const bf16x8 wh = wq[u % (PF + 1)][0], wl = wq[u % (PF + 1)][1];
                bf16x8 xh = in.hi[u], xl = in.lo[u];
                if constexpr (BIAS && K / 16 == u) {        // feature K = 16u + 8(e>>2) + 4h + (e&3)
                    constexpr int o = K % 16, e = (o >> 3) * 4 + (o & 3), hb = (o >> 2) & 1;
                    if (h == hb) { xh[e] = (__bf16)1.0f; xl[e] = (__bf16)0.0f; }
                }
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, xh, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xl, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, xh, acc, 0, 0, 0);
            });
            prev = acc;
            pipe_wait();
            __syncthreads();
            P.buf ^= 1;
        }
        finish(NT - 1, prev);
    }

    // First layers (fan-in <= 32): the NU k16-steps of all five out-tiles are packed into ONE chunk
    // ([5 tiles][NU][hi|lo][64 lanes][8 bf16]), one DMA and one barrier for the whole layer.
    template <int K, class Sink>
    __device__ __forceinline__ static void layer_first(ChunkPipe &P, const Act &in, Sink &&sink)
    {
        constexpr int NU = (K + 15) / 16;
        static_assert(NU <= 2, "compact first layer");
        const int lane = threadIdx.x & 63;
        const unsigned la = lds_addr_of(P.lds) + (unsigned)(P.buf * AG_CHUNK_FLOATS * 4 + lane * 16);
        pipe_dma(P, P.buf ^ 1);
        // fragments of out-tile ti+1 are read while tile ti's MFMAs run (<= 4*NU reads in flight)
        bf16x8 wq[2][NU][2];
        static_for<0, NU>([&](auto U) {
            constexpr int u = decltype(U)::value;
            lds_read16<(u * 2) * 1024>(wq[0][u][0], la);
            lds_read16<(u * 2 + 1) * 1024>(wq[0][u][1], la);
        });
        static_for<0, AG_NT>([&](auto T) {
            constexpr int ti = decltype(T)::value;
            if constexpr (ti + 1 < AG_NT)
                static_for<0, NU>([&](auto U) {
                    constexpr int u = decltype(U)::value;
                    lds_read16<(((ti + 1) * NU + u) * 2) * 1024>(wq[(ti + 1) & 1][u][0], la);
                    lds_read16<(((ti + 1) * NU + u) * 2 + 1) * 1024>(wq[(ti + 1) & 1][u][1], la);
                });
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            static_for<0, NU>([&](auto U) {
                constexpr int u = decltype(U)::value;
                constexpr int later = (NU - 1 - u) + (ti + 1 < AG_NT ? NU : 0);      // pairs issued after this one
                lds_wait_pair<2 * later>(wq[ti & 1][u][0], wq[ti & 1][u][1]);
                const bf16x8 wh = wq[ti & 1][u][0], wl = wq[ti & 1][u][1];
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, in.hi[u], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, in.lo[u], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, in.hi[u], acc, 0, 0, 0);
            });
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = relu1(acc[r]);
            sink(ti, acc);
        });
        pipe_wait();
        __syncthreads();
        P.buf ^= 1;
    }

};


// ---------------------------------------------------------------------------------------------------------------------
// H3: the arithmetic of the EDGE stack in precision mode 2 — fp16 with byte-sized corrections on the block-scaled fp8 MFMA.
//   weight      W = hi + lo:  hi = fp16(W);  the corrections use e4m3(lo / s_lo) and e4m3(hi / s_hi) with one power-of-two scale per
//               (output row, 32-column input tile) (packed on the host: ag_pack.hip pack_layer_h3)
//   activation  x = x16 + r:  x16 = fp16(x) (RNE);  r8 = e5m2(x - x16) (RNE): ONE byte per value;  x8 = the top byte of x16 (= e5m2, truncated)
//   per 32-column input tile t of an out-tile:
//       acc += hi . x16   two v_mfma_f32_32x32x16_f16 (k16-steps 2t, 2t + 1)
//       acc += s_lo (lo8 . x8) + s_hi (hi8 . r8)   ONE v_mfma_scale_f32_32x32x64_f8f6f4 (A e4m3, B e5m2; its two K blocks are the two terms)
//   i.e. W.x = hi.x16 + lo.x16 + hi.r (+ lo.r ~ 2^-23, dropped) with the two 2^-11-sized terms at 3-4 significant bits.
// History: r02-r03 ran hi.x16 + lo.x16 on twenty fp16 MFMAs per out-tile.  On weights trained by the reference the fp16 rounding of
// the ACTIVATIONS (2^-12 relative, every layer contributing alike) then costs 2-5e-5 of the 1e-4 gate and grows with the predicted motion
// (1.4e-4 at |motion| 0.2 in tools/fuzz_parity.py).  A third fp16 product hi.r fixes that (float64 emulation on the fuzz cases,
// tools/scheme_err.py: 4.9e-5 -> 5.6e-6 with the q16 table) but the chip is POWER-limited under MFMA load (1 630 TFLOP/s of fp16 MFMA
// sustained): thirty MFMAs per out-tile measured 0.91 ms for the edge encoder instead of 0.55.  The block-scaled instruction does K = 64 for
// 1.25 fp16-MFMA-times (tools/ubench/mx_mfma.hip): ten fp16 MFMAs + five scaled ones = 16.25 MFMA-times per out-tile, LESS than the r03
// scheme's 20, for the same 5.6e-6 -> 6.0e-6 emulated deviation.
// RANGE: a hidden activation beyond +-65504 converts to +inf.  Every epilogue keeps the largest fp16 bit pattern it produced
// (`bad`, one packed integer maximum per value pair) and raises status bit 0 when it reaches 0x7c00 (inf / NaN): the overflow is
// reported WHERE it happens, whatever later layers make of it.  For checkpoints with larger activations use precision 1
// (split-bf16, fp32 range).  Measured head-room: the trained goldens rescaled to 64x larger edge-stack activations
// (tests/golden/*act64*, tools/gen_trained.py) still match within the mode's tolerance with status 0.
// FIRST layer of the edge stack: its 17 inputs + bias column use 18 of the 32 K slots of two k16-steps.  Twelve of the inputs are
// position / velocity differences of any size (a tool joined to every cloth particle by connect_tools_all sits metres away: |x| ~ 50
// rounds to fp16 with an error of 0.01).  Spare slots 18..29 carry the fp16 rounding residuals of inputs 5..16 against the same weight
// columns (ag_pack.hip pack_first_layer), so the first layer sees them to 2^-22 on two plain fp16 products (split-fp16 weights).
#define AG_EDGE_LO_SLOT0 (AG_EDGE_IN + 1)       // first residual slot
#define AG_EDGE_LO_FEAT0 (2 * AG_ATTR + 1)      // first input with a residual: the state differences (model.py:241-253)
#define AG_EDGE_LO_COUNT (AG_EDGE_IN - AG_EDGE_LO_FEAT0)
static_assert(AG_EDGE_LO_SLOT0 == 18 && AG_EDGE_LO_FEAT0 == 5 && AG_EDGE_LO_COUNT == 12, "edge_encode_ws_kernel builds slots 18..29 by hand");
__device__ __forceinline__ float f16_residual(float v) { return v - (float)(_Float16)v; }

typedef unsigned h3_u32x4 __attribute__((ext_vector_type(4)));
typedef int h3_i32x8 __attribute__((ext_vector_type(8)));
#define AG_H3_HI_BYTES 10240      // a wide unit's chunk image: [0, 10240) fp16 hi fragments, [10240, 20480) the scaled MFMA's A operands
// two (already ReLU'd) fp32 activations -> the packed fp16 pair and their two residual bytes (into the low or high half of R)
template <bool SIGNED = false>      // SIGNED: the values may be negative (raw first-layer inputs): the range check then ignores the sign bits
__device__ __forceinline__ unsigned h3_pair(float x0, float x1, int &R, bool hi_word, unsigned &bad)
{
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    const f32x2 x = {x0, x1};
    const f16x2 hx = __builtin_convertvector(x, f16x2);
    const unsigned H = __builtin_bit_cast(unsigned, hx);
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    bad = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(u16x2, bad), __builtin_bit_cast(u16x2, SIGNED ? (H & 0x7fff7fffu) : H)));
    // r = x - float(x16), exact: one v_fma_mix_f32 per value (fp16 source read in place; the compiler's own selection is convert + subtract)
    float r0, r1;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(H), "v"(x0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(H), "v"(x1));
    R = hi_word ? __builtin_amdgcn_cvt_pk_bf8_f32(r0, r1, R, true) : __builtin_amdgcn_cvt_pk_bf8_f32(r0, r1, R, false);
    return H;
}
// x8 of an input tile: the top bytes of the sixteen fp16 values of k16-steps 2t (xa) and 2t + 1 (xb), in element order
__device__ __forceinline__ h3_u32x4 h3_top_bytes(const h3_u32x4 &xa, const h3_u32x4 &xb)
{
    h3_u32x4 r;
    r[0] = __builtin_amdgcn_perm(xa[1], xa[0], 0x07050301u);
    r[1] = __builtin_amdgcn_perm(xa[3], xa[2], 0x07050301u);
    r[2] = __builtin_amdgcn_perm(xb[1], xb[0], 0x07050301u);
    r[3] = __builtin_amdgcn_perm(xb[3], xb[2], 0x07050301u);
    return r;
}
__device__ __forceinline__ h3_i32x8 h3_b_operand(const h3_u32x4 &x8, const h3_u32x4 &r8)
{
    return h3_i32x8{(int)x8[0], (int)x8[1], (int)x8[2], (int)x8[3], (int)r8[0], (int)r8[1], (int)r8[2], (int)r8[3]};
}
// status bit 0 when a lane produced an fp16 inf / NaN (bit patterns >= 0x7c00 in either half-word of `bad`)
__device__ __forceinline__ void h3_report(unsigned bad, int *status)
{
    if (((bad + 0x04000400u) & 0x80008000u) && status) atomicOr(status, 1);     // AG_STATUS_NONFINITE
}

struct PrecH3 {
    struct Act { f16x8 v[2 * AG_NT]; h3_u32x4 r8[AG_NT]; unsigned bad = 0; };      // fp16 values by k16-step, residual bytes by input tile
    __device__ __forceinline__ static void set_tile(Act &a, int ti, const f32x16 &v)
    {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            h3_u32x4 H;
            int R[2] = {0, 0};
#pragma unroll
            for (int w = 0; w < 4; ++w) H[w] = h3_pair<true>(v[8 * s + 2 * w], v[8 * s + 2 * w + 1], R[w >> 1], (w & 1) != 0, a.bad);
            a.v[2 * ti + s] = __builtin_bit_cast(f16x8, H);
            a.r8[ti][2 * s] = (unsigned)R[0];
            a.r8[ti][2 * s + 1] = (unsigned)R[1];
        }
    }

    // tile loop as PrecB3::layer (weight ring, deferred epilogue); per input tile two fp16 MFMAs and one block-scaled fp8 MFMA
    template <int K, int NT, bool RELU, bool BIAS, class Init, class Epi, class Sink>
    __device__ __forceinline__ static void layer(ChunkPipe &P, const Act &in, const Init &init, const Epi &epi, Sink &&sink)
    {
        static_assert(K == AG_F && BIAS, "the scaled-MFMA images are packed for 150 inputs + the bias column");
        const int lane = threadIdx.x & 63, h = lane >> 5;
        f32x16 prev;
        auto finish = [&](int ti, f32x16 &v) {
            if (RELU) {
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] = relu1(v[r]);
            }
            epi(ti, v);
            sink(ti, v);
        };
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
            const unsigned la = lds_addr_of(P.lds) + (unsigned)(P.buf * AG_CHUNK_FLOATS * 4 + lane * 16);
            const unsigned lm = lds_addr_of(P.lds) + (unsigned)(P.buf * AG_CHUNK_FLOATS * 4 + AG_H3_HI_BYTES + lane * 32);
            const int cur = P.fetch == 0 ? P.total - 1 : P.fetch - 1;         // stream chunk in P.buf (chunk 0 is the first layer)
            const unsigned sc0 = P.scales[(cur - 1) * 128 + lane], sc1 = P.scales[(cur - 1) * 128 + 64 + lane];
            pipe_dma(P, P.buf ^ 1);
            f32x16 acc = init(ti);
            bf16x8 wq[2][4];          // per input tile: hi fragments of its two k16-steps, the scaled operand's two 16-byte halves
            auto issue = [&](auto T) {
                constexpr int t = decltype(T)::value;
                lds_read16<(2 * t) * 1024>(wq[t & 1][0], la);
                lds_read16<(2 * t + 1) * 1024>(wq[t & 1][1], la);
                lds_read16<t * 2048>(wq[t & 1][2], lm);
                lds_read16<t * 2048 + 16>(wq[t & 1][3], lm);
            };
            issue(std::integral_constant<int, 0>{});
            if (ti > 0) finish(ti - 1, prev);
            static_for<0, AG_NT>([&](auto T) {
                constexpr int t = decltype(T)::value;
                if constexpr (t + 1 < AG_NT) issue(std::integral_constant<int, t + 1>{});
                lds_wait_pair<(t + 1 < AG_NT ? 4 : 0)>(wq[t & 1][0], wq[t & 1][1]);
                lds_wait_pair<(t + 1 < AG_NT ? 4 : 0)>(wq[t & 1][2], wq[t & 1][3]);
                f16x8 xa = in.v[2 * t], xb = in.v[2 * t + 1];
                if constexpr (K / 32 == t) {        // bias column: feature K = 16u + 8(e>>2) + 4h + (e&3) := 1.0 (its residual byte is 0: the feature is padding)
                    constexpr int u = K / 16, o = K % 16, e = (o >> 3) * 4 + (o & 3), hb = (o >> 2) & 1;
                    if (h == hb) { if constexpr (u & 1) xb[e] = (_Float16)1.0f; else xa[e] = (_Float16)1.0f; }
                }
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wq[t & 1][0]), xa, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wq[t & 1][1]), xb, acc, 0, 0, 0);
                const h3_u32x4 a0 = __builtin_bit_cast(h3_u32x4, wq[t & 1][2]), a1 = __builtin_bit_cast(h3_u32x4, wq[t & 1][3]);
                const h3_i32x8 A = h3_b_operand(a0, a1);
                const h3_i32x8 B = h3_b_operand(h3_top_bytes(__builtin_bit_cast(h3_u32x4, xa), __builtin_bit_cast(h3_u32x4, xb)), in.r8[t]);
                acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A, B, acc, 0, 1, t & 3, (int)(t < 4 ? sc0 : sc1), 0, 0x7f7f7f7f);
            });
            prev = acc;
            pipe_wait();
            __syncthreads();
            P.buf ^= 1;
        }
        finish(NT - 1, prev);
    }

    // narrow first layer: two plain fp16 products on split-fp16 weights (its inputs carry their own residuals in spare K slots, see above)
    template <int K, class Sink>
    __device__ __forceinline__ static void layer_first(ChunkPipe &P, const Act &in, Sink &&sink)
    {
        constexpr int NU = (K + 15) / 16;
        static_assert(NU <= 2, "compact first layer");
        const int lane = threadIdx.x & 63;
        const unsigned la = lds_addr_of(P.lds) + (unsigned)(P.buf * AG_CHUNK_FLOATS * 4 + lane * 16);
        pipe_dma(P, P.buf ^ 1);
        bf16x8 wq[2][NU][2];
        static_for<0, NU>([&](auto U) {
            constexpr int u = decltype(U)::value;
            lds_read16<(u * 2) * 1024>(wq[0][u][0], la);
            lds_read16<(u * 2 + 1) * 1024>(wq[0][u][1], la);
        });
        static_for<0, AG_NT>([&](auto T) {
            constexpr int ti = decltype(T)::value;
            if constexpr (ti + 1 < AG_NT)
                static_for<0, NU>([&](auto U) {
                    constexpr int u = decltype(U)::value;
                    lds_read16<(((ti + 1) * NU + u) * 2) * 1024>(wq[(ti + 1) & 1][u][0], la);
                    lds_read16<(((ti + 1) * NU + u) * 2 + 1) * 1024>(wq[(ti + 1) & 1][u][1], la);
                });
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            static_for<0, NU>([&](auto U) {
                constexpr int u = decltype(U)::value;
                constexpr int later = (NU - 1 - u) + (ti + 1 < AG_NT ? NU : 0);
                lds_wait_pair<2 * later>(wq[ti & 1][u][0], wq[ti & 1][u][1]);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wq[ti & 1][u][1]), in.v[u], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, wq[ti & 1][u][0]), in.v[u], acc, 0, 0, 0);
            });
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = relu1(acc[r]);
            sink(ti, acc);
        });
        pipe_wait();
        __syncthreads();
        P.buf ^= 1;
    }
};


// layer -> next Act
template <class Prec, int K, bool RELU, bool BIAS, class Init, class Epi = NoEpi>
__device__ __forceinline__ void dense(ChunkPipe &P, const typename Prec::Act &in, typename Prec::Act &out, const Init &init,
                                      const Epi &epi = Epi{})
{
    Prec::template layer<K, AG_NT, RELU, BIAS>(P, in, init, epi, [&](int ti, const f32x16 &v) { Prec::set_tile(out, ti, v); });
}
// narrow first layer (ReLU, bias column already in the input features) -> next Act
template <class Prec, int K>
__device__ __forceinline__ void dense_first(ChunkPipe &P, const typename Prec::Act &in, typename Prec::Act &out)
{
    Prec::template layer_first<K>(P, in, [&](int ti, const f32x16 &v) { Prec::set_tile(out, ti, v); });
}
// layer whose output is only stored (by `epi`)
template <class Prec, int K, bool RELU, bool BIAS, class Init, class Epi>
__device__ __forceinline__ void dense_store(ChunkPipe &P, const typename Prec::Act &in, const Init &init, const Epi &epi)
{
    Prec::template layer<K, AG_NT, RELU, BIAS>(P, in, init, epi, [](int, const f32x16 &) {});
}

__device__ __forceinline__ void load_rowmajor(const float *row, f32x16 (&v)[AG_NT], int h)
{
#pragma unroll
    for (int t = 0; t < AG_NT; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (32 * t + 8 * q < 152) x = *reinterpret_cast<const float4 *>(row + 32 * t + 8 * q + 4 * h);
            v[t][4 * q] = x.x; v[t][4 * q + 1] = x.y; v[t][4 * q + 2] = x.z; v[t][4 * q + 3] = x.w;
        }
}

// `agg` as q16 rows (option "agg_q16", ag_common.h): lane (j, h) of an MFMA kernel needs, per out-tile t, the features 32t + 8q + 4h + p — the sixteen
// CONTIGUOUS 16-bit positions 32t + 16h .. + 15 of row j (two 16-byte loads instead of four) — and the row's exponent bytes 280..284 (one 8-byte load).
__device__ __forceinline__ float agg_q16_tile_scale(const uint2 &ex, int t) { return ag_q16u_scale(t < 4 ? (int)((ex.x >> (8 * t)) & 0xffu) : (int)(ex.y & 0xffu)); }
__device__ __forceinline__ void agg_q16_decode8(const int4 &w, float sc, float (&x)[8]) { ag_q16u_decode8(w, sc, x); }

#define AG_LDS_DECL __shared__ __attribute__((aligned(16))) float lds[2 * AG_CHUNK_FLOATS]; __shared__ int s_next_tile[2];

// Row tiles are CLAIMED from a per-launch counter instead of walked with a static grid stride: the two workgroups that
// share a CU do not progress at the same rate (issue arbitration is oldest-first, so the workgroup launched second runs
// ~40 % slower per row tile, s_memtime trace), and with a static split the early finishers leave their CU half empty for
// the tail.  The atomic is issued together with the row tile's first loads (whose wait it shares) and the claimed index
// travels through LDS under the tile's own barriers, so the queue costs no extra round trip or barrier.
struct TileQueue {
    int *ctr, *slot;
    int tile, par, claimed;
    __device__ __forceinline__ TileQueue(int *c, int *s) : ctr(c), slot(s), tile(blockIdx.x), par(0), claimed(0) {}
    __device__ __forceinline__ void claim() { if (threadIdx.x == 0) claimed = ctr ? (int)gridDim.x + atomicAdd(ctr, 1) : tile + (int)gridDim.x; }
    __device__ __forceinline__ void publish() { if (threadIdx.x == 0) slot[par] = claimed; }   // >= 1 barrier before next()
    __device__ __forceinline__ void next() { tile = slot[par]; par ^= 1; }                      // after the row tile's last barrier
};

template <class Prec> __device__ __forceinline__ const float4 *pick(const float4 *f32, const float4 *b3);
template <> __device__ __forceinline__ const float4 *pick<PrecF32>(const float4 *f32, const float4 *) { return f32; }
template <> __device__ __forceinline__ const float4 *pick<PrecB3>(const float4 *, const float4 *b3) { return b3; }
template <> __device__ __forceinline__ const float4 *pick<PrecH3>(const float4 *, const float4 *b3) { return b3; }   // (the caller passes the fp16 image)

// Maps the sender column to compact node rows (node-encoder de-duplication, ag_node_encode.hip): the body of send_remap_kernel there and of
// the rider workgroups of edge_node_tab_kernel (ag_edge_encode_ws.hip).
__device__ __forceinline__ void send_remap_body(const AgFwdArgs &a, int block, int nblocks)
{
    const int E = a.row_ptr[a.B * a.N];
    const bool ovf = *a.ovf != 0;                // the call overflowed the compact tables: round 0 gathers the full-size sender table by node id
    // four edges per thread and trip with their loads batched (index, then row, then store): a plain strided loop orders every trip's two dependent
    // loads behind the previous trip's store
    const int stride = nblocks * 256;
    for (int e0 = block * 256 + threadIdx.x; e0 < E; e0 += 4 * stride) {
        int sd[4], rw[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) sd[u] = e0 + u * stride < E ? a.edge_send[e0 + u * stride] : 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) rw[u] = ovf ? sd[u] : a.node_row[sd[u]];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (e0 + u * stride < E) a.send_c[e0 + u * stride] = rw[u];
    }
}

// End of a round of the weight-stationary kernels (edge_encode_ws_kernel, node_update_nws_kernel): LDS writes of this wave landed, then the workgroup barrier.  NOT __syncthreads(): its workgroup-scope fence also
// drains vmcnt, i.e. it would wait at every round for the Eterm stores (and gather loads) issued a few hundred cycles earlier.
__device__ __forceinline__ void ws_round_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

}  // namespace

// workgroups of a persistent launch over `rows` rows: one per row tile, at most max_blocks
static inline int grid_for(int rows, int max_blocks)
{
    const int tiles = (rows + AG_ROWS_PER_BLOCK - 1) / AG_ROWS_PER_BLOCK;
    return tiles < max_blocks ? (tiles > 0 ? tiles : 1) : max_blocks;
}
