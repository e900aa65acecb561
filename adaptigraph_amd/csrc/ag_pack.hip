// ag_pack.hip — a model's weights as the chunk images the kernels read (layouts: ag_common.h, and above each packer), and the number formats
// they are rounded to.  Host arithmetic only: no HIP runtime call, so a CPU test can check every bit (tests/test_pack_host.py).
#include "ag_pack.h"
#include "ag_common.h"

#include <cmath>
#include <cstring>

namespace ag_pack {
uint16_t bf16_rne(float x)   // round-to-nearest-even, as v_cvt_pk_bf16_f32 does (finite inputs)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
// split-fp16 weight pair (edge stack of precision mode 2): hi = fp16(v) (RNE), lo = fp16(v - hi), subnormals kept
void f16_split(float v, uint16_t &hi, uint16_t &lo)
{
    const _Float16 h = (_Float16)v;
    const _Float16 l = (_Float16)(v - (float)h);
    memcpy(&hi, &h, 2);
    memcpy(&lo, &l, 2);
}
// OCP e4m3fn (1-4-3, bias 7, subnormals, max 448, no inf), round-to-nearest-even, saturating: the A-operand format of the block-scaled MFMA
uint8_t e4m3_rne(float v)
{
    const uint8_t sign = std::signbit(v) ? 0x80 : 0;
    const float a = fabsf(v);
    if (!(a > 0.0f)) return sign;
    if (a >= 448.0f) return sign | 0x7e;
    int e;
    (void)frexpf(a, &e);
    e -= 1;                                            // a = f * 2^e, f in [1, 2)
    if (e < -6) {                                      // subnormal: multiples of 2^-9 (8 of them reach the smallest normal, whose pattern is 8)
        return sign | (uint8_t)nearbyintf(ldexpf(a, 9));
    }
    int m = (int)nearbyintf((ldexpf(a, -e) - 1.0f) * 8.0f);
    if (m == 8) { m = 0; e += 1; }
    const int bits = ((e + 7) << 3) | m;
    return sign | (uint8_t)(bits > 0x7e ? 0x7e : bits);
}

float bf16_to_f32(uint16_t b)
{
    const uint32_t u = (uint32_t)b << 16;
    float x;
    memcpy(&x, &u, 4);
    return x;
}
}  // namespace ag_pack
using namespace ag_pack;

namespace {

// Where column k of out-row i sits in a fragment image [k16-step u][64 lanes (i, h)][8 slots e] of 16-bit values (ag_common.h, "B3"):
// the 512-slot block of step u = k / 16, and in it lane * 8 + e with lane = 32 h + i, column k = 16u + 8(e>>2) + 4h + (e&3)
struct FragSlot { int u, at; };
inline FragSlot frag_slot(int k, int i)
{
    const int r = k & 15, h = (r >> 2) & 1, e = (r >> 3) * 4 + (r & 3), lane = h * 32 + i;
    return {k >> 4, lane * 8 + e};
}

// Narrow first layer (fan-in K <= 24, + bias column K): all five out-tiles in ONE chunk image.
//   F32: [5 tiles][32 rows][32 floats], 16-byte XOR swizzle;  B3: [5 tiles][NU steps][hi|lo][64 lanes][8 bf16]
// b3: 0 = fp32 image, 1 = split-bf16 fragment image, 2 = split-fp16 fragment image (same layout)
// lo_feat0 >= 0 (split-fp16 edge stack): image columns K + 1 + i repeat input column lo_feat0 + i, i < K - lo_feat0 — the kernels put the
// fp16 rounding residual of that input there (ag_mlp_dev.h, f16_residual), so the first layer multiplies hi + lo of those inputs.
void pack_first_layer(std::vector<float> &dst, int b3, const float *W, int K, int n_out, const float *bias, int lo_feat0 = -1)
{
    const size_t base = dst.size();
    dst.resize(base + AG_CHUNK_FLOATS, 0.0f);
    float *c = dst.data() + base;
    uint16_t *cb = reinterpret_cast<uint16_t *>(c);
    const int NU = (K + 1 + 15) / 16;
    for (int ti = 0; ti < AG_NT; ++ti)
        for (int i = 0; i < 32; ++i) {
            const int o = 32 * ti + i;
            if (o >= n_out) continue;
            const int k_end = lo_feat0 >= 0 ? K + 1 + (K - lo_feat0) : K + 1;
            for (int k = 0; k < k_end; ++k) {
                const float v = k < K ? W[(size_t)o * K + k] : (k == K ? bias[o] : W[(size_t)o * K + (k - K - 1 + lo_feat0)]);
                if (!b3) {
                    c[ti * 1024 + i * 32 + 4 * ((k >> 2) ^ ((i >> 1) & 7)) + (k & 3)] = v;
                } else {
                    const FragSlot f = frag_slot(k, i);
                    uint16_t hi = bf16_rne(v), lo = bf16_rne(v - bf16_to_f32(hi));
                    if (b3 == 2) f16_split(v, hi, lo);
                    cb[(size_t)((ti * NU + f.u) * 2 + 0) * 512 + f.at] = hi;
                    cb[(size_t)((ti * NU + f.u) * 2 + 1) * 512 + f.at] = lo;
                }
            }
        }
}

// Append one layer as n_tiles chunk images (AG_CHUNK_FLOATS floats each): input columns [col0, col0+K) of W in
// image columns [0, K), the bias (if any) in image column K; layout per `b3` as described in ag_common.h.
void pack_layer(std::vector<float> &dst, int b3, const float *W, int ld, int col0, int K, int n_out, const float *bias,
                int n_tiles)
{
    for (int ti = 0; ti < n_tiles; ++ti) {
        const size_t base = dst.size();
        dst.resize(base + AG_CHUNK_FLOATS, 0.0f);
        float *c = dst.data() + base;
        uint16_t *cb = reinterpret_cast<uint16_t *>(c);
        for (int i = 0; i < 32; ++i) {
            const int o = 32 * ti + i;
            if (o >= n_out) continue;
            for (int k = 0; k <= K; ++k) {
                if (k == K && !bias) break;
                const float v = k < K ? W[(size_t)o * ld + col0 + k] : bias[o];
                if (!b3) {
                    c[i * AG_WSTRIDE + 4 * ((k >> 2) ^ ((i >> 1) & 7)) + (k & 3)] = v;
                } else {
                    const FragSlot f = frag_slot(k, i);
                    uint16_t hi = bf16_rne(v), lo = bf16_rne(v - bf16_to_f32(hi));
                    if (b3 >= 2) f16_split(v, hi, lo);
                    if (b3 == 3) {      // PrecH6: fp16 hi fragments only, [k16-step][64][8]; the fp6 lo part is packed on the device (pack_lo6_kernel)
                        cb[(size_t)f.u * 512 + f.at] = hi;
                        continue;
                    }
                    cb[(size_t)(2 * f.u + 0) * 512 + f.at] = hi;
                    cb[(size_t)(2 * f.u + 1) * 512 + f.at] = lo;
                }
            }
        }
    }
}

// One wide layer of the fp16 edge stack (PrecH3, ag_mlp_dev.h) as n_tiles chunk images of 20 480 bytes + their block scales:
//   bytes [0, 10240):      hi = fp16(W) fragments, [10 k16-steps u][64 lanes (i, h)][8 fp16], slot e = column 16u + 8(e>>2) + 4h + (e&3)
//   bytes [10240, 20480):  the A operands of the block-scaled fp8 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4), [5 input tiles t][64 lanes (i, h)][32 B]:
//                          bytes 0..15 = e4m3(W_lo / s_lo), bytes 16..31 = e4m3(W_hi / s_hi) of columns 32t + 8q + 4h + p at byte 4q + p
//                          (W_lo = W - hi; the instruction pairs byte k of an A lane with byte k of the B lane of the same half, and the two
//                          16-byte groups are its two K blocks: the kernels put [top byte of x16 | e5m2(x - x16)] of the same columns there)
//   scales (appended to `scales`, 128 dwords per tile): [2 dwords][64 lanes]: lane (i, h) holds the E8M0 exponents of its row's five input tiles,
//                          h = 0: s_lo, h = 1: s_hi (a K block takes its A scale from the lanes of the half with the block's number):
//                          dword 0 = tiles 0..3 (one byte each, selected by op_sel), dword 1 byte 0 = tile 4.  s = 2^(floor(log2(block max)) - 7).
void pack_layer_h3(std::vector<float> &dst, std::vector<uint32_t> &scales, const float *W, int ld, int col0, int K, int n_out, const float *bias,
                   int n_tiles)
{
    for (int ti = 0; ti < n_tiles; ++ti) {
        const size_t base = dst.size();
        dst.resize(base + AG_CHUNK_FLOATS, 0.0f);
        uint16_t *hi16 = reinterpret_cast<uint16_t *>(dst.data() + base);
        uint8_t *mx = reinterpret_cast<uint8_t *>(dst.data() + base) + 10240;
        const size_t sbase = scales.size();
        scales.resize(sbase + 128, 0x7f7f7f7fu);
        for (int i = 0; i < 32; ++i) {
            const int o = 32 * ti + i;
            float w[AG_FP], lo[AG_FP], hif[AG_FP];
            for (int k = 0; k < AG_FP; ++k) {
                w[k] = 0.0f;
                if (o < n_out) w[k] = k < K ? W[(size_t)o * ld + col0 + k] : ((k == K && bias) ? bias[o] : 0.0f);
                uint16_t hb, lb;
                f16_split(w[k], hb, lb);
                const _Float16 hh = (_Float16)w[k];
                hif[k] = (float)hh;
                lo[k] = w[k] - hif[k];
                const FragSlot f = frag_slot(k, i);
                hi16[(size_t)f.u * 512 + f.at] = hb;
            }
            for (int t = 0; t < AG_NT; ++t) {
                float mlo = 0.0f, mhi = 0.0f;
                for (int k = 32 * t; k < 32 * t + 32; ++k) { mlo = fmaxf(mlo, fabsf(lo[k])); mhi = fmaxf(mhi, fabsf(hif[k])); }
                auto expo = [](float m) {      // E8M0 byte of 2^(floor(log2 m) - 7): the block maximum lands in [128, 256) <= 448
                    int e = 0;
                    (void)frexpf(m, &e);
                    const int b = (e - 1) - 7 + 127;
                    return b < 1 ? 1 : (b > 254 ? 254 : b);
                };
                const int elo = mlo > 0.0f ? expo(mlo) : 127, ehi = mhi > 0.0f ? expo(mhi) : 127;
                for (int h = 0; h < 2; ++h) {
                    const int lane = h * 32 + i;
                    uint32_t &word = scales[sbase + (t >> 2) * 64 + lane];
                    const uint32_t byte = (uint32_t)(h ? ehi : elo);
                    word = (word & ~(0xffu << (8 * (t & 3)))) | (byte << (8 * (t & 3)));
                    for (int q = 0; q < 4; ++q)
                        for (int pp = 0; pp < 4; ++pp) {
                            const int k = 32 * t + 8 * q + 4 * h + pp;
                            uint8_t *dstb = mx + ((size_t)t * 64 + lane) * 32 + 4 * q + pp;
                            dstb[0] = e4m3_rne(ldexpf(lo[k], 127 - elo));
                            dstb[16] = e4m3_rne(ldexpf(hif[k], 127 - ehi));
                        }
                }
            }
        }
    }
}

// |v| <= fp16's largest finite value, for every element of a rows x cols block of row stride ld
bool fits_f16(const float *p, int rows, int cols, int ld)
{
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c)
            if (!(fabsf(p[(size_t)r * ld + c]) <= 65504.0f)) return false;
    return true;
}

}  // namespace

AgPackedWeights ag_pack_weights(const ag_model_config &cfg, const float *const *t)
{
    const int F = cfg.nf, dn = cfg.attr_dim + cfg.phys_dim + cfg.action_dim;
    const int de = 2 * cfg.attr_dim + 1 + 3 * cfg.n_his;
    AgPackedWeights p;
    std::vector<float> &s = p.image;
    s.reserve((size_t)(2 * 81 + 16) * AG_CHUNK_FLOATS);
    size_t (&off)[2][4] = p.off;
    for (int b3 = 0; b3 < 2; ++b3) {
        off[b3][0] = s.size();                                             // node_encode stream
        pack_first_layer(s, b3, t[W_PE0], dn, F, t[B_PE0]);
        pack_layer(s, b3, t[W_PE1], F, 0, F, F, t[B_PE1], AG_NT);
        pack_layer(s, b3, t[W_PE2], F, 0, F, F, t[B_PE2], AG_NT);
        pack_layer(s, b3, t[W_PP], 2 * F, 0, F, F, t[B_PP], AG_NT);        // Pn  = W_pp[:, :F] enc + b_pp
        pack_layer(s, b3, t[W_RP], 3 * F, F, F, F, nullptr, AG_NT);        // Hr  = W_rp[:, F:2F] h
        pack_layer(s, b3, t[W_RP], 3 * F, 2 * F, F, F, nullptr, AG_NT);    // Hs  = W_rp[:, 2F:3F] h
        off[b3][1] = s.size();                                             // edge_encode stream
        pack_first_layer(s, b3, t[W_RE0], de, F, t[B_RE0]);
        pack_layer(s, b3, t[W_RE1], F, 0, F, F, t[B_RE1], AG_NT);
        pack_layer(s, b3, t[W_RE2], F, 0, F, F, t[B_RE2], AG_NT);
        pack_layer(s, b3, t[W_RP], 3 * F, 0, F, F, t[B_RP], AG_NT);        // Eterm = W_rp[:, :F] enc_e + b_rp
        off[b3][2] = s.size();                                             // node_update (not last)
        pack_layer(s, b3, t[W_PP], 2 * F, F, F, F, nullptr, AG_NT);        // W_pp[:, F:2F] agg
        pack_layer(s, b3, t[W_RP], 3 * F, F, F, F, nullptr, AG_NT);
        pack_layer(s, b3, t[W_RP], 3 * F, 2 * F, F, F, nullptr, AG_NT);
        off[b3][3] = s.size();                                             // node_update (last) + decoder
        pack_layer(s, b3, t[W_PP], 2 * F, F, F, F, nullptr, AG_NT);
        pack_layer(s, b3, t[W_D0], F, 0, F, F, t[B_D0], AG_NT);
        pack_layer(s, b3, t[W_D1], F, 0, F, F, t[B_D1], AG_NT);
        pack_layer(s, b3, t[W_D2], F, 0, F, 3, t[B_D2], 1);
    }
    p.off_h2 = s.size();                                                   // edge_encode stream of the fp16 edge stack (PrecH3)
    std::vector<uint32_t> sc;                                              // block scales of its 15 wide units, 128 dwords each
    pack_first_layer(s, 2, t[W_RE0], de, F, t[B_RE0], 2 * cfg.attr_dim + 1);         // + residual columns for the 12 state differences, inputs 5..16 (AG_EDGE_LO_FEAT0)
    pack_layer_h3(s, sc, t[W_RE1], F, 0, F, F, t[B_RE1], AG_NT);
    pack_layer_h3(s, sc, t[W_RE2], F, 0, F, F, t[B_RE2], AG_NT);
    pack_layer_h3(s, sc, t[W_RP], 3 * F, 0, F, F, t[B_RP], AG_NT);
    p.off_sc = s.size();
    s.resize(p.off_sc + sc.size());
    memcpy(s.data() + p.off_sc, sc.data(), sc.size() * sizeof(uint32_t));
    // the stack packed just above is usable only if every one of its weights and biases is representable in fp16 (else hi = inf)
    p.h2_ok = fits_f16(t[W_RE0], F, de, de) && fits_f16(t[B_RE0], 1, F, F) && fits_f16(t[W_RE1], F, F, F) && fits_f16(t[B_RE1], 1, F, F) &&
              fits_f16(t[W_RE2], F, F, F) && fits_f16(t[B_RE2], 1, F, F) && fits_f16(t[W_RP], F, F, 3 * F) && fits_f16(t[B_RP], 1, F, F);
    return p;
}
