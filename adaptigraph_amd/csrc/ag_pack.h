// ag_pack.h — the host image of a model's weight streams (ag_pack.hip): pure host code, no HIP runtime call.
#pragma once
#include "../../include/adaptigraph_hip.h"

#include <vector>

namespace ag_pack {

// state_dict order (model.py:103-122)
enum { W_PE0, B_PE0, W_PE1, B_PE1, W_PE2, B_PE2, W_RE0, B_RE0, W_RE1, B_RE1, W_RE2, B_RE2, W_PP, B_PP, W_RP, B_RP,
       W_D0, B_D0, W_D1, B_D1, W_D2, B_D2, N_TENSORS };

uint16_t bf16_rne(float x);
void f16_split(float v, uint16_t &hi, uint16_t &lo);
uint8_t e4m3_rne(float v);
float bf16_to_f32(uint16_t b);

}  // namespace ag_pack

struct AgPackedWeights {
    std::vector<float> image;      // every stream, one behind the other; the offsets below in floats
    size_t off[2][4];              // [fp32 | split-bf16][node_encode, edge_encode, node_mid, node_last]
    size_t off_h2, off_sc;         // the edge_encode stream of the fp16 edge stack, and its block scales (dwords)
    bool h2_ok;                    // every edge-stack weight and bias is representable in fp16
};
AgPackedWeights ag_pack_weights(const ag_model_config &cfg, const float *const *t);
