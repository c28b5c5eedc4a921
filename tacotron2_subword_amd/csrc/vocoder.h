// What vocoder.hip (inference) and vocoder_bwd.hip (training) share: the layer table, the plan and the forward launchers.
#pragma once
#include <vector>

#include "kernels.h"

namespace t2 {

constexpr int kVocMaxPad = 60;                   // (k*d - d)/2 at k = 11, d = 12
// One layer on packed weights.  u == 0: Conv1d, kernel k, dilation d, stride 1, padding (k*d - d)/2, x [B,Cin,L] ->
// y [B,Cout,L];  y = ((accumulate ? y : 0) + conv(lrelu(x, slope)) + bias + res) * scale, bias and res nullable.
// u > 0: ConvTranspose1d, kernel k = 2u, stride u, padding (k - u)/2, x [B,Cin,L] -> y [B,Cout,L*u]; no res / accumulate.
struct VocConv {
    int B, Cin, Cout; long L; int k, d, u;
    const float* x; const float* packed; const float* bias; const float* res; float* y;
    float slope; int accumulate; float scale;
    // nullable, device: item b's rows hold clamp(frames[b], 0, T) * factor inputs (L = T * factor).  What x, res and (accumulate) y
    // hold behind that is never read; y behind it is left as it was
    const int32_t* frames = nullptr; int T = 0, factor = 0;
};
// kind 0 Conv1d, 1 ConvTranspose1d, 2 conv_post; offsets in floats into the packed weights.  Order: conv_pre, ups[i],
// resblocks[n] (ResBlock1: convs1[m] then convs2[m]; ResBlock2: convs[m]), conv_post: the order of the state dict.
struct HifiganLayer { int kind, cin, cout, k, d, u; size_t w_off, b_off; };
struct HifiganPlan { long out_len; size_t buf_floats, workspace_bytes, packed_bytes; int n_layers; };

constexpr int kVocStride = 288;                   // slab row stride in floats: = 32 mod 64 banks, >= kVocTT + 2*kVocMaxPad
static_assert(kVocStride % 64 == 32 && kVocStride >= kVocTT + 2 * kVocMaxPad, "slab row stride");

constexpr int kVocPostK = 7;                      // conv_post's kernel size

int voc_shape_check(const char* who, int Cin, int Cout, int k, int d, int u);
int voc_conv(const VocConv& a, hipStream_t s);
// conv_post and the tanh: x [B][C][len] -> audio (and pre, nullable) [B][len]; frames, sample_lengths nullable
int voc_post(const float* x, const float* w, const float* bias, float* audio, float* pre, int B, int C, long len, const int32_t* frames, int T, int factor,
             int32_t* sample_lengths, hipStream_t s);
int hifigan_layers(const t2_hifigan_config& c, std::vector<HifiganLayer>* out, size_t* packed_floats);   // validates; no device
int hifigan_plan(const t2_hifigan_config& c, int B, int T, HifiganPlan* out);

}  // namespace t2
