// Flash-style multi-head self-attention on the matrix cores (kernels_fft_attn.hip): the attention of
// nn.MultiheadAttention as the FFTransformer layers of ForwardTTS (FastPitch) run it, for long
// sequences (mel frames) and wide heads (one head of 384 channels).
// Reference: TTS/tts/layers/generic/transformer.py (FFTransformer.self_attn).
#pragma once

#include "common.hpp"

namespace tts {

// queries of one workgroup
constexpr int kMhaTile = 64;
// Accepted head sizes dk = E / heads: 32, 64, 128, 192, 256, 384, with E <= 512.
constexpr int kMhaMaxE = 512;
bool mha_head_size_ok(int dk);

// out[b][h dk + d][i] = sum_j softmax_j((q_i dk^-0.5) . k_j)[j] v_j[d] over the keys j < key_len[b]
// (key_len == nullptr: every j < T), for every query i < T, padded ones included.
//   qkv: [B][3E][T] fp32, rows q | k | v, head h at channels h dk .. h dk + dk - 1 (the layout
//        launch_attention takes); the dk^-0.5 query scale is applied here, not by the caller
//   key_len: [B] int64 on the device, values in [1, T] (larger values count as T, negative ones as 0;
//        with 0 keys the item's output is all zeros: an invalid item gives zeros, where the
//        reference's softmax over an all -inf row is NaN)
//   out: [B][E][T] fp32, must not alias qkv
// mode: MATH_FP32_X6 or MATH_BF16.  Results do not depend on B.
void launch_mha(int mode, const float* qkv, const int64_t* key_len, float* out, int B, int E, int heads, int T,
                hipStream_t s);
// The causal variant (the XTTS GPT's attention over a whole sequence): query i attends to the keys
// j <= i with j < key_len[b].  Key tiles wholly above a workgroup's diagonal are skipped, the diagonal
// tiles are masked; the outputs at positions <= i do not depend on anything at a position > i.
// Head sizes 32, 64, 128 with E <= kMhaCausalMaxE; otherwise as launch_mha.
constexpr int kMhaCausalMaxE = 2048;
void launch_mha_causal(int mode, const float* qkv, const int64_t* key_len, float* out, int B, int E, int heads, int T,
                       hipStream_t s);

// launch_mha's kernel at the causal variant's limits (head sizes 32, 64, 128 with E <= kMhaCausalMaxE), no
// mask but key_len: the XTTS conditioning encoder's self-attention.  Bitwise launch_mha where both accept.
void launch_mha_wide(int mode, const float* qkv, const int64_t* key_len, float* out, int B, int E, int heads, int T,
                     hipStream_t s);

}  // namespace tts
