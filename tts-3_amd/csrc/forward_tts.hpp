// ForwardTTS (FastPitch / FastSpeech) inference: executor (forward_tts.cpp) and its glue kernels
// (kernels_forward_tts.hip).  Reference (Coqui TTS 0.22.0): TTS/tts/models/forward_tts.py (inference),
// TTS/tts/layers/generic/transformer.py (FFTransformer, FFTransformerBlock),
// TTS/tts/layers/feed_forward/{encoder,decoder}.py, TTS/tts/layers/generic/pos_encoding.py,
// TTS/tts/layers/glow_tts/duration_predictor.py.
#pragma once

#include <memory>
#include <vector>

#include "common.hpp"
#include "hifigan.hpp"
#include "text.hpp"
#include "tts_mi355x.h"

namespace tts {

constexpr int kFftKernel = 3;  // FFTransformer kernel_size_fft (FFTransformerBlock does not pass another)

void launch_ftts_embed(const int64_t* tok, const int64_t* len, const float* emb, float* x, float* mask, int B, int H,
                       int T, int num_chars, hipStream_t s);
void launch_ftts_mask_add(const float* x, const float* mask, const float* table, const int64_t* spk, float* y, int B,
                          int C, int T, int num_speakers, hipStream_t s);
void launch_ftts_durations(const float* dlog, const float* xm, const float* given, float* dur, int64_t* y_len, int B,
                           int T, float length_scale, hipStream_t s);
void launch_ftts_pitch_emb(const float* pitch, const float* w, const float* bias, float* x, int B, int C, int T, int k,
                           hipStream_t s);
void launch_ftts_posenc(float* x, const float* pe, const float* mask, int B, int C, int T, int pe_len, float scale,
                        hipStream_t s);

void forward_tts_validate(const TtsForwardTtsCfg& c);
std::vector<int64_t> forward_tts_weight_shapes(const TtsForwardTtsCfg& c);

class ForwardTts {
 public:
  ForwardTts(const TtsForwardTtsCfg& cfg, const float* const* host_weights, int device);

  // Everything before the host read of y_len (text side, always fp32x6):
  //   o_en [B][H][T] = encoder(emb(tok)) * x_mask + emb_g[spk] (+ pitch_emb(pitch) with use_pitch)
  //   dur_log, pitch [B][T]; dur [B][T] (rounded, or `given`); y_len [B] = sum of dur
  void encode(const int64_t* tok, const int64_t* x_len, const int64_t* spk, const float* given, int B, int T,
              float length_scale, float* o_en, float* x_mask, float* dur_log, float* pitch, float* dur,
              int64_t* y_len, hipStream_t s, Profiler* prof = nullptr);
  // out [B][out_channels][T_de], attn [B][T][T_de], y_mask [B][T_de]; T_de >= max(y_len)
  void decode(const float* o_en, const float* dur, const float* x_mask, const int64_t* y_len, int B, int T, int T_de,
              bool mask_keys, float* out, float* attn, float* y_mask, hipStream_t s, Profiler* prof = nullptr);
  // y = FFTransformerBlock(x) of the encoder (decoder = false, fp32x6) or the decoder (its math
  // mode): x, y [B][H][T]; key_len [B] or NULL
  void block(bool decoder, const float* x, const int64_t* key_len, int B, int T, float* y, hipStream_t s,
             Profiler* prof = nullptr);
  int device() const { return device_; }

 private:
  using Conv = PackedConv;
  struct Layer {
    Conv qkv, o, ffn1, ffn2;  // o holds 2 out_proj: norm1 is LN(x + 2 a)
    float *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr;
  };
  void reserve(int B, int T);
  // runs the layers on the state in X0 (workspace); returns the buffer holding the result
  float* run_layers(const std::vector<Layer>& layers, int mode, int heads, const int64_t* key_len, int B, int T,
                    hipStream_t s, Profiler* prof, const char* tag);

  TtsForwardTtsCfg cfg_;
  int device_;
  int dec_mode_;  // MATH_FP32_X6 or MATH_BF16
  float* emb_ = nullptr;
  std::vector<Layer> enc_, dec_;
  float* pe_ = nullptr;
  Conv postnet_;
  std::unique_ptr<VitsDp> dp_, pp_;
  float *pitch_w_ = nullptr, *pitch_b_ = nullptr;
  float* emb_g_ = nullptr;
  DeviceBuffer arena_, ws_;
};

}  // namespace tts
