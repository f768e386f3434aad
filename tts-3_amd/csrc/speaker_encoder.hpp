// ResNetSpeakerEncoder (TTS/encoder/models/resnet.py, base_encoder.py) on the device: executor
// (speaker_encoder.cpp) and its small kernels (kernels_speaker_encoder.hip).  The trunk's convs and
// the two attention convs run on the Conv2d kernel (conv2d.hpp), the STFT on the spectrogram GEMM
// (stft.hpp) with frame centring and a power output.
#pragma once

#include <memory>
#include <string>
#include <vector>

#include "common.hpp"
#include "conv2d.hpp"
#include "hifigan.hpp"
#include "stft.hpp"
#include "tts_mi355x.h"

namespace tts {

// ---- kernels (kernels_speaker_encoder.hip); every reduction runs in one fixed order ----
// y[b][n] = f[0] x[b][n - 1] + f[1] x[b][n], x[b][-1] := x[b][1] (PreEmphasis: reflect pad 1 on the left)
void launch_spk_preemph(const float* x, int B, int64_t N, const float* filt, float* y, hipStream_t s);
// mel[b][m][t] = sum_k fb[k][m] P[b][k][t]  (fp32 FMA, k ascending)
void launch_spk_mel(const float* P, int B, int K, int M, int T, const float* fb, float* mel, hipStream_t s);
// y[b][m][:] = instance_norm(log_in ? log(x + 1e-6) : x) over t (biased variance, eps 1e-5)
void launch_spk_instnorm(const float* x, int B, int M, int T, int log_in, float* y, hipStream_t s);
// gate[b][c] = sigmoid(w2 relu(w0 mean[b] + b0) + b2), mean[b][c] = (sum of the n partial sums of (b, c)) / count
void launch_spk_se_gate(const float* pool, int B, int C, int n, float count, const float* w0, const float* b0,
                        const float* w2, const float* b2, float* gate, hipStream_t s);
// out = relu(h gate[b][c] + res), planes of P elements
void launch_spk_se_apply(const float* h, const float* res, const float* gate, int B, int C, int64_t P, float* out,
                         hipStream_t s);
// w = softmax_t(att[b][d][:]); pooled[b][d] = sum_t x w; asp: pooled[b][D + d] = sqrt(max(sum_t w (x - mu)^2, 1e-5))
void launch_spk_pool(const float* x, const float* att, int B, int D, int T, int asp, float* pooled, hipStream_t s);
// out[b][j] = bias[j] + sum_k w[j][k] p[b][k]
void launch_spk_fc(const float* p, int B, int K, int J, const float* w, const float* bias, float* out, hipStream_t s);
// out[b][:] /= max(||out[b][:]||_2, 1e-12)
void launch_spk_l2norm(float* out, int B, int J, hipStream_t s);

// ---- executor ----
void speaker_encoder_validate(const TtsSpeakerEncoderCfg& c);
std::vector<int64_t> speaker_encoder_weight_shapes(const TtsSpeakerEncoderCfg& c);

class SpeakerEncoder {
 public:
  SpeakerEncoder(const TtsSpeakerEncoderCfg& cfg, const float* const* host_weights, int device);
  // frames of an n-sample wav (torch_spec) or n itself (features); throws outside the limits
  int num_frames(int64_t n) const;
  void features(const float* x, int B, int64_t n, float* feat, hipStream_t s, Profiler* prof = nullptr);
  void forward(const float* x, int B, int64_t n, int l2_norm, float* out, hipStream_t s, Profiler* prof = nullptr);
  int device() const { return device_; }

 private:
  struct Conv {
    int Cin = 0, Cout = 0, KS = 3, stride = 1, relu = 0;
    int64_t numel16 = 0;
    float* a = nullptr;  // packed fragments
    float* bias = nullptr;
    float* scale = nullptr;
    float* shift = nullptr;
    std::string name;
  };
  struct Block {
    Conv c1, c2, down;
    bool has_down = false;
    int C = 0;
    float *w0 = nullptr, *b0 = nullptr, *w2 = nullptr, *b2 = nullptr;
  };
  void check_shape(int B, int T) const;
  void run_conv(const Conv& c, const float* x, int B, int F, int T, float* y, float* pool, hipStream_t s,
                Profiler* prof) const;

  TtsSpeakerEncoderCfg cfg_;
  int device_;
  int mode_;  // the math mode of the convs: MATH_FP32_X6 or MATH_BF16
  int D_ = 0;  // channels of the pooled sequence: num_filters[3] * input_dim / 8
  std::unique_ptr<Stft> stft_;
  float* filt_ = nullptr;
  float* fb_ = nullptr;
  Conv stem_, att1_, att2_;
  std::vector<Block> blocks_;
  float* fc_w_ = nullptr;
  float* fc_b_ = nullptr;
  DeviceBuffer arena_, ws_;
};

}  // namespace tts
