// XTTS voice cloning (the GPT half of Xtts.get_conditioning_latents): the conditioning encoder
// (TTS/tts/layers/xtts/latent_encoder.py), the perceiver resampler (perceiver_encoder.py), the mel
// front end wav_to_mel_cloning (TTS/tts/models/xtts.py) and torchaudio's polyphase resampler.
// Executors: xtts_cond.cpp; kernels: kernels_xtts_cond.hip; host row permutation: pack.cpp.
// Semantics as restated in DESIGN.md section 4 "XTTS conditioning".
#pragma once

#include <memory>
#include <vector>

#include "arena.hpp"
#include "common.hpp"
#include "fft_attn.hpp"
#include "stft.hpp"
#include "tts_mi355x.h"

namespace tts {

constexpr int kCondMaxBatch = TTS_XTTS_COND_MAX_BATCH;
constexpr int kCondMaxLatents = TTS_XTTS_COND_MAX_LATENTS;
constexpr int kCondMaxKeys = TTS_XTTS_COND_MAX_KEYS;
constexpr int kResampleMaxFactor = TTS_RESAMPLE_MAX_FACTOR;

// ---- host (pack.cpp) ----
// The reference's normalization() rule: groups of GroupNorm(channels)
int cond_groupnorm_groups(int channels);
// Row r of the q | k | v layout the attention kernel reads (q rows [0, E), k rows [E, 2E), v rows [2E, 3E),
// head h at h dk .. h dk + dk - 1) -> row of the reference's qkv conv, whose 3E rows are head-major and
// interleaved (head h: q rows 3 h dk .. + dk, then its k rows, then its v rows)
int cond_qkv_source_row(int r, int E, int heads);
// w [3E][E] and b [3E] of the reference's qkv conv -> the permuted rows
void pack_cond_qkv(const float* w, const float* b, int E, int heads, float* w_out, float* b_out);
// A perceiver matrix of n entries for launch_cond_product: copied (fp32) or rounded to nearest even to
// bf16, two per float of out; cond_rows_numel: floats of out
int64_t cond_rows_numel(int64_t n, bool bf16);
void pack_cond_rows(const float* w, int64_t n, bool bf16, float* out);
// torchaudio's sinc_interp_hann table (width 6, rolloff 0.99), transposed: out[k * n + p] = kern[p][k]
// for o = orig / gcd, n = new / gcd, k < 2 w + o; fp64, rounded to fp32.  w = resample_width(o, n).
int resample_width(int o, int n);
void build_resample_table(int o, int n, float* out);

// ---- kernels (kernels_xtts_cond.hip); every reduction runs in one fixed order ----
// y = GroupNorm(G, C, eps)(x) with the affine, planes [B][C][T]; two-pass statistics per (b, group)
void launch_cond_groupnorm(const float* x, const float* gamma, const float* beta, int B, int C, int T, int G, float eps,
                           float* y, hipStream_t s);
// out[b][h dh + d][l] = sum_j softmax_j(q_l . k_j dh^-0.5) v_j[d] over the keys of kv_lat (L of them,
// first) and then kv_ctx (T of them); q [B][H dh][L], kv_* [B][2 H dh][L | T] (k rows, then v rows)
void launch_cond_cross_attn(const float* q, const float* kv_lat, const float* kv_ctx, int B, int H, int dh, int L, int T,
                            float* out, hipStream_t s);
// The perceiver's products over its L <= kCondMaxLatents latent columns, planes x [B][K][L] -> out [B][R][L]:
// out = W x + bias (bias may be nullptr) + res (nullptr: none); geglu: out [B][R / 2][L] =
// gelu_erf(gate) a with [a | gate] = W x + bias.  w: [R][K] row-major as torch stores it, fp32 or
// (bf16 = true) bf16 (pack_cond_rows); fp32 FMA on fp32 activations either way, k ascending.
void launch_cond_product(const void* w, bool bf16, const float* bias, const float* x, const float* res, int B, int R,
                         int K, int L, int geglu, float* out, hipStream_t s);
// y[b][i] = x[i], i < n: the learned latents as every batch item's first plane
void launch_cond_broadcast(const float* x, int B, int64_t n, float* y, hipStream_t s);
// y[b][:][l] = x[b][:][l] / max(||x[b][:][l]||_2, 1e-12) sqrt(E) gamma, planes [B][E][L]
void launch_cond_rmsnorm(const float* x, const float* gamma, int B, int E, int L, float* y, hipStream_t s);
// mel[b][m][t] = log(max(sum_k fb[k][m] P[b][k][t], 1e-5)) / norms[m]; range [M][2]: the bins [lo, hi) outside
// which column m of fb is zero
void launch_cond_logmel(const float* P, int B, int K, int M, int T, const float* fb, const int* range,
                        const float* norms, float* mel, hipStream_t s);
// y[b][f n + p] = sum_k table[k][p] xpad[b][f o + k], xpad = x with w zeros in front; i < Nout
void launch_resample(const float* x, int B, int64_t N, const float* table, int o, int n, int w, int64_t Nout, float* y,
                     hipStream_t s);

// ---- executors ----
void xtts_cond_validate(const TtsXttsCondCfg& c);
std::vector<int64_t> xtts_cond_weight_shapes(const TtsXttsCondCfg& c);
inline int cond_ff_inner(const TtsXttsCondCfg& c) { return (int)((int64_t)c.model_dim * c.ff_mult * 2 / 3); }

class XttsCond {
 public:
  XttsCond(const TtsXttsCondCfg& cfg, const float* const* host_weights, int device);
  int num_frames(int64_t N) const;
  // wav [B][N] at 22 050 Hz -> mel [B][spec_dim][T]
  void mel(const float* wav, int B, int64_t N, const float* mel_norms, float* out, hipStream_t s,
           Profiler* prof = nullptr);
  // mel [B][spec_dim][T] -> out [B][E][num_latents]
  void style_emb(const float* mel, int B, int T, float* out, hipStream_t s, Profiler* prof = nullptr);
  int device() const { return device_; }

 private:
  struct Block {
    float *gn_g = nullptr, *gn_b = nullptr;
    PackedConv qkv, proj;
  };
  struct Layer {
    PackedConv to_kv;  // over the context's T columns: the conv path
    // the products over the latent columns (launch_cond_product): fp32, or bf16 in the bf16 mode
    float *w_q = nullptr, *w_kv = nullptr, *w_out = nullptr, *w_ff0 = nullptr, *b_ff0 = nullptr, *w_ff2 = nullptr,
          *b_ff2 = nullptr;
  };
  void conv(const char* name, const PackedConv& cv, const float* in, float* out, const float* res, int B, int T,
            hipStream_t s, Profiler* prof) const;

  TtsXttsCondCfg cfg_;
  int device_;
  int mode_;  // the convs' and the self-attention's math mode: MATH_FP32_X6 or MATH_BF16
  bool bf16_;
  int E_, H_, G_, L_, inner_, I_;
  PackedConv init_;
  std::vector<Block> blocks_;
  std::vector<Layer> layers_;
  float *lat0_ = nullptr, *gamma_ = nullptr, *fb_ = nullptr;  // latents as a plane [E][L]
  float* fb_range_ = nullptr;  // [spec_dim][2] ints: the nonzero bins of every filterbank column
  std::unique_ptr<Stft> stft_;
  DeviceBuffer arena_, ws_;
};

// The perceiver's feed-forward alone, for kernel tests: out = x + W2 (gelu_erf(gate) a) + b2 with
// [a | gate] = W0 x + b0 over planes [B][E][L]; host weights W0 [2I][E], b0 [2I], W2 [E][I], b2 [E]
void op_cond_ff(const float* d_x, int B, int E, int I, int L, const float* w0, const float* b0, const float* w2,
                const float* b2, int math_mode, float* d_out, hipStream_t s);

class Resampler {
 public:
  Resampler(int orig_freq, int new_freq, int device);
  int64_t num_samples(int64_t N) const;
  void forward(const float* x, int B, int64_t N, float* y, hipStream_t s);
  int device() const { return device_; }

 private:
  int device_, o_, n_, w_;
  DeviceBuffer table_;
};

}  // namespace tts
