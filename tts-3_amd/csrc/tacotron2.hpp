// Tacotron2 inference: executor (tacotron2.cpp), its kernels (kernels_tacotron2.hip) and the host
// packer of the skinny recurrent products (pack.cpp).  Reference (Coqui TTS 0.22.0):
// TTS/tts/models/tacotron2.py (inference), TTS/tts/layers/tacotron/{tacotron2,attentions,common_layers}.py.
#pragma once

#include <vector>

#include "common.hpp"
#include "hifigan.hpp"
#include "tts_mi355x.h"

namespace tts {

// ---- skinny product [R x K] . [K x B], B <= 32: 16 rows per workgroup, weights streamed once ----
// Packed weights: out[rb][k][j] = W[row(16 rb + j)][k], k < Kp = K rounded up to kSkinnyKAlign (zeros
// beyond K), fp32 or bf16 (round to nearest even).  LSTM: R = 4H and row(16 ub + 4 u + g) = g H + 4 ub + u,
// so a workgroup owns the (i, f, g, o) rows of kLstmUnitBlock hidden units; W = [w_ih | w_hh].
constexpr int kLstmUnitBlock = TTS_LSTM_UNIT_BLOCK;
constexpr int kSkinnyRows = 16;
constexpr int kSkinnyKAlign = 64;
constexpr int kSkinnyMaxBatch = TTS_TACOTRON2_MAX_BATCH;
inline int skinny_kp(int K) { return ceil_div(K, kSkinnyKAlign) * kSkinnyKAlign; }
// floats of the packed image (bf16: two elements per float)
int64_t packed_skinny_numel(int R, int K, bool bf16);
int64_t packed_lstm_numel(int H, int K, bool bf16);
// w_ih [4H][I] (NULL with I = 0), w_hh [4H][H]
void pack_lstm(const float* w_ih, const float* w_hh, int H, int I, bool bf16, float* out);
// out[4 unit + g] = b_ih[g H + unit] + b_hh[g H + unit] (either may be NULL)
void pack_lstm_bias(const float* b_ih, const float* b_hh, int H, float* out);
// w [R][K] in row order, rows padded with zeros to whole blocks of 16
void pack_skinny_rows(const float* w, int R, int K, bool bf16, float* out);

// State vectors are batch-minor: v[k * BT + b] with BT = skinny_batch_tile(B), so a workgroup stages
// [x0 | x1 | x2] with contiguous loads.
int skinny_batch_tile(int B);  // 1, 2, 4, 8, 16 or 32
struct SkinnyArgs {
  const void* w[2];        // per direction (grid.z)
  const float* bias[2];    // LSTM: [4H] in (unit, gate) order; linear: [R]; or nullptr
  const float* x[2][3];    // up to three input segments [n][BT]; LSTM: the last one is h
  int n[3];
  int K, Kp, B, BT, bf16, ndir;
  int lstm;                // 1: LSTM cell epilogue, 0: out = W x + bias
  // LSTM
  int H;
  float* c[2];             // [H][BT], updated in place (a unit's cell is touched by one thread only)
  float* h_out[2];         // [H][BT]: never the buffer x reads
  const float* pre;        // precomputed input term [B][ndir 4H][T] (rows in torch order), or nullptr
  float* y;                // [B][T][ldy]: h' at column dir H + unit of row t, or nullptr
  int T, ldy, step;
  const int64_t* len;      // with pre / y: utterance b is active while step < len[b] (nullptr: T); the
                           // second direction reads and writes t = len[b] - 1 - step
  const int* done;         // utterances with done[b] != 0 are left untouched, or nullptr
  // linear
  int R;
  float* out;              // out[b * ldo + row]
  int64_t ldo;
};
void launch_skinny(const SkinnyArgs& a, hipStream_t s);

constexpr int kT2MaxA = 128, kT2MaxF = 32, kT2MaxLocK = 31, kT2MaxQ = 2048, kT2MaxP = 1024, kT2MaxOut = 1024;
constexpr int kT2AttnTile = 128;  // encoder positions one pass of the attention kernel covers
struct T2AttnArgs {
  const float* query;  // [Q][BT]
  const float* wq;     // [A][Q]
  const float *aw_in, *awc_in;  // [B][T]
  float *aw_out, *awc_out;      // [B][T]: never the buffers read (the location conv reads a halo)
  const float* loc_w;  // [F][2][Kl]
  const float* loc_d;  // [A][F]
  const float* pinp;   // [B][A][T]
  const float* v;      // [A]
  const float* v_bias; // [1]
  const float* inputs; // [B][T][D]
  const int64_t* len;  // [B] or nullptr
  const int* done;
  float* ctx;          // [D][BT]
  float* align;        // [B][S][T]
  int B, BT, T, D, A, F, Kl, Q, S, step, softmax;
};
void launch_t2_attention(const T2AttnArgs& a, hipStream_t s);

struct T2StopArgs {
  const float* dec_out;  // [B][S][Cr]: this step's row was written by the projection
  const float* hd;       // [Q][BT]
  const float* stop_w;   // [Q + Cr]
  const float* stop_b;   // [1]
  const float* w0t;      // [C][P] prenet layer 0, transposed
  const float* w1t;      // [P][P] prenet layer 1, transposed
  float* prenet;         // [P][BT]: the next step's prenet output
  float* stop_tokens;    // [B][S]
  int* done;             // [B]
  int* steps;            // [B]
  int* counters;         // [0] utterances ended, [1] all ended
  int B, BT, Q, C, r, P, S, step, max_steps;
  float threshold;
};
void launch_t2_stop_prenet(const T2StopArgs& a, hipStream_t s);

// glue (kernels_tacotron2.hip)
void launch_t2_embed(const int64_t* tok, const float* emb, float* x, int B, int E, int T, int num_chars, hipStream_t s);
// inputs[b][t][E + j] = table[ids[b]][j] (ids) or vec[b][j]
void launch_t2_speaker(const int64_t* ids, const float* table, int num_speakers, const float* vec, float* inputs, int B,
                       int T, int E, int W, hipStream_t s);
// pinp[b][a][t] = sum_d wt[d][a] inputs[b][t][d]
void launch_t2_processed_inputs(const float* inputs, const float* wt, float* pinp, int B, int T, int D, int A,
                                hipStream_t s);
// x[b][c][t] = dec[b][t][c] (t < L; dec rows of ld floats), mask[b][t] = t < steps[b] * r
void launch_t2_to_planes(const float* dec, const int* steps, int r, float* x, float* mask, int B, int C, int L,
                         int64_t dec_bstride, hipStream_t s);
void launch_t2_tanh(float* x, int64_t n, hipStream_t s);
// out[b][t][c] = (dec[b][t][c] + post[b][c][t]) * mask[b][t]
void launch_t2_residual_out(const float* dec, const float* post, const float* mask, float* out, int B, int C, int L,
                            int64_t dec_bstride, hipStream_t s);
// dst[c * ldd + r] = src[r * lds + c], r < rows, c < cols
void launch_t2_transpose(const float* src, float* dst, int rows, int cols, int lds, int ldd, hipStream_t s);

// tts_op_lstm_cell: one cell step on torch-layout operands (packs, uploads, runs, synchronises)
void op_lstm_cell(const float* d_x, const float* d_h, const float* d_c, int B, int I, int H, const float* w_ih,
                  const float* w_hh, const float* b_ih, const float* b_hh, int math_mode, float* d_h_out,
                  float* d_c_out, hipStream_t s);

void tacotron2_validate(const TtsTacotron2Cfg& c);
std::vector<int64_t> tacotron2_weight_shapes(const TtsTacotron2Cfg& c);

class Tacotron2 {
 public:
  Tacotron2(const TtsTacotron2Cfg& cfg, const float* const* host_weights, int device);
  void encode(const int64_t* tok, const int64_t* x_len, const int64_t* spk, const float* dvec, int B, int T,
              float* inputs, float* pinp, hipStream_t s, Profiler* prof = nullptr);
  // returns the largest step count (host value: the stream is synchronised once per chunk)
  int decode(const float* inputs, const float* pinp, const int64_t* x_len, int B, int T, int max_steps,
             float stop_threshold, float* dec_out, float* align, float* stop_tokens, int* steps, hipStream_t s,
             Profiler* prof = nullptr);
  void postnet(const float* dec_out, const int* steps, int B, int S, int row_stride, float* model_out, hipStream_t s,
               Profiler* prof = nullptr);
  int device() const { return device_; }

 private:
  struct Lstm {
    float* w = nullptr;  // packed [w_ih | w_hh]
    float* b = nullptr;  // packed bias
    int H = 0, I = 0;
    bool bf16 = false;
  };
  void conv(const PackedConv& cv, const float* x, float* y, const float* mask, float out_slope, int B, int T,
            hipStream_t s, Profiler* prof, const char* name);

  TtsTacotron2Cfg cfg_;
  int device_;
  int conv_mode_;  // MATH_FP32_X6 or MATH_BF16
  int E_, He_, Q_, P_, A_, F_, Kl_, C_, Cr_, D_;
  float* emb_ = nullptr;
  PackedConv enc_conv_[3], enc_pre_, post_conv_[5];
  Lstm enc_lstm_[2], att_rnn_, dec_rnn_;
  float *prenet0t_ = nullptr, *prenet1t_ = nullptr;
  float *wq_ = nullptr, *win_t_ = nullptr, *v_ = nullptr, *vb_ = nullptr, *loc_w_ = nullptr, *loc_d_ = nullptr;
  float *proj_w_ = nullptr, *proj_b_ = nullptr, *stop_w_ = nullptr, *stop_b_ = nullptr;
  float* spk_ = nullptr;
  DeviceBuffer arena_, ws_;
};

}  // namespace tts
