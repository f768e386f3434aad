// MelGAN-family generators (MelGAN, full-band MelGAN, multi-band MelGAN with its PQMF synthesis):
// executor (melgan.cpp), kernels (kernels_melgan.hip) and the host packer of the residual block
// (pack.cpp).  Reference: TTS/vocoder/models/melgan_generator.py, layers/melgan.py, layers/pqmf.py.
#pragma once

#include <string>
#include <vector>

#include "common.hpp"
#include "hifigan.hpp"
#include "tts_mi355x.h"

namespace tts {

// ---- whole residual block (kernels_melgan.hip) ----
//   out = Ws x + bs + W2 lrelu(W1 (*)_d reflpad(lrelu(x)) + b1) + b2      (slope 0.2, kernel 3)
// Rows come in blocks of 32 channels (MB = ceil(C / 32); rows >= C are zero rows), depth in
// 16-channel groups (G = ceil(C / 16); channels >= C are zero columns).
//   A1: 3 G steps, step s = 3 g + k:  W1[row][16 g + j][k]
//   A2: 2 G steps, step s < G: W2[row][16 s + j];  step G + g: Ws[row][16 g + j]  ("[W2 | Ws]")
// Fragment order (16-bit units), one MFMA k-step = 16 channels:
//   out[mb][step][piece][lane][j] = piece(A)[32 mb + (lane & 31)][16 step + 8 (lane >> 5) + j]
// bias1 = b1, bias2 = b2 + bs, both zero-padded to 32 MB floats.
constexpr int kMelganBlockTile = 64;   // output columns of one workgroup
constexpr int kMelganMaxDil = 27;      // res_kernel^3: the fourth block of a stack
constexpr int kMelganMaxC = 256;       // channels of a residual stack (base_channels 512 >> 1)
constexpr int kMelganLdsLimit = 160 * 1024;
inline int melgan_groups(int C) { return (C + 15) / 16; }
inline int melgan_mblocks(int C) { return (C + 31) / 32; }
int melgan_pieces(int mode);
int64_t packed_melgan_a1_numel16(int mode, int C);
int64_t packed_melgan_a2_numel16(int mode, int C);
// the fp32 entries the packer splits: row < 32 MB, col < 48 G (A1) / 32 G (A2)
float melgan_a1_entry(const float* w1, int C, int row, int col);
float melgan_a2_entry(const float* w2, const float* ws, int C, int row, int col);
void pack_melgan_block(int mode, const float* w1, const float* b1, const float* w2, const float* b2,
                       const float* ws, const float* bs, int C, uint16_t* a1, uint16_t* a2, float* bias1,
                       float* bias2);

struct MelganBlockArgs {
  const float* x;  // [B][C][L]
  float* y;        // [B][C][L], must not alias x
  const void* a1;
  const void* a2;
  const float* bias1;  // [32 MB]
  const float* bias2;
  unsigned a1_bytes, a2_bytes;
  int C, L, dil;
};
size_t melgan_block_lds(int mode, int C, int dil);
void launch_melgan_block(int mode, const MelganBlockArgs& a, int B, hipStream_t s);

// out[b][c][t] = mel[b][c][clamp(refl(t - rp) - pad, 0, T - 1)], t < T + 2 pad + 2 rp, with refl the
// reflection over [0, T + 2 pad): the replicate padding of inference and the reflection padding
// of the first conv as one gather
void launch_melgan_gather(const float* mel, int B, int C, int T, int pad, int rp, float* out, hipStream_t s);

struct MelganTailArgs {
  const float* x;  // [B][Cin][L]
  const float* w;  // [Co][Cin][K]
  const float* b;  // [Co]
  const float* g;  // synthesis filters [Co][taps + 1], or nullptr: no PQMF
  float* y;        // [B][Co][L], or [B][1][Co L] with the PQMF
  int Cin, Co, K, L, taps;
};
constexpr int kMelganTailMaxCo = 4;
void launch_melgan_tail(const MelganTailArgs& a, int B, hipStream_t s);
// y[b][0][n] = N sum_k sum_j G[k][j] x[b][k][(n + j - taps/2) / N] over the j with an integer index in [0, L)
void launch_pqmf_synthesis(const float* x, int B, int N, int L, const float* g, int taps, float* y, hipStream_t s);

// ---- executor ----
void melgan_validate(const TtsMelganCfg& c);
std::vector<int64_t> melgan_weight_shapes(const TtsMelganCfg& c);
// the host-side length checks of a forward: every reflection pad must be smaller than its plane
void melgan_check_length(const TtsMelganCfg& c, int64_t T, int pad);

class Melgan {
 public:
  Melgan(const TtsMelganCfg& cfg, const float* const* host_weights, int device);
  int64_t out_len(int T, int pad, int synth) const;
  int64_t workspace_bytes(int B, int T, int pad) const;
  void forward(const float* mel, int B, int C, int T, int pad, int synth, float* out, hipStream_t s,
               Profiler* prof = nullptr);
  int device() const { return device_; }

 private:
  struct Conv : PackedConv {
    int U = 0;  // upsamplers: the factor (the K = 2 polyphase conv form, Conv1dArgs::ups)
    std::string name;
  };
  struct Block {
    int C = 0, dil = 1;
    int64_t a1_numel16 = 0, a2_numel16 = 0;
    float* a1 = nullptr;  // 16-bit fragments (a1_numel16, a2_numel16 units)
    float* a2 = nullptr;
    float* bias1 = nullptr;
    float* bias2 = nullptr;
    std::string name;
  };
  int64_t plane_floats(int B, int T, int pad) const;

  TtsMelganCfg cfg_;
  int device_;
  int mode_;  // the math mode the kernels run: MATH_FP32_X6 or MATH_BF16
  int hop_ = 1;
  Conv pre_;
  std::vector<Conv> ups_;
  std::vector<Block> blocks_;  // num_ups * num_res_blocks, in execution order
  float* tail_w_ = nullptr;
  float* tail_b_ = nullptr;
  float* g_ = nullptr;
  DeviceBuffer arena_, ws_;
};

}  // namespace tts
