// Conv2d on the matrix cores (kernels_conv2d.hip) and its host packer (pack.cpp): the 3x3 (pad 1)
// and 1x1 (pad 0) convs, stride 1 or 2, of the SE-ResNet speaker encoder
// (TTS/encoder/models/resnet.py: conv1, SEBasicBlock.conv1 / conv2, downsample.0).
#pragma once

#include "common.hpp"
#include "tts_mi355x.h"

namespace tts {

//   y[b][co][fo][to] = scale[co] act(bias[co] + sum_{ci,kf,kt} w[co][ci][kf][kt] x[b][ci][s fo + kf - P][s to + kt - P]) + shift[co]
// with P = (KS - 1) / 2, zeros outside the plane, act = relu or the identity, Fo = ceil(F / s),
// To = ceil(T / s).  Planes are [B][C][F][T] fp32, T contiguous.
// A GEMM per output row fo: rows = output channels in blocks of 32 (MB = ceil(Cout / 32); rows
// >= Cout are zero rows), columns = to, depth = KS KS 16 G (G = ceil(Cin / 16) channel groups;
// channels >= Cin are zero columns), ordered step s = (g KS + kf) KS + kt.
// Fragment order of the packed weights (16-bit units), one MFMA k-step = 16 channels of one tap:
//   out[mb][step][piece][lane][j] = piece(w)[32 mb + (lane & 31)][16 g + 8 (lane >> 5) + j][kf][kt]
// bias / scale / shift are padded to 32 MB floats (0 / 1 / 0).
constexpr int kConv2dTile = 64;    // output columns of one workgroup
constexpr int kConv2dMaxCout = 4096;  // in groups of 256 (8 row blocks) per workgroup
constexpr int kConv2dLdsLimit = 160 * 1024;
inline int conv2d_groups(int Cin) { return (Cin + 15) / 16; }
inline int conv2d_mblocks(int Cout) { return (Cout + 31) / 32; }
inline int conv2d_rowgroups(int Cout) { return (conv2d_mblocks(Cout) + 7) / 8; }
inline int conv2d_out(int n, int stride) { return (n + stride - 1) / stride; }
int conv2d_pieces(int mode);
// the math mode the kernels run for a requested one: MATH_BF16, or MATH_FP32_X6 for every fp32 name
inline int conv2d_mode(int mode) { return mode == MATH_BF16 ? MATH_BF16 : MATH_FP32_X6; }
int64_t packed_conv2d_numel16(int mode, int Cout, int Cin, int KS);
// w [Cout][Cin][KS][KS] -> fragments (packed_conv2d_numel16 units); bias / scale / shift (each may
// be nullptr) -> [32 MB] floats
void pack_conv2d(int mode, const float* w, int Cout, int Cin, int KS, uint16_t* out);
void pack_conv2d_epilogue(const float* bias, const float* scale, const float* shift, int Cout, float* bias_p,
                          float* scale_p, float* shift_p);

struct Conv2dArgs {
  const float* x;  // [B][Cin][F][T]
  float* y;        // [B][Cout][Fo][To], must not alias x
  const void* a;   // packed weights
  const float* bias;   // [32 MB] each
  const float* scale;
  const float* shift;
  // SE pooling partial sums [B][Cout][Fo][conv2d_pool_slots(To)] (every slot is written), or nullptr
  float* pool;
  unsigned a_bytes;
  int Cin, Cout, F, T, KS, stride, relu;
};
inline int conv2d_pool_slots(int To) { return 2 * ((To + kConv2dTile - 1) / kConv2dTile); }
size_t conv2d_lds(int mode, int KS, int stride);
// every limit is checked here, before the launch (TTS_ERR_UNSUPPORTED / TTS_ERR_INVALID)
void conv2d_check(const Conv2dArgs& a, int B);
void launch_conv2d(int mode, const Conv2dArgs& a, int B, hipStream_t s);

}  // namespace tts
