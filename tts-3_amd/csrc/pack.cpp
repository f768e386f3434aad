// Host-side packing of PyTorch conv weights into the chunked layouts the MFMA kernels
// stage into LDS with contiguous 16-byte loads.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "conv2d.hpp"
#include "melgan.hpp"
#include "stft.hpp"
#include "tacotron2.hpp"
#include "wino_consts.hpp"
#include "xtts_cond.hpp"
#include "xtts_gpt.hpp"

namespace tts {

// MFMA-fragment layout of the conv1d A operand (see conv1d_mfma_kernel):
//   out[mb][c8][k][lane][j] = w[mb*32 + (lane&31)][c8*8 + 4*(lane>>5) + j][k]
// mb over ceil(Cout/BM)*BM/32 blocks, c8 over n_chunks*CK/8 groups (zero padded), plus one
// trailing fragments of slack for the kernel's prefetch (up to 2 steps ahead).
int64_t packed_conv1d_numel(int Cout, int Cin, int K, const ConvTile& t) {
  const int64_t mblocks = (int64_t)ceil_div(Cout, t.BM) * (t.BM / 32);
  const int64_t groups = (int64_t)ceil_div(Cin, t.CK) * (t.CK / 8);
  return mblocks * groups * K * 256 + 512;
}

void pack_conv1d(const float* w, int Cout, int Cin, int K, const ConvTile& t, float* out) {
  const int mblocks = ceil_div(Cout, t.BM) * (t.BM / 32);
  const int groups = ceil_div(Cin, t.CK) * (t.CK / 8);
  int64_t o = 0;
  for (int mb = 0; mb < mblocks; ++mb)
    for (int c8 = 0; c8 < groups; ++c8)
      for (int k = 0; k < K; ++k)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 4; ++j) {
            const int co = mb * 32 + (lane & 31);
            const int ci = c8 * 8 + 4 * (lane >> 5) + j;
            out[o++] = (co < Cout && ci < Cin) ? w[((int64_t)co * Cin + ci) * K + k] : 0.f;
          }
  for (int i = 0; i < 512; ++i) out[o++] = 0.f;
}

// bf16x6 split of an fp32 value: x = p0 + p1 + p2 exactly, round-to-nearest-even per piece
// (same rounding as the device's v_cvt_pk_bf16_f32).
static inline uint16_t f2bf_rne(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static inline float bf2f(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
void split3_host(float x, uint16_t& p0, uint16_t& p1, uint16_t& p2) {
  p0 = f2bf_rne(x);
  const float r1 = x - bf2f(p0);
  p1 = f2bf_rne(r1);
  const float r2 = r1 - bf2f(p1);
  p2 = f2bf_rne(r2);
}

// fp16 hi/lo split of a value already scaled into [0, 2^14] magnitude: x ~ hi + lo
// (round-to-nearest-even, as the device's v_cvt_f16_f32; see kernels_conv_split.hip).
static inline void split_h3_host(float x, uint16_t& hi, uint16_t& lo) {
  const _Float16 h = (_Float16)x;
  hi = __builtin_bit_cast(uint16_t, h);
  lo = __builtin_bit_cast(uint16_t, (_Float16)(x - (float)h));
}

static int split_pieces(int mode) { return mode == MATH_FP32_F16X3 ? 2 : (mode == MATH_BF16 ? 1 : 3); }

// Split-mode A-operand fragments (conv1d_split_kernel), in floats (2 x 16-bit per float):
//   out[mb][c16][k][piece][lane][j] = piece_p(w'[mb*32 + (lane&31)][c16*16 + 8*(lane>>5) + j][k])
// plus 4 steps of slack for the prefetch (up to 4 steps ahead).  w' = w for bf16x6, w * 2^-e for fp16 hi/lo with e
// chosen so max|w'| lies in [2^13, 2^14) (exact; undone in the kernel epilogue).
int64_t packed_conv1d_split_numel(int mode, int Cout, int Cin, int K, const ConvTile& t) {
  const int64_t mblocks = (int64_t)ceil_div(Cout, t.BM) * (t.BM / 32);
  const int64_t groups = (int64_t)ceil_div(Cin, t.CK) * (t.CK / 16);
  return (mblocks * groups * K + 4) * split_pieces(mode) * 64 * 4;
}

int pack_conv1d_split(int mode, const float* w, int Cout, int Cin, int K, const ConvTile& t, float* out_f,
                      bool quad_perm) {
  const int NP = split_pieces(mode);
  int e = 0;
  if (mode == MATH_FP32_F16X3) {
    float m = 0.f;
    bool finite = true;  // std::max(m, NaN) keeps m: test every element, not the running max
    for (int64_t i = 0; i < (int64_t)Cout * Cin * K; ++i) {
      finite = finite && std::isfinite(w[i]);
      m = std::max(m, std::fabs(w[i]));
    }
    TTS_REQUIRE(finite, 1, "conv weights contain inf/NaN");
    if (m > 0.f) {
      int E;
      (void)std::frexp(m, &E);
      e = E - 14;
    }
  }
  uint16_t* out = reinterpret_cast<uint16_t*>(out_f);
  const int mblocks = ceil_div(Cout, t.BM) * (t.BM / 32);
  const int groups = ceil_div(Cin, t.CK) * (t.CK / 16);
  int64_t o = 0;
  for (int mb = 0; mb < mblocks; ++mb)
    for (int c16 = 0; c16 < groups; ++c16)
      for (int k = 0; k < K; ++k) {
        uint16_t pc[3][64][8];
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j) {
            const int co = mb * 32 + (lane & 31);
            const int pos = 8 * (lane >> 5) + j;  // MFMA k index = 16-bit position in the LDS row
            const int ci = c16 * 16 + (quad_perm ? 4 * quad_pos(pos >> 2) + (pos & 3) : pos);
            const float v = (co < Cout && ci < Cin) ? w[((int64_t)co * Cin + ci) * K + k] : 0.f;
            if (NP == 3) split3_host(v, pc[0][lane][j], pc[1][lane][j], pc[2][lane][j]);
            else if (NP == 2) split_h3_host(std::ldexp(v, -e), pc[0][lane][j], pc[1][lane][j]);
            else pc[0][lane][j] = f2bf_rne(v);
          }
        for (int p = 0; p < NP; ++p)
          for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j) out[o++] = pc[p][lane][j];
      }
  for (int i = 0; i < 4 * NP * 64 * 8; ++i) out[o++] = 0;
  return e;
}

int pack_convT_split(int mode, const float* w, int Cin, int Cout, int U, const ConvTile& t, float* out) {
  // y[co][U*m + s - U/2] = sum_ci W[ci][co][s] x[ci][m] + W[ci][co][s+U] x[ci][m-1]
  // -> conv weight w'[co*U + s][ci][tap]: tap 0 reads x[m-1], tap 1 reads x[m]
  const int K = 2 * U;
  std::vector<float> wc((size_t)U * Cout * Cin * 2);
  for (int co = 0; co < Cout; ++co)
    for (int s = 0; s < U; ++s)
      for (int ci = 0; ci < Cin; ++ci) {
        const float* src = w + ((int64_t)ci * Cout + co) * K;
        float* dst = wc.data() + (((size_t)co * U + s) * Cin + ci) * 2;
        dst[0] = src[s + U];
        dst[1] = src[s];
      }
  return pack_conv1d_split(mode, wc.data(), U * Cout, Cin, 2, t, out);
}

int64_t packed_convT_numel(int Cin, int Cout, int U, const ConvTile& t) {
  const int64_t mtiles = ceil_div(Cout, t.BM);
  const int64_t chunks = ceil_div(Cin, t.CK);
  return mtiles * chunks * 2 * U * t.CK * t.BM;
}

// torch ConvTranspose1d weight w[Cin][Cout][2U] -> out[mt][c][tap][ci_l][co_l]
void pack_convT(const float* w, int Cin, int Cout, int U, const ConvTile& t, float* out) {
  const int K = 2 * U;
  const int mtiles = ceil_div(Cout, t.BM);
  const int chunks = ceil_div(Cin, t.CK);
  int64_t o = 0;
  for (int mt = 0; mt < mtiles; ++mt)
    for (int c = 0; c < chunks; ++c)
      for (int k = 0; k < K; ++k)
        for (int cl = 0; cl < t.CK; ++cl)
          for (int ml = 0; ml < t.BM; ++ml) {
            const int co = mt * t.BM + ml;
            const int ci = c * t.CK + cl;
            out[o++] = (co < Cout && ci < Cin) ? w[((int64_t)ci * Cout + co) * K + k] : 0.f;
          }
}

// U_c[p][co][ci] = gc[p] * sum_k ga[p]^k w[co][ci][4c + k]  (fp64, taps >= K are zero), laid out as
// the 7*NCH "taps" s = c*7 + p of an ordinary split-mode conv weight, then packed by
// pack_conv1d_split (one power-of-two scale for all points: see split_device.hpp / DESIGN.md).
int pack_conv1d_wino(int mode, const float* w, int Cout, int Cin, int K, const ConvTile& t, float* out) {
  const int nch = wino_chunks(K);
  const int KS = kWinoPoints * nch;
  std::vector<float> wt((size_t)Cout * Cin * KS);
  for (int64_t oc = 0; oc < (int64_t)Cout * Cin; ++oc) {
    const float* src = w + oc * K;
    float* dst = wt.data() + oc * KS;
    for (int c = 0; c < nch; ++c)
      for (int p = 0; p < kWinoPoints; ++p) {
        double acc = 0.0;
        for (int k = 0; k < 4; ++k) {
          const int tap = 4 * c + k;
          if (tap >= K) continue;
          const double g = p == 6 ? (k == 3 ? 1.0 : 0.0) : (p == 0 ? (k == 0 ? 1.0 : 0.0) : std::pow(kWinoGa[p], k));
          acc += g * (double)src[tap];
        }
        dst[c * kWinoPoints + p] = (float)(kWinoGc[p] * acc);
      }
  }
  // channel order within each 16-channel group: the transform jobs store channels 4q + 2jp + e
  // (quad q, pair jp, e = 0, 1) at 16-bit position 2 (q + 4 jp) + e of the staged row, so that a
  // 32-lane store covers all banks; the MFMA k index runs over those positions
  TTS_REQUIRE(Cin % 16 == 0, 1, "winograd packing: Cin must be a multiple of 16");
  std::vector<float> wp(wt.size());
  for (int64_t o = 0; o < Cout; ++o)
    for (int g = 0; g < Cin / 16; ++g)
      for (int kk = 0; kk < 16; ++kk) {
        const int jp = kk >> 3, q = (kk >> 1) & 3, e = kk & 1;
        const int ch = 4 * q + 2 * jp + e;
        std::copy_n(wt.data() + ((size_t)o * Cin + g * 16 + ch) * KS, KS, wp.data() + ((size_t)o * Cin + g * 16 + kk) * KS);
      }
  return pack_conv1d_split(mode, wp.data(), Cout, Cin, KS, t, out, /*quad_perm=*/false);
}

// ---- windowed DFT matrix of the linear-spectrogram GEMM (layout: stft.hpp) ----
int stft_pieces(int mode) { return split_pieces(mode); }

int64_t packed_stft_numel16(int mode, int n_fft) {
  return (int64_t)stft_blocks(n_fft) * (n_fft / 16) * 2 * split_pieces(mode) * 512;
}

double stft_matrix_entry(const float* window, int win_length, int n_fft, int c, int row, int n) {
  const int left = (n_fft - win_length) / 2;
  if (n < left || n >= left + win_length) return 0.0;
  const double w = (double)window[n - left];
  if (row == 0 && c == 1) return (n & 1) ? -w : w;  // the Nyquist bin in the DC bin's im slot
  if (row >= n_fft / 2) return 0.0;
  // the angle from (k n) mod n_fft: exact integer reduction, so large k n loses nothing
  const double ang = 2.0 * M_PI * (double)(((int64_t)row * n) % n_fft) / (double)n_fft;
  return c == 0 ? w * std::cos(ang) : -w * std::sin(ang);
}

int pack_stft_matrix(int mode, const float* window, int win_length, int n_fft, uint16_t* out) {
  const int NP = split_pieces(mode);
  const int nblk = stft_blocks(n_fft), nsteps = n_fft / 16;
  int e = 0;
  if (mode == MATH_FP32_F16X3) {
    float m = 0.f;
    bool finite = true;
    for (int i = 0; i < win_length; ++i) {
      finite = finite && std::isfinite(window[i]);
      m = std::max(m, std::fabs(window[i]));  // |entry| <= |window|, reached at bin 0
    }
    TTS_REQUIRE(finite, 1, "stft window contains inf/NaN");
    if (m > 0.f) {
      int E;
      (void)std::frexp(m, &E);
      e = E - 14;
    }
  }
  int64_t o = 0;
  for (int blk = 0; blk < nblk; ++blk)
    for (int s = 0; s < nsteps; ++s)
      for (int c = 0; c < 2; ++c) {
        uint16_t pc[3][64][8];
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j) {
            const float v = (float)stft_matrix_entry(window, win_length, n_fft, c, blk * 32 + (lane & 31),
                                                     s * 16 + 8 * (lane >> 5) + j);
            if (NP == 3) split3_host(v, pc[0][lane][j], pc[1][lane][j], pc[2][lane][j]);
            else if (NP == 2) split_h3_host(std::ldexp(v, -e), pc[0][lane][j], pc[1][lane][j]);
            else pc[0][lane][j] = f2bf_rne(v);
          }
        for (int p = 0; p < NP; ++p)
          for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j) out[o++] = pc[p][lane][j];
      }
  return e;
}

// ---- MelGAN residual block (melgan.hpp): A1 = W1 by (group, tap), A2 = [W2 | Ws], 32-row blocks ----
int melgan_pieces(int mode) { return split_pieces(mode); }

int64_t packed_melgan_a1_numel16(int mode, int C) {
  return (int64_t)melgan_mblocks(C) * 3 * melgan_groups(C) * split_pieces(mode) * 512;
}

int64_t packed_melgan_a2_numel16(int mode, int C) {
  return (int64_t)melgan_mblocks(C) * 2 * melgan_groups(C) * split_pieces(mode) * 512;
}

float melgan_a1_entry(const float* w1, int C, int row, int col) {
  const int s = col / 16, g = s / 3, k = s % 3, ci = 16 * g + col % 16;
  return (row < C && ci < C) ? w1[((int64_t)row * C + ci) * 3 + k] : 0.f;
}

float melgan_a2_entry(const float* w2, const float* ws, int C, int row, int col) {
  const int G = melgan_groups(C), s = col / 16;
  const int ci = 16 * (s < G ? s : s - G) + col % 16;
  if (row >= C || ci >= C) return 0.f;
  return (s < G ? w2 : ws)[(int64_t)row * C + ci];
}

namespace {
template <class F>
void pack_melgan_a(int mode, int MB, int nsteps, uint16_t* out, F&& entry) {
  const int NP = split_pieces(mode);
  int64_t o = 0;
  for (int mb = 0; mb < MB; ++mb)
    for (int s = 0; s < nsteps; ++s) {
      uint16_t pc[3][64][8];
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const float v = entry(mb * 32 + (lane & 31), s * 16 + 8 * (lane >> 5) + j);
          if (NP == 3) split3_host(v, pc[0][lane][j], pc[1][lane][j], pc[2][lane][j]);
          else pc[0][lane][j] = f2bf_rne(v);
        }
      for (int p = 0; p < NP; ++p)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j) out[o++] = pc[p][lane][j];
    }
}
}  // namespace

void pack_melgan_block(int mode, const float* w1, const float* b1, const float* w2, const float* b2,
                       const float* ws, const float* bs, int C, uint16_t* a1, uint16_t* a2, float* bias1,
                       float* bias2) {
  TTS_REQUIRE(mode == MATH_FP32_X6 || mode == MATH_BF16, 3, "melgan block: math mode must be fp32x6 or bf16");
  TTS_REQUIRE(C >= 1 && C <= kMelganMaxC, 3, "melgan block: channels must lie in [1, 256]");
  const int MB = melgan_mblocks(C), G = melgan_groups(C);
  pack_melgan_a(mode, MB, 3 * G, a1, [&](int row, int col) { return melgan_a1_entry(w1, C, row, col); });
  pack_melgan_a(mode, MB, 2 * G, a2, [&](int row, int col) { return melgan_a2_entry(w2, ws, C, row, col); });
  for (int r = 0; r < 32 * MB; ++r) {
    bias1[r] = r < C ? b1[r] : 0.f;
    bias2[r] = r < C ? b2[r] + bs[r] : 0.f;
  }
}

// ---- Conv2d 3x3 / 1x1 (conv2d.hpp): step (g KS + kf) KS + kt, 32-row blocks, the MelGAN fragment order ----
int conv2d_pieces(int mode) { return split_pieces(conv2d_mode(mode)); }

int64_t packed_conv2d_numel16(int mode, int Cout, int Cin, int KS) {
  return (int64_t)conv2d_mblocks(Cout) * KS * KS * conv2d_groups(Cin) * conv2d_pieces(mode) * 512;
}

void pack_conv2d(int mode, const float* w, int Cout, int Cin, int KS, uint16_t* out) {
  TTS_REQUIRE(mode == MATH_FP32_X6 || mode == MATH_BF16, 3, "conv2d: math mode must be fp32x6 or bf16");
  TTS_REQUIRE(KS == 3 || KS == 1, 3, "conv2d: the kernel must be 3x3 (pad 1) or 1x1 (pad 0)");
  TTS_REQUIRE(Cout >= 1 && Cout <= kConv2dMaxCout, 3, "conv2d: output channels must lie in [1, 4096]");
  TTS_REQUIRE(Cin >= 1 && w && out, 1, "conv2d: bad weights");
  const int KK = KS * KS;
  pack_melgan_a(mode, conv2d_mblocks(Cout), KK * conv2d_groups(Cin), out, [&](int row, int col) {
    const int s = col / 16, g = s / KK, k = s % KK, ci = 16 * g + col % 16;
    return (row < Cout && ci < Cin) ? w[((int64_t)row * Cin + ci) * KK + k] : 0.f;
  });
}

void pack_conv2d_epilogue(const float* bias, const float* scale, const float* shift, int Cout, float* bias_p,
                          float* scale_p, float* shift_p) {
  for (int r = 0; r < 32 * conv2d_mblocks(Cout); ++r) {
    bias_p[r] = (bias && r < Cout) ? bias[r] : 0.f;
    scale_p[r] = (scale && r < Cout) ? scale[r] : 1.f;
    shift_p[r] = (shift && r < Cout) ? shift[r] : 0.f;
  }
}

// ---- skinny recurrent products (tacotron2.hpp): out[rb][k][j] = W[row(16 rb + j)][k], k < Kp ----
int64_t packed_skinny_numel(int R, int K, bool bf16) {
  const int64_t n = (int64_t)ceil_div(R, kSkinnyRows) * skinny_kp(K) * kSkinnyRows;
  return bf16 ? n / 2 : n;
}

int64_t packed_lstm_numel(int H, int K, bool bf16) {
  TTS_REQUIRE(H >= kLstmUnitBlock && H % kLstmUnitBlock == 0, 3,
              "LSTM: the hidden size must be a multiple of " + std::to_string(kLstmUnitBlock));
  return packed_skinny_numel(4 * H, K, bf16);
}

namespace {
// entry(row, k): the value of packed row `row` (< 16 * blocks), column k (< K)
template <class F>
void pack_skinny(int blocks, int K, bool bf16, float* out, F&& entry) {
  const int Kp = skinny_kp(K);
  uint16_t* out16 = reinterpret_cast<uint16_t*>(out);
  int64_t o = 0;
  for (int rb = 0; rb < blocks; ++rb)
    for (int k = 0; k < Kp; ++k)
      for (int j = 0; j < kSkinnyRows; ++j, ++o) {
        const float v = k < K ? entry(rb * kSkinnyRows + j, k) : 0.f;
        if (bf16) out16[o] = f2bf_rne(v);
        else out[o] = v;
      }
}
}  // namespace

void pack_lstm(const float* w_ih, const float* w_hh, int H, int I, bool bf16, float* out) {
  TTS_REQUIRE(H >= kLstmUnitBlock && H % kLstmUnitBlock == 0, 3,
              "LSTM: the hidden size must be a multiple of " + std::to_string(kLstmUnitBlock));
  TTS_REQUIRE(I >= 0 && w_hh && (I == 0 || w_ih), 1, "LSTM: bad weights");
  pack_skinny(H / kLstmUnitBlock, I + H, bf16, out, [&](int row, int k) {
    const int unit = row / 4, g = row % 4;  // 16 ub + 4 u + g = 4 (4 ub + u) + g
    const int64_t r = (int64_t)g * H + unit;
    return k < I ? w_ih[r * I + k] : w_hh[r * H + (k - I)];
  });
}

void pack_lstm_bias(const float* b_ih, const float* b_hh, int H, float* out) {
  for (int unit = 0; unit < H; ++unit)
    for (int g = 0; g < 4; ++g)
      out[4 * unit + g] = (b_ih ? b_ih[g * H + unit] : 0.f) + (b_hh ? b_hh[g * H + unit] : 0.f);
}

void pack_skinny_rows(const float* w, int R, int K, bool bf16, float* out) {
  TTS_REQUIRE(R >= 1 && K >= 1 && w, 1, "skinny product: bad weights");
  pack_skinny(ceil_div(R, kSkinnyRows), K, bf16, out,
              [&](int row, int k) { return row < R ? w[(int64_t)row * K + k] : 0.f; });
}

// HF Conv1D (xtts_gpt.hpp): w [K][R], y = x w + b, so packed row `row` is column `row` of w
void pack_skinny_cols(const float* w, int K, int R, bool bf16, float* out) {
  TTS_REQUIRE(R >= 1 && K >= 1 && w, 1, "skinny product: bad weights");
  pack_skinny(ceil_div(R, kSkinnyRows), K, bf16, out,
              [&](int row, int k) { return row < R ? w[(int64_t)k * R + row] : 0.f; });
}

// ---- XTTS conditioning (xtts_cond.hpp) ----
int cond_groupnorm_groups(int channels) {
  int g = 32;
  if (channels <= 16) g = 8;
  else if (channels <= 64) g = 16;
  while (g > 1 && channels % g != 0) g /= 2;
  return g;
}

int cond_qkv_source_row(int r, int E, int heads) {
  const int dk = E / heads;
  const int part = r / E, c = r % E;  // part: 0 q, 1 k, 2 v
  const int h = c / dk, d = c % dk;
  return h * 3 * dk + part * dk + d;
}

void pack_cond_qkv(const float* w, const float* b, int E, int heads, float* w_out, float* b_out) {
  TTS_REQUIRE(w && b && w_out && b_out, 1, "qkv permutation: NULL argument");
  TTS_REQUIRE(E >= 1 && heads >= 1 && E % heads == 0, 1, "qkv permutation: the channels must divide into the heads");
  for (int r = 0; r < 3 * E; ++r) {
    const int src = cond_qkv_source_row(r, E, heads);
    std::memcpy(w_out + (size_t)r * E, w + (size_t)src * E, (size_t)E * sizeof(float));
    b_out[r] = b[src];
  }
}

int64_t cond_rows_numel(int64_t n, bool bf16) { return bf16 ? (n + 1) / 2 : n; }

void pack_cond_rows(const float* w, int64_t n, bool bf16, float* out) {
  TTS_REQUIRE(w && out && n >= 1, 1, "perceiver matrix: bad weights");
  if (!bf16) {
    std::memcpy(out, w, (size_t)n * sizeof(float));
    return;
  }
  uint16_t* o = reinterpret_cast<uint16_t*>(out);
  for (int64_t i = 0; i < n; ++i) {
    uint32_t u;
    std::memcpy(&u, &w[i], 4);
    u += 0x7fffu + ((u >> 16) & 1u);  // round to nearest even
    o[i] = (uint16_t)(u >> 16);
  }
  if (n & 1) o[n] = 0;
}

int resample_width(int o, int n) {
  const double base = std::min(o, n) * 0.99;
  return (int)std::ceil(6.0 * o / base);
}

void build_resample_table(int o, int n, float* out) {
  TTS_REQUIRE(o >= 1 && n >= 1 && out, 1, "resample: bad ratio");
  const double kPi = 3.14159265358979323846;
  const double base = std::min(o, n) * 0.99;
  const int w = resample_width(o, n), taps = 2 * w + o;
  for (int p = 0; p < n; ++p)
    for (int k = 0; k < taps; ++k) {
      double t = (-(double)p / n + (double)(k - w) / o) * base;
      t = std::max(-6.0, std::min(6.0, t));
      const double c = std::cos(t * kPi / 12.0);
      const double a = t * kPi;
      const double sinc = a == 0.0 ? 1.0 : std::sin(a) / a;
      out[(size_t)k * n + p] = (float)(sinc * c * c * base / o);
    }
}

}  // namespace tts
