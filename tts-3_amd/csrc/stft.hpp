// Linear spectrogram (wav_to_spec of TTS/tts/models/vits.py, center=False) as a GEMM of the
// windowed DFT matrix with the wav's frames on the matrix cores (kernels_stft.hip), and its plan.
#pragma once

#include <vector>

#include "common.hpp"
#include "hifigan.hpp"
#include "tts_mi355x.h"

namespace tts {

// ---- packed DFT matrix (pack.cpp; host only) ----
// Rows come in blocks of 32 bins k = 32 blk + i, blk < stft_blocks(n_fft) = ceil((n_fft/2) / 32),
// each with a "re" row and an "im" row over n < n_fft:
//   re[k][n] =  wpad[n] cos(2 pi k n / n_fft)
//   im[k][n] = -wpad[n] sin(2 pi k n / n_fft)
// (fp64 from the fp32 window values, rounded to fp32, then split like conv weights; wpad = the
// window zero-padded to n_fft, centred).  Bins k >= n_fft/2 of the last block are zero rows.  The DC
// bin's im row is identically zero, so its slot carries the Nyquist bin instead:
//   im[0][n] = wpad[n] cos(pi n)   (X[n_fft/2] is real)
// which keeps the n_fft/2 + 1 bins in n_fft/64 full blocks (16 for n_fft = 1024, not 16 and a
// one-row 17th).  Fragment order, 16-bit units, one MFMA k-step = 16 samples:
//   out[blk][step][c][piece][lane][j] = piece(c ? im : re)[32 blk + (lane & 31)][16 step + 8 (lane >> 5) + j]
inline int stft_blocks(int n_fft) { return (n_fft / 2 + 31) / 32; }
int64_t packed_stft_numel16(int mode, int n_fft);  // 16-bit elements
// the fp32 matrix entry the packer splits (c = 0 re, 1 im; row = 32 blk + i), in fp64
double stft_matrix_entry(const float* window, int win_length, int n_fft, int c, int row, int n);
// returns the f16x3 scale exponent e (entries stored as value * 2^-e; 0 in the other modes)
int pack_stft_matrix(int mode, const float* window, int win_length, int n_fft, uint16_t* out);

void stft_validate(const TtsStftCfg& c);
// center = false: reflect padding (n_fft - hop) / 2, T = 1 + (N + 2 pad - n_fft) / hop (VITS);
// center = true: reflect padding n_fft / 2, T = 1 + N / hop (torch.stft / torchaudio at their defaults)
int stft_pad(const TtsStftCfg& c, bool center);
int stft_num_frames(const TtsStftCfg& c, int64_t N, bool center = false);

struct StftArgs {
  const float* wav;      // [B] rows of N samples, wav_bstride floats apart
  const void* a;         // packed DFT matrix
  float* spec;           // [B][n_fft/2 + 1][T]
  const unsigned* amax;  // [B][64] max-abs slots of the wav (f16x3), or nullptr
  int64_t wav_bstride;
  unsigned a_bytes;
  int N, T, n_fft, hop, pad;  // pad = stft_pad()
  int power;                  // 0: sqrt(|X|^2 + 1e-6) (wav_to_spec), 1: |X|^2 (torchaudio power = 2)
  int nblk, nsteps;           // 32-bin blocks, 16-sample k-steps
  int bn;                     // frames per workgroup (<= 32 TN)
  int nhb;                    // hop blocks of the LDS window = bn - 1 + ceil(n_fft / hop)
  int pitch, plane;           // LDS bytes per hop block / per piece plane
  int w_exp;
};
constexpr int kStftLdsLimit = 160 * 1024;
inline int stft_pitch(int hop) { return 2 * hop + ((hop / 8) % 2 == 0 ? 16 : 0); }
int stft_pieces(int mode);
// grid (tiles, B, RS): RS workgroups share a tile's row passes
void launch_stft(int mode, int TN, const StftArgs& a, int B, int tiles, int RS, hipStream_t s);

class Stft {
 public:
  // center: frame centring (above); power: the spectrogram holds |X|^2 instead of sqrt(|X|^2 + 1e-6)
  Stft(const TtsStftCfg& cfg, const float* h_window, int device, bool center = false, bool power = false);
  int num_frames(int64_t N) const { return stft_num_frames(cfg_, N, center_); }
  void forward(const float* wav, int B, int64_t N, int64_t wav_bstride, float* spec, hipStream_t s,
               Profiler* prof = nullptr);
  int device() const { return device_; }

 private:
  TtsStftCfg cfg_;
  int device_;
  bool center_ = false, power_ = false;
  DeviceBuffer a_;  // the packed DFT matrix
  int w_exp_ = 0;
  DeviceBuffer slots_;  // f16x3: [B][64] max-abs slots
};

}  // namespace tts
