// Plan of the linear-spectrogram op (tts_stft_*): validation, the packed DFT matrix on the device,
// the launch geometry.  Kernel: kernels_stft.hip; packer: pack.cpp.
#include "stft.hpp"

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

namespace tts {

void stft_validate(const TtsStftCfg& c) {
  TTS_REQUIRE(c.math_mode >= MATH_FP32 && c.math_mode <= MATH_LAST, 1, "stft: unknown math_mode");
  TTS_REQUIRE(c.n_fft >= 1 && c.hop_length >= 1, 1, "stft: n_fft and hop_length must be positive");
  TTS_REQUIRE(c.win_length >= 1 && c.win_length <= c.n_fft, 1, "stft: win_length must lie in [1, n_fft]");
  TTS_REQUIRE(c.n_fft % 32 == 0 && c.n_fft >= 64 && c.n_fft <= 2048, 3,
              "stft: n_fft must be a multiple of 32 in [64, 2048]");
  TTS_REQUIRE(c.hop_length % 8 == 0 && c.hop_length <= c.n_fft, 3,
              "stft: hop_length must be a multiple of 8 in [8, n_fft]");
  TTS_REQUIRE(c.math_mode != MATH_FP32, 3,
              "stft: no TTS_MATH_FP32 kernel; use TTS_MATH_FP32_X6 (fp32-exact products) or TTS_MATH_FP32_F16X3");
}

int stft_pad(const TtsStftCfg& c, bool center) { return center ? c.n_fft / 2 : (c.n_fft - c.hop_length) / 2; }

int stft_num_frames(const TtsStftCfg& c, int64_t N, bool center) {
  stft_validate(c);
  const int64_t p = stft_pad(c, center);
  if (center) TTS_REQUIRE(N > p, 1, "stft: the wav must be longer than the reflect padding n_fft / 2");
  TTS_REQUIRE(N > p, 1, "stft: the wav must be longer than the reflect padding (n_fft - hop_length) / 2");
  TTS_REQUIRE(N + 2 * p >= c.n_fft, 1, "stft: the padded wav is shorter than one frame");
  TTS_REQUIRE(N * 4 < (int64_t)1 << 31, 3, "stft: a wav row must stay below 2 GiB");
  const int64_t T = 1 + (N + 2 * p - c.n_fft) / c.hop_length;  // center: 1 + N / hop
  TTS_REQUIRE((int64_t)(c.n_fft / 2 + 1) * T * 4 < (int64_t)1 << 31, 3, "stft: a spectrogram must stay below 2 GiB");
  return (int)T;
}

Stft::Stft(const TtsStftCfg& cfg, const float* h_window, int device, bool center, bool power)
    : cfg_(cfg), device_(device), center_(center), power_(power) {
  stft_validate(cfg);
  std::vector<uint16_t> packed((size_t)packed_stft_numel16(cfg.math_mode, cfg.n_fft));
  w_exp_ = pack_stft_matrix(cfg.math_mode, h_window, cfg.win_length, cfg.n_fft, packed.data());
  a_.grow(device_, packed.size() * sizeof(uint16_t), "the DFT matrix");
  DeviceGuard g(device_);
  TTS_HIP_CHECK(hipMemcpy(a_.as<void>(), packed.data(), a_.bytes(), hipMemcpyHostToDevice));
}

void Stft::forward(const float* wav, int B, int64_t N, int64_t wav_bstride, float* spec, hipStream_t s,
                   Profiler* prof) {
  TTS_REQUIRE(wav && spec, 1, "stft: NULL argument");
  TTS_REQUIRE(B >= 1 && B <= 65535, 1, "stft: batch size must lie in [1, 65535]");
  const int T = stft_num_frames(cfg_, N, center_);
  if (wav_bstride == 0) wav_bstride = N;
  TTS_REQUIRE(wav_bstride >= 0, 1, "stft: negative wav_bstride");
  const int mode = cfg_.math_mode;
  const int NP = stft_pieces(mode);
  const int hop = cfg_.hop_length, n_fft = cfg_.n_fft;
  DeviceGuard g(device_);

  StftArgs a{};
  a.wav = wav;
  a.a = a_.as<void>();
  a.spec = spec;
  a.wav_bstride = wav_bstride;
  a.a_bytes = (unsigned)a_.bytes();
  a.N = (int)N;
  a.T = T;
  a.n_fft = n_fft;
  a.hop = hop;
  a.pad = stft_pad(cfg_, center_);
  a.power = power_ ? 1 : 0;
  a.nblk = stft_blocks(n_fft);
  a.nsteps = n_fft / 16;
  a.w_exp = w_exp_;
  a.pitch = stft_pitch(hop);
  // frames per workgroup: 64 (two column blocks per wave) when that still fills the device, else 32;
  // fewer when the window of that many frames would not fit the LDS (large hops: the spare MFMA
  // columns then idle)
  const int fpb = (n_fft + hop - 1) / hop;  // hop blocks of one frame
  const int bn_max = kStftLdsLimit / (NP * a.pitch) + 1 - fpb;
  TTS_REQUIRE(bn_max >= 1, 3, "stft: one frame does not fit the LDS");
  int TN = ((int64_t)B * ((T + 63) / 64) >= 256 && bn_max > 32) ? 2 : 1;
  // TTS_MI355X_STFT_TN = 1 / 2 forces the column blocks per wave (tests run both at small shapes)
  if (const char* e = std::getenv("TTS_MI355X_STFT_TN")) {
    const int v = std::atoi(e);
    TTS_REQUIRE(v == 1 || v == 2, 1, "TTS_MI355X_STFT_TN must be 1 or 2");
    TN = v;
  }
  a.bn = std::min(32 * TN, bn_max);
  a.nhb = a.bn - 1 + fpb;
  a.plane = a.nhb * a.pitch;
  const int tiles = (T + a.bn - 1) / a.bn;
  // few tiles: the row passes of a tile go to separate workgroups (each restages the window)
  const int npt = (a.nblk + 7) / 8;
  const int RS = (int64_t)B * tiles < 512 ? npt : 1;

  if (mode == MATH_FP32_F16X3) {
    slots_.grow(device_, (size_t)B * 64 * sizeof(unsigned), "stft statistics");
    unsigned* slots = slots_.as<unsigned>();
    run(prof, s, "stft_amax", 0.0, (double)B * N * 4, [&] {
      TTS_HIP_CHECK(hipMemsetAsync(slots, 0, (size_t)B * 64 * sizeof(unsigned), s));
      launch_amax(wav, N, B, slots, s, wav_bstride);
    });
    a.amax = slots;
  }
  const double bins = n_fft / 2 + 1;
  const std::string name = std::string("stft_") + (mode == MATH_FP32_F16X3 ? "f16x3" : mode == MATH_BF16 ? "bf16" : "fp32x6");
  run(prof, s, name.c_str(), 2.0 * 2.0 * bins * n_fft * (double)T * B,
      (double)B * ((double)N * 4 + bins * T * 4) + (double)a_.bytes(),
      [&] { launch_stft(mode, TN, a, B, tiles, RS, s); });
}

}  // namespace tts
