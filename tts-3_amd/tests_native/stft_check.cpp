// Host-side check of the linear-spectrogram op's DFT-matrix packer (pack_stft_matrix, csrc/pack.cpp),
// built with AddressSanitizer and UndefinedBehaviorSanitizer by `make -C tts-3_amd asan-check-stft`.
// The output buffer has exactly packed_stft_numel16 elements, so a write past it is an ASan
// heap-buffer-overflow.  The fragments are decoded back,
//   out[blk][step][c][piece][lane][j] = piece(c ? im : re)[32 blk + (lane & 31)][16 step + 8 (lane >> 5) + j]
// and compared with a direct fp64 evaluation written out here (not the packer's helper):
//   re[k][n] = wpad[n] cos(2 pi k n / n_fft), im[k][n] = -wpad[n] sin(2 pi k n / n_fft),
//   im[0][n] = wpad[n] cos(pi n) (the Nyquist bin in the DC bin's slot), rows k >= n_fft/2 zero.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "stft.hpp"

using namespace tts;

static int failures = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      std::fprintf(stderr, "FAIL: " __VA_ARGS__); \
      std::fprintf(stderr, "\n");                 \
      ++failures;                                 \
    }                                             \
  } while (0)

static float h2f(uint16_t h) {
  _Float16 v;
  std::memcpy(&v, &h, 2);
  return (float)v;
}
static float bf2f(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// torch.hann_window(win) (periodic), evaluated in fp32 like the reference
static std::vector<float> hann(int win) {
  std::vector<float> w(win);
  for (int i = 0; i < win; ++i) w[i] = 0.5f - 0.5f * std::cos(2.0f * (float)M_PI * (float)i / (float)win);
  return w;
}

static double direct(const std::vector<float>& w, int n_fft, int c, int row, int n) {
  const int win = (int)w.size(), left = (n_fft - win) / 2;
  const double wp = (n >= left && n < left + win) ? (double)w[n - left] : 0.0;
  if (row == 0 && c == 1) return wp * std::cos(M_PI * n);
  if (row >= n_fft / 2) return 0.0;
  const long double ang = 2.0L * 3.14159265358979323846264338327950288L * (long double)row * (long double)n / (long double)n_fft;
  return c == 0 ? wp * (double)std::cos(ang) : -wp * (double)std::sin(ang);
}

static void check(int mode, int n_fft, int win) {
  const auto w = hann(win);
  const int NP = stft_pieces(mode);
  const int nblk = stft_blocks(n_fft), nsteps = n_fft / 16;
  std::vector<uint16_t> out((size_t)packed_stft_numel16(mode, n_fft));
  CHECK(out.size() == (size_t)nblk * nsteps * 2 * NP * 512, "numel n_fft %d", n_fft);
  const int e = pack_stft_matrix(mode, w.data(), win, n_fft, out.data());
  CHECK(mode == MATH_FP32_F16X3 || e == 0, "scale exponent in mode %d", mode);
  auto decode = [&](int c, int row, int n) {
    const int blk = row / 32, lane = (row % 32) + 32 * ((n % 16) / 8), j = n % 8, step = n / 16;
    auto piece = [&](int q) { return out[(((((size_t)blk * nsteps + step) * 2 + c) * NP + q) * 64 + lane) * 8 + j]; };
    if (mode == MATH_FP32_F16X3) return std::ldexp((double)h2f(piece(0)) + (double)h2f(piece(1)), e);
    if (mode == MATH_BF16) return (double)bf2f(piece(0));
    return (double)bf2f(piece(0)) + (double)bf2f(piece(1)) + (double)bf2f(piece(2));
  };
  // every row of the first, a middle and the last block (its padded rows included) x a spread of n
  const int rows = nblk * 32;
  for (int row = 0; row < rows; ++row) {
    const int blk = row / 32;
    if (blk != 0 && blk != nblk / 2 && blk != nblk - 1) continue;
    for (int n = 0; n < n_fft; n += (row % 7 == 0 ? 1 : 37)) {
      for (int c = 0; c < 2; ++c) {
        const double want = direct(w, n_fft, c, row, n), got = decode(c, row, n);
        // entries are fp32-rounded (2^-24) before the split; x6 keeps fp32 exactly, f16x3 22 bits of
        // the scaled value (max-abs in [2^13, 2^14)), bf16 one rounding (2^-9)
        const double tol = mode == MATH_FP32_X6 ? std::ldexp(std::fabs(want), -24) + 1e-12
                         : mode == MATH_FP32_F16X3 ? std::ldexp(1.0, e + 14 - 22) + std::ldexp(std::fabs(want), -24)
                                                   : std::ldexp(std::fabs(want), -8) + 1e-12;
        if (!(std::fabs(got - want) <= tol)) {
          CHECK(false, "mode %d n_fft %d win %d c %d row %d n %d: got %.9g want %.9g", mode, n_fft, win, c, row, n,
                got, want);
          return;
        }
        if (row >= n_fft / 2 && !(row == 0 && c == 1)) CHECK(got == 0.0, "padded row %d not zero", row);
      }
    }
  }
}

int main() {
  const int modes[] = {MATH_FP32_X6, MATH_FP32_F16X3, MATH_BF16};
  const int cfgs[][2] = {{1024, 1024}, {1024, 800}, {512, 512}, {64, 64}, {96, 33}, {2048, 2048}, {160, 1}};
  for (int m : modes)
    for (const auto& c : cfgs) check(m, c[0], c[1]);
  // an all-zero window: scale exponent 0; a non-finite one: a clean error
  {
    std::vector<float> z(64, 0.f);
    std::vector<uint16_t> out((size_t)packed_stft_numel16(MATH_FP32_F16X3, 64));
    CHECK(pack_stft_matrix(MATH_FP32_F16X3, z.data(), 64, 64, out.data()) == 0, "zero window");
    z[3] = INFINITY;
    bool threw = false;
    try {
      pack_stft_matrix(MATH_FP32_F16X3, z.data(), 64, 64, out.data());
    } catch (const Error& e) {
      threw = e.code == 1;
    }
    CHECK(threw, "inf window must raise TTS_ERR_INVALID");
  }
  if (failures) {
    std::fprintf(stderr, "%d stft check(s) failed\n", failures);
    return 1;
  }
  std::printf("stft_check: DFT matrix packer OK\n");
  return 0;
}
