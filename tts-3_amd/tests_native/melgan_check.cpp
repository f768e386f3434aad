// Host-side check of the MelGAN residual-block packer (pack_melgan_block, csrc/pack.cpp), built with
// AddressSanitizer and UndefinedBehaviorSanitizer by `make -C tts-3_amd asan-check-melgan`.  The
// output buffers have exactly packed_melgan_a{1,2}_numel16 / 32 MB elements, so a write past one is
// an ASan heap-buffer-overflow.  The fragments are decoded back,
//   out[mb][step][piece][lane][j] = piece(A)[32 mb + (lane & 31)][16 step + 8 (lane >> 5) + j]
// and compared with the torch weights indexed directly here (not through the packer's helpers):
//   A1 step 3 g + k: W1[row][16 g + j][k];  A2 step s < G: W2[row][16 s + j], step G + g: Ws[row][16 g + j]
// with rows and channels >= C zero (C = 48 pads 16 rows and, in A1 / A2, no column; C = 40 pads both).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "melgan.hpp"

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

static float bf2f(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

static std::vector<float> noise(size_t n, unsigned seed) {
  std::vector<float> v(n);
  unsigned s = seed;
  for (auto& x : v) {
    s = s * 1664525u + 1013904223u;
    x = ((float)(s >> 8) / (float)(1u << 24) - 0.5f) * 0.37f;
  }
  return v;
}

static void check(int mode, int C) {
  const int NP = melgan_pieces(mode), MB = melgan_mblocks(C), G = melgan_groups(C);
  const auto w1 = noise((size_t)C * C * 3, 1 + C), w2 = noise((size_t)C * C, 2 + C), ws = noise((size_t)C * C, 3 + C);
  const auto b1 = noise(C, 4), b2 = noise(C, 5), bs = noise(C, 6);
  std::vector<uint16_t> a1((size_t)packed_melgan_a1_numel16(mode, C)), a2((size_t)packed_melgan_a2_numel16(mode, C));
  CHECK(a1.size() == (size_t)MB * 3 * G * NP * 512 && a2.size() == (size_t)MB * 2 * G * NP * 512, "numel C %d", C);
  std::vector<float> bias1((size_t)32 * MB), bias2((size_t)32 * MB);
  pack_melgan_block(mode, w1.data(), b1.data(), w2.data(), b2.data(), ws.data(), bs.data(), C, a1.data(), a2.data(),
                    bias1.data(), bias2.data());
  auto decode = [&](const std::vector<uint16_t>& a, int nsteps, int row, int col) {
    const int mb = row / 32, lane = (row % 32) + 32 * ((col % 16) / 8), j = col % 8, step = col / 16;
    double v = 0.0;
    for (int q = 0; q < NP; ++q) v += (double)bf2f(a[((((size_t)mb * nsteps + step) * NP + q) * 64 + lane) * 8 + j]);
    return v;
  };
  auto close = [&](double got, double want) {
    // x6 keeps the fp32 value exactly, bf16 one rounding (2^-9)
    return std::fabs(got - want) <= (mode == MATH_BF16 ? std::ldexp(std::fabs(want), -8) : 0.0);
  };
  for (int row = 0; row < 32 * MB; ++row) {
    for (int col = 0; col < 48 * G; ++col) {
      const int s = col / 16, g = s / 3, k = s % 3, ci = 16 * g + col % 16;
      const double want = (row < C && ci < C) ? (double)w1[((size_t)row * C + ci) * 3 + k] : 0.0;
      if (!close(decode(a1, 3 * G, row, col), want)) {
        CHECK(false, "A1 mode %d C %d row %d col %d: got %.9g want %.9g", mode, C, row, col, decode(a1, 3 * G, row, col), want);
        return;
      }
    }
    for (int col = 0; col < 32 * G; ++col) {
      const int s = col / 16, ci = 16 * (s < G ? s : s - G) + col % 16;
      const double want = (row < C && ci < C) ? (double)(s < G ? w2 : ws)[(size_t)row * C + ci] : 0.0;
      if (!close(decode(a2, 2 * G, row, col), want)) {
        CHECK(false, "A2 mode %d C %d row %d col %d: got %.9g want %.9g", mode, C, row, col, decode(a2, 2 * G, row, col), want);
        return;
      }
    }
    CHECK(bias1[row] == (row < C ? b1[row] : 0.f), "bias1 row %d", row);
    CHECK(bias2[row] == (row < C ? b2[row] + bs[row] : 0.f), "bias2 row %d", row);
  }
}

int main() {
  const int modes[] = {MATH_FP32_X6, MATH_BF16};
  const int chans[] = {1, 32, 40, 48, 96, 192, 256};
  for (int m : modes)
    for (int c : chans) check(m, c);
  // outside the implemented range: clean errors, nothing written
  {
    std::vector<float> w(4, 0.f);
    std::vector<uint16_t> a(1);
    bool threw = false;
    try {
      pack_melgan_block(MATH_FP32_F16X3, w.data(), w.data(), w.data(), w.data(), w.data(), w.data(), 1, a.data(), a.data(),
                        w.data(), w.data());
    } catch (const Error& e) {
      threw = e.code == 3;
    }
    CHECK(threw, "f16x3 must raise TTS_ERR_UNSUPPORTED");
    threw = false;
    try {
      pack_melgan_block(MATH_BF16, w.data(), w.data(), w.data(), w.data(), w.data(), w.data(), 257, a.data(), a.data(),
                        w.data(), w.data());
    } catch (const Error& e) {
      threw = e.code == 3;
    }
    CHECK(threw, "C = 257 must raise TTS_ERR_UNSUPPORTED");
  }
  if (failures) {
    std::fprintf(stderr, "%d melgan check(s) failed\n", failures);
    return 1;
  }
  std::printf("melgan_check: residual-block packer OK\n");
  return 0;
}
