// Host-side check of the Conv2d packer (pack_conv2d / pack_conv2d_epilogue, csrc/pack.cpp), built
// with AddressSanitizer and UndefinedBehaviorSanitizer by `make -C tts-3_amd asan-check-conv2d`.  The
// output buffers have exactly packed_conv2d_numel16 / 32 MB elements, so a write past one is an ASan
// heap-buffer-overflow.  The fragments are decoded back,
//   out[mb][step][piece][lane][j] = piece(w)[32 mb + (lane & 31)][16 g + 8 (lane >> 5) + j][kf][kt],
//   step = (g KS + kf) KS + kt
// and compared with the torch-layout weights w[co][ci][kf][kt] indexed directly here (not through the
// packer's helpers), rows >= Cout and channels >= Cin zero: (Cout, Cin) = (16, 1) and (40, 24) pad
// both, (32, 16) and (256, 256) neither, (288, 8) has a second 256-row group, (64, 32) / (128, 64) are the downsample shapes.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "conv2d.hpp"

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

static void check(int mode, int Cout, int Cin, int KS) {
  const int NP = conv2d_pieces(mode), MB = conv2d_mblocks(Cout), G = conv2d_groups(Cin), KK = KS * KS;
  const auto w = noise((size_t)Cout * Cin * KK, 1 + Cout + 7 * Cin + KS);
  std::vector<uint16_t> a((size_t)packed_conv2d_numel16(mode, Cout, Cin, KS));
  CHECK(a.size() == (size_t)MB * KK * G * NP * 512, "numel Cout %d Cin %d KS %d", Cout, Cin, KS);
  CHECK(NP == (mode == MATH_BF16 ? 1 : 3), "pieces of mode %d", mode);
  pack_conv2d(conv2d_mode(mode), w.data(), Cout, Cin, KS, a.data());
  const int nsteps = KK * G;
  for (int row = 0; row < 32 * MB; ++row)
    for (int g = 0; g < G; ++g)
      for (int kf = 0; kf < KS; ++kf)
        for (int kt = 0; kt < KS; ++kt)
          for (int c = 0; c < 16; ++c) {
            const int step = (g * KS + kf) * KS + kt, ci = 16 * g + c;
            const int mb = row / 32, lane = (row % 32) + 32 * (c / 8), j = c % 8;
            double got = 0.0;
            for (int q = 0; q < NP; ++q) got += (double)bf2f(a[((((size_t)mb * nsteps + step) * NP + q) * 64 + lane) * 8 + j]);
            const double want = (row < Cout && ci < Cin) ? (double)w[(((size_t)row * Cin + ci) * KS + kf) * KS + kt] : 0.0;
            // x6 keeps the fp32 value exactly, bf16 one rounding (2^-9)
            const double tol = conv2d_mode(mode) == MATH_BF16 ? std::ldexp(std::fabs(want), -8) : 0.0;
            if (std::fabs(got - want) > tol) {
              CHECK(false, "mode %d Cout %d Cin %d KS %d row %d ci %d tap (%d, %d): got %.9g want %.9g", mode, Cout, Cin, KS,
                    row, ci, kf, kt, got, want);
              return;
            }
          }
  // epilogue vectors: given, and the NULL defaults (0 / 1 / 0); rows >= Cout padded the same way
  const auto b = noise(Cout, 4), sc = noise(Cout, 5), sh = noise(Cout, 6);
  std::vector<float> bp((size_t)32 * MB), sp((size_t)32 * MB), tp((size_t)32 * MB);
  pack_conv2d_epilogue(b.data(), sc.data(), sh.data(), Cout, bp.data(), sp.data(), tp.data());
  for (int r = 0; r < 32 * MB; ++r)
    CHECK(bp[r] == (r < Cout ? b[r] : 0.f) && sp[r] == (r < Cout ? sc[r] : 1.f) && tp[r] == (r < Cout ? sh[r] : 0.f),
          "epilogue row %d", r);
  pack_conv2d_epilogue(nullptr, nullptr, nullptr, Cout, bp.data(), sp.data(), tp.data());
  for (int r = 0; r < 32 * MB; ++r) CHECK(bp[r] == 0.f && sp[r] == 1.f && tp[r] == 0.f, "default epilogue row %d", r);
}

template <class F>
static bool throws_unsupported(F&& f) {
  try {
    f();
  } catch (const Error& e) {
    return e.code == 3;
  }
  return false;
}

int main() {
  const int modes[] = {MATH_FP32, MATH_FP32_X6, MATH_FP32_F16X3, MATH_BF16};
  const int shapes[][2] = {{16, 1}, {32, 16}, {40, 24}, {64, 32}, {128, 64}, {256, 256}, {288, 8}};
  for (int m : modes)
    for (const auto& s : shapes)
      for (int ks : {3, 1}) check(m, s[0], s[1], ks);
  // outside the implemented range: clean errors, nothing written
  {
    std::vector<float> w(4, 0.f);
    std::vector<uint16_t> a(1);
    CHECK(throws_unsupported([&] { pack_conv2d(MATH_BF16, w.data(), 1, 1, 5, a.data()); }), "KS = 5 must raise TTS_ERR_UNSUPPORTED");
    CHECK(throws_unsupported([&] { pack_conv2d(MATH_BF16, w.data(), 4097, 1, 3, a.data()); }),
          "Cout = 4097 must raise TTS_ERR_UNSUPPORTED");
    CHECK(throws_unsupported([&] { pack_conv2d(MATH_FP32_F16X3, w.data(), 1, 1, 3, a.data()); }),
          "an unmapped f16x3 must raise TTS_ERR_UNSUPPORTED");
  }
  if (failures) {
    std::fprintf(stderr, "%d conv2d check(s) failed\n", failures);
    return 1;
  }
  std::printf("conv2d_pack_check: conv2d packer OK\n");
  return 0;
}
