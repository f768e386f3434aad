// Host-side check of the LSTM / skinny-product packers (pack_lstm, pack_lstm_bias, pack_skinny_rows,
// csrc/pack.cpp), built with AddressSanitizer and UndefinedBehaviorSanitizer by
// `make -C tts-3_amd asan-check-tacotron2`.  The output buffers have exactly packed_lstm_numel /
// packed_skinny_numel elements, so a write past one is an ASan heap-buffer-overflow.  The image is
// decoded back,
//   out[ub][k][4 u + g] = [w_ih | w_hh][g H + 4 ub + u][k],  k < Kp = K rounded up to 64, zero beyond K
// and compared with the torch weights indexed directly here (not through the packer's helpers).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "tacotron2.hpp"

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

static void check_lstm(int H, int I, bool bf16) {
  const int K = I + H, Kp = (K + 63) / 64 * 64;
  const auto w_ih = noise((size_t)4 * H * I, 1 + H), w_hh = noise((size_t)4 * H * H, 2 + I);
  const auto b_ih = noise((size_t)4 * H, 3), b_hh = noise((size_t)4 * H, 4);
  const int64_t n = packed_lstm_numel(H, K, bf16);
  CHECK(n == (int64_t)4 * H * Kp / (bf16 ? 2 : 1), "numel H %d I %d", H, I);
  std::vector<float> out((size_t)n);
  pack_lstm(w_ih.data(), w_hh.data(), H, I, bf16, out.data());
  const uint16_t* out16 = reinterpret_cast<const uint16_t*>(out.data());
  for (int unit = 0; unit < H; ++unit)
    for (int g = 0; g < 4; ++g)
      for (int k = 0; k < Kp; ++k) {
        const size_t o = ((size_t)(unit / 4) * Kp + k) * 16 + 4 * (unit % 4) + g;
        const float got = bf16 ? bf2f(out16[o]) : out[o];
        const size_t r = (size_t)g * H + unit;
        const float want = k < I ? w_ih[r * I + k] : (k < K ? w_hh[r * H + (k - I)] : 0.f);
        const float tol = bf16 ? std::ldexp(std::fabs(want), -8) : 0.f;  // one rounding to 8 bits
        if (std::fabs(got - want) > tol) {
          CHECK(false, "H %d I %d bf16 %d unit %d gate %d k %d: got %.9g want %.9g", H, I, (int)bf16, unit, g, k, got,
                want);
          return;
        }
      }
  std::vector<float> bias((size_t)4 * H);
  pack_lstm_bias(b_ih.data(), b_hh.data(), H, bias.data());
  for (int unit = 0; unit < H; ++unit)
    for (int g = 0; g < 4; ++g)
      CHECK(bias[4 * unit + g] == b_ih[g * H + unit] + b_hh[g * H + unit], "bias unit %d gate %d", unit, g);
  // the encoder's form: no input matrix (its term is precomputed), no bias
  std::vector<float> hh((size_t)packed_lstm_numel(H, H, false));
  pack_lstm(nullptr, w_hh.data(), H, 0, false, hh.data());
  const int Hp = (H + 63) / 64 * 64;
  for (int unit = 0; unit < H; ++unit)
    for (int k = 0; k < Hp; ++k)
      CHECK(hh[((size_t)(unit / 4) * Hp + k) * 16 + 4 * (unit % 4) + 2] ==
                (k < H ? w_hh[((size_t)2 * H + unit) * H + k] : 0.f),
            "w_hh-only unit %d k %d", unit, k);
}

static void check_rows(int R, int K) {
  const int Kp = (K + 63) / 64 * 64, RB = (R + 15) / 16;
  const auto w = noise((size_t)R * K, 7 + R);
  std::vector<float> out((size_t)packed_skinny_numel(R, K, false));
  CHECK(out.size() == (size_t)RB * Kp * 16, "rows numel R %d K %d", R, K);
  pack_skinny_rows(w.data(), R, K, false, out.data());
  for (int row = 0; row < 16 * RB; ++row)
    for (int k = 0; k < Kp; ++k)
      CHECK(out[((size_t)(row / 16) * Kp + k) * 16 + row % 16] == ((row < R && k < K) ? w[(size_t)row * K + k] : 0.f),
            "rows R %d K %d row %d k %d", R, K, row, k);
}

int main() {
  const int shapes[][2] = {{8, 5}, {40, 24}, {96, 160}, {256, 512}, {1024, 1792}};  // (H, I): K padded or not
  for (auto& s : shapes)
    for (int bf16 = 0; bf16 < 2; ++bf16) check_lstm(s[0], s[1], bf16 != 0);
  check_rows(40, 160);   // the narrow projection: 8 padded rows
  check_rows(160, 1536); // the reference projection
  check_rows(1, 7);
  {  // a hidden size that is no multiple of the unit block: a clean error, nothing written
    std::vector<float> w(4 * 6 * 6, 0.f), out(1);
    bool threw = false;
    try {
      pack_lstm(w.data(), w.data(), 6, 6, false, out.data());
    } catch (const Error& e) {
      threw = e.code == 3;
    }
    CHECK(threw, "H = 6 must raise TTS_ERR_UNSUPPORTED");
  }
  if (failures) {
    std::fprintf(stderr, "%d lstm pack check(s) failed\n", failures);
    return 1;
  }
  std::printf("lstm_pack_check: LSTM packer OK\n");
  return 0;
}
