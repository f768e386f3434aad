// Host-side check of the XTTS GPT packers (pack_skinny_cols for the HF Conv1D matrices, pack_skinny_rows
// for mel_head, csrc/pack.cpp), built with AddressSanitizer and UndefinedBehaviorSanitizer by
// `make -C tts-3_amd asan-check-gpt`.  The output buffers have exactly packed_skinny_numel elements, so
// a write past one is an ASan heap-buffer-overflow.  The image is decoded back,
//   out[rb][k][j] = W[k][16 rb + j] (Conv1D, [in][out])  or  W[16 rb + j][k] (Linear, [out][in]),
// k < Kp = K rounded up to 64: every weight must appear exactly once, at its place, and every padded
// row and column must be zero.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "xtts_gpt.hpp"

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

// distinct nonzero values: weight i is i + 1 (exact in fp32 below 2^24), so a weight that appears
// twice or not at all shows in the census
static void check(int K, int R, bool cols, bool bf16) {
  const int Kp = (K + 63) / 64 * 64, RB = (R + 15) / 16;
  std::vector<float> w((size_t)K * R);
  for (size_t i = 0; i < w.size(); ++i) w[i] = bf16 ? (float)((i % 251) + 1) : (float)(i + 1);
  const int64_t n = packed_skinny_numel(R, K, bf16);
  CHECK(n == (int64_t)RB * Kp * 16 / (bf16 ? 2 : 1), "numel K %d R %d", K, R);
  std::vector<float> out((size_t)n);
  if (cols) pack_skinny_cols(w.data(), K, R, bf16, out.data());
  else pack_skinny_rows(w.data(), R, K, bf16, out.data());
  const uint16_t* out16 = reinterpret_cast<const uint16_t*>(out.data());
  std::vector<int> seen(w.size(), 0);
  for (int row = 0; row < 16 * RB; ++row)
    for (int k = 0; k < Kp; ++k) {
      const size_t o = ((size_t)(row / 16) * Kp + k) * 16 + row % 16;
      const float got = bf16 ? bf2f(out16[o]) : out[o];
      if (row >= R || k >= K) {
        CHECK(got == 0.f, "K %d R %d cols %d bf16 %d: padding at row %d k %d is %.9g", K, R, (int)cols, (int)bf16, row,
              k, got);
        continue;
      }
      const size_t src = cols ? (size_t)k * R + row : (size_t)row * K + k;
      ++seen[src];
      if (got != w[src]) {  // the bf16 values are integers below 256: exact in 8 bits
        CHECK(false, "K %d R %d cols %d bf16 %d row %d k %d: got %.9g want %.9g", K, R, (int)cols, (int)bf16, row, k,
              got, w[src]);
        return;
      }
    }
  for (size_t i = 0; i < seen.size(); ++i)
    if (seen[i] != 1) {
      CHECK(false, "K %d R %d cols %d: weight %zu appears %d times", K, R, (int)cols, i, seen[i]);
      return;
    }
}

int main() {
  // (K, R) of c_attn, attn.c_proj, c_fc, mlp.c_proj at the narrow and the reference widths, and
  // shapes with padded rows and columns
  const int conv1d[][2] = {{128, 384}, {128, 128}, {128, 512}, {512, 128}, {1024, 3072}, {1024, 1024},
                           {1024, 4096}, {4096, 1024}, {70, 21}, {1, 1}};
  for (auto& s : conv1d)
    for (int bf16 = 0; bf16 < 2; ++bf16) check(s[0], s[1], true, bf16 != 0);
  const int linear[][2] = {{128, 67}, {1024, 1026}, {64, 8194}};  // mel_head: (E, n_audio)
  for (auto& s : linear)
    for (int bf16 = 0; bf16 < 2; ++bf16) check(s[0], s[1], false, bf16 != 0);
  {  // a Conv1D weight with one nonzero entry: w[in = 3][out = 5] lands at packed row 5, column 3
    const int K = 64, R = 32;
    std::vector<float> w((size_t)K * R, 0.f), out((size_t)packed_skinny_numel(R, K, false));
    w[(size_t)3 * R + 5] = 2.5f;
    pack_skinny_cols(w.data(), K, R, false, out.data());
    for (size_t o = 0; o < out.size(); ++o)
      CHECK(out[o] == (o == ((size_t)0 * K + 3) * 16 + 5 ? 2.5f : 0.f), "single entry: out[%zu] = %.9g", o, out[o]);
  }
  if (failures) {
    std::fprintf(stderr, "%d gpt pack check(s) failed\n", failures);
    return 1;
  }
  std::printf("gpt_pack_check: GPT packers OK\n");
  return 0;
}
