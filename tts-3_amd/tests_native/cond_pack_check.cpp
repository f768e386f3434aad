// Host-side check of the XTTS conditioning host code (csrc/pack.cpp: cond_qkv_source_row, pack_cond_qkv,
// cond_groupnorm_groups, resample_width, build_resample_table), built with AddressSanitizer and
// UndefinedBehaviorSanitizer by `make -C tts-3_amd asan-check-cond`.  Every output buffer has exactly
// the advertised size, so a write past one is an ASan heap-buffer-overflow.
//   - the qkv permutation: a single entry placed in the reference's head-major interleaved rows must land
//     in the q | k | v row the attention kernel reads, and the map is a bijection at every width;
//   - the perceiver's matrices at the feed-forward's inner widths int(E ff_mult 2 / 3) = 341 (odd), 256 and
//     2730 (pack_cond_rows: fp32 copies, or bf16 pairs with an odd count padded): a single entry placed in
//     the last row and column is found exactly once, at its row-major place, and nothing else is written;
//     the conv packer at the shapes of the encoder's products (no stray write, one piece per entry; the
//     tile tables live in device translation units, so the tile here is a stand-in and the placement under
//     the executor's own tile is what the GPU parity tests at these widths check);
//   - the resample table: taps 2 w + o, each phase summing to 1 (a DC input stays DC), transposed storage.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "xtts_cond.hpp"

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

static void check_qkv(int E, int heads) {
  const int dk = E / heads;
  std::vector<int> seen((size_t)3 * E, 0);
  for (int r = 0; r < 3 * E; ++r) {
    const int src = cond_qkv_source_row(r, E, heads);
    CHECK(src >= 0 && src < 3 * E, "E %d heads %d: row %d maps to %d", E, heads, r, src);
    if (src >= 0 && src < 3 * E) ++seen[src];
    // written out: part (q, k, v), head and channel of the kernel's row
    const int part = r / E, h = (r % E) / dk, d = r % dk;
    CHECK(src == (h * 3 + part) * dk + d, "E %d heads %d: row %d maps to %d", E, heads, r, src);
  }
  for (int i = 0; i < 3 * E; ++i) CHECK(seen[i] == 1, "E %d heads %d: source row %d used %d times", E, heads, i, seen[i]);
  // single entries: the reference's row of (head, part, channel), column c
  const int probes[][3] = {{0, 0, 0}, {heads - 1, 2, dk - 1}, {heads / 2, 1, 3 % dk}, {heads - 1, 0, 1 % dk}};
  for (auto& p : probes) {
    const int h = p[0], part = p[1], d = p[2], c = (7 * h + d) % E;
    std::vector<float> w((size_t)3 * E * E, 0.f), b((size_t)3 * E, 0.f), wo((size_t)3 * E * E), bo((size_t)3 * E);
    const int src = (h * 3 + part) * dk + d;
    w[(size_t)src * E + c] = 2.5f;
    b[src] = -1.5f;
    pack_cond_qkv(w.data(), b.data(), E, heads, wo.data(), bo.data());
    const int want = part * E + h * dk + d;
    for (int r = 0; r < 3 * E; ++r) {
      CHECK(bo[r] == (r == want ? -1.5f : 0.f), "E %d heads %d: bias row %d is %.9g", E, heads, r, bo[r]);
      for (int k = 0; k < E; ++k)
        if (wo[(size_t)r * E + k] != ((r == want && k == c) ? 2.5f : 0.f)) {
          CHECK(false, "E %d heads %d: w[%d][%d] = %.9g", E, heads, r, k, wo[(size_t)r * E + k]);
          return;
        }
    }
  }
}

// a 1x1 conv [Cout][Cin] with one nonzero entry in its last row and column: exactly one nonzero piece
// group in the packed image of the advertised size, in every mode the executor packs for
static void check_conv_tail(int Cout, int Cin) {
  for (int mode : {MATH_FP32_X6, MATH_BF16}) {
    ConvTile t{};  // a split tile's packing parameters (the kernels' tile tables are device translation units)
    t.BM = 128; t.BN = 128; t.TM = 1; t.TN = 1; t.CK = 16; t.PD = 2;
    const int64_t n = packed_conv_numel(mode, Cout, Cin, 1, t);
    std::vector<float> w((size_t)Cout * Cin, 0.f), out((size_t)n, 0.f);
    w[(size_t)(Cout - 1) * Cin + (Cin - 1)] = 1.0f;  // exact in bf16: one nonzero piece
    pack_conv(mode, w.data(), Cout, Cin, 1, t, out.data());
    int nonzero = 0;
    const uint16_t* o16 = reinterpret_cast<const uint16_t*>(out.data());
    for (int64_t i = 0; i < 2 * n; ++i) nonzero += o16[i] != 0;
    CHECK(nonzero == 1, "conv %d x %d mode %d: %d nonzero 16-bit pieces for a single entry", Cout, Cin, mode, nonzero);
    std::vector<float> zero((size_t)Cout * Cin, 0.f), out0((size_t)n, 1.f);
    pack_conv(mode, zero.data(), Cout, Cin, 1, t, out0.data());
    for (int64_t i = 0; i < n; ++i)
      if (out0[(size_t)i] != 0.f) {
        CHECK(false, "conv %d x %d mode %d: padding at %lld is not zero", Cout, Cin, mode, (long long)i);
        break;
      }
  }
}

// W [R][K] with one entry at (R - 1, K - 1): row-major image, fp32 or bf16
static void check_rows(int R, int K) {
  const int64_t n = (int64_t)R * K;
  for (int bf16 = 0; bf16 < 2; ++bf16) {
    CHECK(cond_rows_numel(n, bf16 != 0) == (bf16 ? (n + 1) / 2 : n), "rows %d x %d: numel", R, K);
    std::vector<float> w((size_t)n, 0.f), out((size_t)cond_rows_numel(n, bf16 != 0), 7.f);
    w[(size_t)n - 1] = -2.5f;  // exact in bf16
    w[0] = 1.0f + 1.0f / 256;  // a bf16 tie: rounds to even (1.0)
    pack_cond_rows(w.data(), n, bf16 != 0, out.data());
    const uint16_t* o16 = reinterpret_cast<const uint16_t*>(out.data());
    for (int64_t i = 0; i < n; ++i) {
      float got;
      if (bf16) {
        const uint32_t u = (uint32_t)o16[i] << 16;
        std::memcpy(&got, &u, 4);
      } else {
        got = out[(size_t)i];
      }
      const float want = i == n - 1 ? -2.5f : (i == 0 ? (bf16 ? 1.0f : 1.0f + 1.0f / 256) : 0.f);
      if (got != want) {
        CHECK(false, "rows %d x %d bf16 %d: entry %lld is %.9g, expected %.9g", R, K, bf16, (long long)i, got, want);
        break;
      }
    }
    if (bf16 && (n & 1)) CHECK(o16[n] == 0, "rows %d x %d: the odd count's padding is not zero", R, K);
  }
}

static void check_resample(int o, int n, int want_w) {
  const int w = resample_width(o, n), taps = 2 * w + o;
  CHECK(w == want_w, "resample %d -> %d: width %d, expected %d", o, n, w, want_w);
  std::vector<float> t((size_t)taps * n);
  build_resample_table(o, n, t.data());
  for (int p = 0; p < n; ++p) {
    double s = 0.0;
    for (int k = 0; k < taps; ++k) s += t[(size_t)k * n + p];
    CHECK(std::fabs(s - 1.0) < 1e-3, "resample %d -> %d: phase %d sums to %.6f", o, n, p, s);
  }
  // phase 0 peaks at tap w (t = 0) with the value base / o
  const double base = (o < n ? o : n) * 0.99;
  CHECK(std::fabs(t[(size_t)w * n] - base / o) < 1e-6, "resample %d -> %d: centre tap %.7f", o, n, t[(size_t)w * n]);
}

int main() {
  check_qkv(128, 2);
  check_qkv(96, 3);
  check_qkv(1024, 16);
  check_qkv(32, 1);
  // the FF's matrices at the inner widths 341 (odd), 256 and 2730; 3 x 341 has an odd entry count
  check_rows(3, 341);
  const int ff[][2] = {{128, 341}, {96, 256}, {1024, 2730}};
  for (auto& s : ff) {
    check_rows(2 * s[1], s[0]);
    check_rows(s[0], s[1]);
  }
  // the convs the executor packs: init (80 -> E), qkv (E -> 3E), proj_out (E -> E), to_kv (E -> 1024)
  const int convs[][2] = {{128, 80}, {96, 80}, {1024, 80}, {384, 128}, {288, 96}, {3072, 1024}, {96, 96}, {1024, 96}};
  for (auto& c : convs) check_conv_tail(c[0], c[1]);
  const int groups[][2] = {{8, 8}, {16, 8}, {24, 8}, {64, 16}, {96, 32}, {128, 32}, {1024, 32}, {80, 16}, {100, 4}};
  for (auto& g : groups)
    CHECK(cond_groupnorm_groups(g[0]) == g[1], "groups(%d) = %d, expected %d", g[0], cond_groupnorm_groups(g[0]), g[1]);
  check_resample(441, 320, 9);   // 22 050 -> 16 000
  check_resample(160, 147, 7);   // 24 000 -> 22 050
  check_resample(147, 160, 7);   // 22 050 -> 24 000
  if (failures) {
    std::fprintf(stderr, "%d conditioning check(s) failed\n", failures);
    return 1;
  }
  std::printf("cond_pack_check: conditioning host code OK\n");
  return 0;
}
