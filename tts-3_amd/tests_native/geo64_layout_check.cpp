// Host-side check of the 64-channel f16x3 kernels' 256-column tiles on the swizzled 64-byte LDS rows
// (csrc/res3_layout.hpp), built by `make -C tts-3_amd check-geo64-layout`.  Like
// res3_layout_check.cpp it replays, lane by lane, every LDS access to the staged operands and counts
// bank conflicts with the MI355X banking of each instruction:
//   ds_read_b128   4 groups of 16 lanes {0-3,12-15,20-27}, {4-11,16-19,28-31}, the same + 32;
//                  bank = (byte / 4) mod 64
//   ds_write_b128  8 groups of 8 contiguous lanes;  bank = (byte / 4) mod 32
//   ds_write_b64   4 groups of 16 contiguous lanes; bank = (byte / 4) mod 32
//
// The pair kernel (kernels_resblock.hip, PairCfg<SchemeH3, K, 64, PD, GEO 0, ALLX, POST, SWZ>):
// 4 waves side by side, each 64 columns as two blocks of 32; the X window is NC = 4 buffers of
// XROWS = 256 + 5 (K - 1) rows, xt is 4 groups of TROWS = 288 rows in the same bytes.  An address
// is base + off(row, unit) with the row counted inside its buffer and the base a multiple of 64.
//   staging stores    row r of buffer c, channel quad at position 4 qp: 8 bytes at
//                     off(r, qp / 2 + 2 p) + 8 (qp & 1), rows r < 256 + (K - 1) d
//   tap reads         row xrow0 + k d, + 32 n rows as an immediate; d = 1, 3, 5, K = 3, 7, 11
//   store_xt8         row xrow0 of group (row block, gl), + 32 n rows
//   phase-2 reads     row xrow0 + k, k = 0 .. K - 1 (row offsets 0 .. 10)
// The whole-block kernel (resblock_block.hpp, Res3Cfg<SchemeH3, 64, GEO 0, .., SW>): 4 groups of
// PR = 266 rows counted through the whole region, X offset 5: the prologue's stores, store_pieces
// at row offsets 5 and 1, the taps of convs1 (dilations 1, 3, 5), convs2 and the two-tap tail.
// Asserted: every read group touches 64 distinct banks, every store group is at most 2-way
// conflicted, every address stays inside its buffer and the kernel's LDS array, and a read returns
// the bytes the store of the same (buffer, row, unit) wrote (the + 32 n rows rule).
#include <algorithm>
#include <cstdio>
#include <vector>

#include "common.hpp"
#include "res3_layout.hpp"

using namespace tts;

static int failures = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      if (failures < 20) {                        \
        std::fprintf(stderr, "FAIL: " __VA_ARGS__); \
        std::fprintf(stderr, "\n");               \
      }                                           \
      ++failures;                                 \
    }                                             \
  } while (0)

using R = Res3Rows<2, true>;
constexpr int NP = 2, NC = 4, RP_W = 256, NT = 256, PITCH = R::PITCH;
static long n_reads = 0, n_stores = 0;

// worst conflict of one lane group: lanes' byte addresses (-1: inactive), `dw` dwords each, `banks`
// banks; the largest number of distinct dword addresses on one bank
static int worst(const std::vector<int>& addr, const std::vector<int>& lanes, int dw, int banks) {
  std::vector<std::vector<int>> on(banks);
  for (int l : lanes) {
    if (addr[l] < 0) continue;
    for (int j = 0; j < dw; ++j) {
      const int d = addr[l] / 4 + j;
      auto& v = on[d % banks];
      if (std::find(v.begin(), v.end(), d) == v.end()) v.push_back(d);
    }
  }
  size_t w = 0;
  for (const auto& v : on) w = std::max(w, v.size());
  return (int)w;
}

static std::vector<std::vector<int>> read128_groups() {
  const int a[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                        {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
  std::vector<std::vector<int>> g;
  for (int h = 0; h < 2; ++h)
    for (int s = 0; s < 2; ++s) {
      std::vector<int> v;
      for (int i = 0; i < 16; ++i) v.push_back(a[s][i] + 32 * h);
      g.push_back(v);
    }
  return g;
}
static std::vector<std::vector<int>> contiguous_groups(int n) {
  std::vector<std::vector<int>> g;
  for (int l0 = 0; l0 < 64; l0 += n) {
    std::vector<int> v;
    for (int i = 0; i < n; ++i) v.push_back(l0 + i);
    g.push_back(v);
  }
  return g;
}

static const std::vector<std::vector<int>> RG = read128_groups(), W8 = contiguous_groups(8), W16 = contiguous_groups(16);

static void expect_read(const std::vector<int>& addr, const char* what, int a, int b, int c, int d) {
  for (const auto& grp : RG)
    CHECK(worst(addr, grp, 4, 64) == 1, "%s: ds_read_b128 conflict (%d %d %d %d)", what, a, b, c, d);
  ++n_reads;
}
static void expect_store(const std::vector<int>& addr, bool b128, const char* what, int a, int b, int c, int d) {
  for (const auto& grp : b128 ? W8 : W16)
    CHECK(worst(addr, grp, b128 ? 4 : 2, 32) <= 2, "%s: %s conflict above 2-way (%d %d %d %d)", what,
          b128 ? "ds_write_b128" : "ds_write_b64", a, b, c, d);
  ++n_stores;
}

// ---- the pair kernel, kernel size K
static void check_pair(int K) {
  const int XROWS = RP_W + (K - 1) * 5, XSZB = XROWS * PITCH, TROWS = RP_W + 32;
  const int LDSB = std::max(NC * XSZB, NC * TROWS * PITCH);
  const int UPT = (XROWS * 4 + NT - 1) / NT;
  CHECK(LDSB + 4 * 4 + 2 * 64 * 4 + 64 * 7 * 4 <= 80 * 1024, "pair k%d: LDS %d B does not fit twice", K, LDSB);
  std::vector<int> addr(64);
  for (int d : {1, 3, 5}) {
    const int XW = RP_W + (K - 1) * d;
    // staging stores (RES_STAGE_8R lane map)
    for (int c = 0; c < NC; ++c)
      for (int i = 0; i < UPT; ++i)
        for (int wave = 0; wave < 4; ++wave)
          for (int p = 0; p < NP; ++p) {
            for (int lane = 0; lane < 64; ++lane) {
              const int u = wave * 64 + lane + i * NT;
              const int q = quad_pos((u >> 3) & 3), r = (u >> 5) * 8 + (u & 7), qp = quad_pos(q);
              const int ulds = r < XW ? R::off(r, qp >> 1) + 8 * (qp & 1) : -1;
              addr[lane] = ulds < 0 ? -1 : c * XSZB + R::piece(ulds, p);
              if (ulds >= 0) {
                CHECK(addr[lane] >= c * XSZB + r * PITCH && addr[lane] + 8 <= c * XSZB + (r + 1) * PITCH,
                      "pair k%d: staging store leaves row %d of buffer %d", K, r, c);
                CHECK(addr[lane] == c * XSZB + R::off(r, (qp >> 1) + 2 * p) + 8 * (qp & 1), "pair k%d: staging piece()", K);
              }
            }
            expect_store(addr, false, "pair staging", K, d, c, i);
          }
    // tap reads of phase 1
    for (int c = 0; c < NC; ++c)
      for (int wn = 0; wn < 4; ++wn)
        for (int n = 0; n < 2; ++n)
          for (int k = 0; k < K; ++k)
            for (int q = 0; q < NP; ++q) {
              for (int lane = 0; lane < 64; ++lane) {
                const int half = lane >> 5, row = wn * 64 + (lane & 31) + k * d;
                addr[lane] = c * XSZB + R::piece(R::off(row, half), q) + n * 32 * PITCH;
                CHECK(row + n * 32 < XW, "pair k%d: tap read of an unstaged row %d", K, row + n * 32);
                CHECK(addr[lane] == c * XSZB + R::off(row + n * 32, half + 2 * q), "pair k%d: read and store disagree, row %d",
                      K, row + n * 32);
              }
              expect_read(addr, "pair tap", K, d, c, k);
            }
  }
  // store_xt8 and the phase-2 reads (row offsets 0 .. K - 1)
  for (int g = 0; g < NC; ++g)
    for (int wn = 0; wn < 4; ++wn)
      for (int n = 0; n < 2; ++n) {
        for (int p = 0; p < NP; ++p) {
          for (int lane = 0; lane < 64; ++lane) {
            const int half = lane >> 5, row = wn * 64 + (lane & 31);
            addr[lane] = (g * TROWS + n * 32) * PITCH + R::piece(R::off(row, half), p);
            CHECK(addr[lane] == g * TROWS * PITCH + R::off(row + n * 32, half + 2 * p), "pair k%d: store_xt8 unit map", K);
            CHECK(addr[lane] + 16 <= LDSB, "pair k%d: store_xt8 leaves the LDS array", K);
          }
          expect_store(addr, true, "pair store_xt8", K, g, wn, n);
        }
        for (int k = 0; k <= 10; ++k)
          for (int q = 0; q < NP; ++q) {
            for (int lane = 0; lane < 64; ++lane) {
              const int half = lane >> 5, row = wn * 64 + (lane & 31) + k;
              addr[lane] = (g * TROWS + n * 32) * PITCH + R::piece(R::off(row, half), q);
              CHECK(row + n * 32 < TROWS, "pair k%d: phase-2 read past the zero rows", K);
              CHECK(addr[lane] == g * TROWS * PITCH + R::off(row + n * 32, half + 2 * q), "pair k%d: phase-2 unit map", K);
              CHECK(addr[lane] + 16 <= LDSB, "pair k%d: phase-2 read leaves the LDS array", K);
            }
            expect_read(addr, "pair phase 2", K, g, wn, k);
          }
      }
}

// ---- the whole-block kernel at 64 channels, 256 columns (rows counted through the whole region)
static void check_block() {
  constexpr int XO = 5, HK = 1, PR = RP_W + 2 * XO, LDSB = NC * PR * PITCH;
  static_assert(LDSB + 2 * 4 * 4 + 7 * 64 * 4 <= 80 * 1024, "the block fits twice");
  std::vector<int> addr(64);
  struct Tap { int roff, kstep, ntaps; };
  std::vector<Tap> taps;
  for (int d : {1, 3, 5}) taps.push_back({XO - HK * d, d, 3});  // convs1 on X rows
  taps.push_back({0, 1, 3});                                     // convs2 on xt rows
  taps.push_back({XO - 1, 1, 2});                                // the tail's two taps: columns c - 1, c
  for (const Tap& t : taps)
    for (int g = 0; g < NC; ++g)
      for (int wn = 0; wn < 4; ++wn)
        for (int n = 0; n < 2; ++n)
          for (int k = 0; k < t.ntaps; ++k)
            for (int q = 0; q < NP; ++q) {
              for (int lane = 0; lane < 64; ++lane) {
                const int half = lane >> 5, row = g * PR + wn * 64 + (lane & 31) + t.roff + k * t.kstep;
                addr[lane] = R::piece(R::off(row, half), q) + n * 32 * PITCH;
                CHECK(row + n * 32 >= g * PR && row + n * 32 < (g + 1) * PR, "block: read row outside group %d", g);
                CHECK(addr[lane] == R::off(row + n * 32, half + 2 * q), "block: read unit map, row %d", row + n * 32);
              }
              expect_read(addr, "block tap", t.roff, t.kstep, g, k);
            }
  for (int roff : {XO, HK})
    for (int g = 0; g < NC; ++g)
      for (int wn = 0; wn < 4; ++wn)
        for (int n = 0; n < 2; ++n)
          for (int p = 0; p < NP; ++p) {
            for (int lane = 0; lane < 64; ++lane) {
              const int half = lane >> 5, row = g * PR + wn * 64 + (lane & 31) + roff;
              addr[lane] = R::piece(R::off(row, half), p) + n * 32 * PITCH;
              CHECK(addr[lane] == R::off(row + n * 32, half + 2 * p), "block: store_pieces unit map");
              CHECK(addr[lane] + 16 <= LDSB, "block: store_pieces leaves the LDS array");
            }
            expect_store(addr, true, "block store_pieces", roff, g, wn, n);
          }
  for (int g = 0; g < NC; ++g)
    for (int u0 = 0; u0 < ((PR * 4 + NT - 1) / NT) * NT; u0 += 64)
      for (int p = 0; p < NP; ++p) {
        for (int lane = 0; lane < 64; ++lane) {
          const int u = u0 + lane;
          const int q = quad_pos((u >> 3) & 3), r = (u >> 5) * 8 + (u & 7), qp = quad_pos(q);
          addr[lane] = r < PR ? R::off(g * PR + r, (qp >> 1) + 2 * p) + 8 * (qp & 1) : -1;
        }
        expect_store(addr, false, "block prologue", g, u0, p, 0);
      }
}

int main() {
  static_assert(R::PITCH == 64 && R::SWIZZLED, "the swizzled two-piece row");
  for (int K : {3, 7, 11}) check_pair(K);
  check_block();
  // the replay must see what the swizzle is for: plain 64-byte rows read 4-way conflicted
  {
    std::vector<int> addr(64);
    for (int lane = 0; lane < 64; ++lane) addr[lane] = (lane & 31) * 64 + 16 * (lane >> 5);
    CHECK(worst(addr, RG[0], 4, 64) == 4, "the replay does not see the 4-way conflict of plain 64-byte rows");
  }
  if (failures) {
    std::fprintf(stderr, "%d layout check(s) failed\n", failures);
    return 1;
  }
  std::printf("geo64_layout_check: %ld read and %ld store instructions replayed: reads conflict-free, stores at most 2-way\n",
              n_reads, n_stores);
  return 0;
}
