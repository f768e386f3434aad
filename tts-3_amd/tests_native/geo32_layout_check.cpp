// Host-side check of the 32-channel f16x3 whole block's 512-column tile on the swizzled 64-byte LDS
// rows (csrc/res3_layout.hpp), built by `make -C tts-3_amd check-geo32-layout`.  Like
// geo64_layout_check.cpp it replays, lane by lane, every LDS access to the staged operands and counts
// bank conflicts with the MI355X banking of each instruction:
//   ds_read_b128   4 groups of 16 lanes {0-3,12-15,20-27}, {4-11,16-19,28-31}, the same + 32;
//                  bank = (byte / 4) mod 64
//   ds_write_b128  8 groups of 8 contiguous lanes;  bank = (byte / 4) mod 32
//   ds_write_b64   4 groups of 16 contiguous lanes; bank = (byte / 4) mod 32
//
// The kernel (resblock_block.hpp, Res3Cfg<SchemeH3, 32, GEO 5, K, 6, r3_xoff(K), r3_lead(K)>; K = 7,
// 11 are launched, K = 3 is replayed as well): 4 waves side by side, each 32 rows x 128 columns as
// four blocks of 32 columns; NC = 2 groups of PR = 512 + 2 XO rows counted through the whole region,
// XO = 5 (K - 1) / 2.
//   prologue stores   row r of group g, channel quad at position 4 qp: 8 bytes at
//                     off(g PR + r, qp / 2 + 2 p) + 8 (qp & 1), r < PR
//   store_pieces      row g PR + column + roff, roff = XO (X rows) or (K - 1) / 2 (xt rows), + 32 n
//                     rows, then whole edge rows [0, roff) and [roff + 512, PR) zeroed 16 bytes a lane
//   taps              convs1: row column + XO + (k - HK) d, d = 1, 3, 5 (offsets up to +-25 at K = 11);
//                     convs2: row column + k, k = 0 .. K - 1; + 32 n rows
// Asserted: every read group touches 64 distinct banks, every store group is at most 2-way
// conflicted, every address stays inside its group's rows and the kernel's LDS array, a read returns
// the bytes the store of the same (group, row, unit) wrote (the + 32 n rows rule), and the edge
// zeroing covers exactly the rows store_pieces leaves out.
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
constexpr int NP = 2, NC = 2, RP_W = 512, NT = 256, TN = 4, C = 32, NCV = 6, PITCH = R::PITCH;
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

// ---- the whole block of kernel size K on 512 columns (rows counted through the whole region)
static void check_block(int K) {
  const int HK = (K - 1) / 2, XO = 5 * HK, LEAD = 12 * HK, PR = RP_W + 2 * XO, LDSB = NC * PR * PITCH;
  CHECK(LDSB == 2 * (512 + 2 * XO) * 64, "k%d: LDS region %d B", K, LDSB);
  CHECK(LDSB + 2 * 4 * 4 + NCV * C * 4 <= 80 * 1024, "k%d: LDS %d B does not fit twice", K, LDSB);
  CHECK(RP_W - 2 * LEAD == (K == 3 ? 488 : (K == 7 ? 440 : 392)), "k%d: kept columns", K);
  std::vector<int> addr(64);
  struct Tap { int roff, kstep; };
  std::vector<Tap> taps;
  for (int d : {1, 3, 5}) taps.push_back({XO - HK * d, d});  // convs1 on X rows: column + XO + (k - HK) d
  taps.push_back({0, 1});                                    // convs2 on xt rows: column + k
  for (const Tap& t : taps) {
    CHECK(t.roff >= 0 && t.roff + (K - 1) * t.kstep <= 2 * XO, "k%d: tap offsets leave the staged rows", K);
    CHECK(t.kstep == 1 || (t.roff - XO == -HK * t.kstep && HK * t.kstep <= 25), "k%d: offsets up to +-25", K);
    for (int g = 0; g < NC; ++g)
      for (int wn = 0; wn < 4; ++wn)
        for (int n = 0; n < TN; ++n)
          for (int k = 0; k < K; ++k)
            for (int q = 0; q < NP; ++q) {
              for (int lane = 0; lane < 64; ++lane) {
                const int half = lane >> 5, row = g * PR + wn * TN * 32 + (lane & 31) + t.roff + k * t.kstep;
                addr[lane] = R::piece(R::off(row, half), q) + n * 32 * PITCH;
                CHECK(row + n * 32 >= g * PR && row + n * 32 < (g + 1) * PR, "k%d: read row outside group %d", K, g);
                CHECK(addr[lane] >= 0 && addr[lane] + 16 <= LDSB, "k%d: read leaves the LDS array", K);
                CHECK(addr[lane] == R::off(row + n * 32, half + 2 * q), "k%d: read unit map, row %d", K, row + n * 32);
              }
              expect_read(addr, "block tap", K, t.roff, t.kstep, k);
            }
  }
  for (int roff : {XO, HK}) {
    for (int g = 0; g < NC; ++g)
      for (int wn = 0; wn < 4; ++wn)
        for (int n = 0; n < TN; ++n)
          for (int p = 0; p < NP; ++p) {
            for (int lane = 0; lane < 64; ++lane) {
              const int half = lane >> 5, row = g * PR + wn * TN * 32 + (lane & 31) + roff;
              addr[lane] = R::piece(R::off(row, half), p) + n * 32 * PITCH;
              CHECK(row + n * 32 >= g * PR + roff && row + n * 32 < g * PR + roff + RP_W, "k%d: store_pieces row", K);
              CHECK(addr[lane] == R::off(row + n * 32, half + 2 * p), "k%d: store_pieces unit map", K);
              CHECK(addr[lane] >= 0 && addr[lane] + 16 <= LDSB, "k%d: store_pieces leaves the LDS array", K);
            }
            expect_store(addr, true, "block store_pieces", K, roff, g, wn * TN + n);
          }
    // the edge rows: every thread's 16-byte stores, as the kernel's loop walks them
    const int EB = 2 * XO * PITCH, lead_b = roff * PITCH, tail_b = (PR - roff - RP_W) * PITCH;
    std::vector<int> zeroed(LDSB / 16, 0);
    for (int e0 = 0; e0 < NC * EB; e0 += NT * 16)
      for (int wave = 0; wave < 4; ++wave) {
        for (int lane = 0; lane < 64; ++lane) {
          const int e = e0 + (wave * 64 + lane) * 16;
          addr[lane] = -1;
          if (e >= NC * EB) continue;
          const int g = e / EB, o = e - g * EB;
          if (o < lead_b) addr[lane] = g * PR * PITCH + o;
          else if (o - lead_b < tail_b) addr[lane] = (g * PR + roff + RP_W) * PITCH + (o - lead_b);
          if (addr[lane] >= 0) {
            CHECK(addr[lane] + 16 <= LDSB, "k%d: edge zeroing leaves the LDS array", K);
            ++zeroed[addr[lane] / 16];
          }
        }
        expect_store(addr, true, "block edge rows", K, roff, e0, wave);
      }
    for (int g = 0; g < NC; ++g)
      for (int r = 0; r < PR; ++r)
        for (int u = 0; u < 4; ++u) {
          const bool edge = r < roff || r >= roff + RP_W;
          CHECK(zeroed[((g * PR + r) * PITCH + 16 * u) / 16] == (edge ? 1 : 0), "k%d: edge zeroing of row %d (roff %d)", K, r, roff);
        }
  }
  // the prologue's 8-byte stores (RES_STAGE_8R lane map): every (row, channel quad) once
  std::vector<int> staged(LDSB / 8, 0);
  for (int g = 0; g < NC; ++g)
    for (int u0 = 0; u0 < ((PR * 4 + NT - 1) / NT) * NT; u0 += 64)
      for (int p = 0; p < NP; ++p) {
        for (int lane = 0; lane < 64; ++lane) {
          const int u = u0 + lane;
          const int q = quad_pos((u >> 3) & 3), r = (u >> 5) * 8 + (u & 7), qp = quad_pos(q);
          addr[lane] = r < PR ? R::off(g * PR + r, (qp >> 1) + 2 * p) + 8 * (qp & 1) : -1;
          if (addr[lane] >= 0) {
            CHECK(addr[lane] >= (g * PR + r) * PITCH && addr[lane] + 8 <= (g * PR + r + 1) * PITCH,
                  "k%d: prologue store leaves row %d of group %d", K, r, g);
            ++staged[addr[lane] / 8];
          }
        }
        expect_store(addr, false, "block prologue", K, g, u0, p);
      }
  for (int s : staged) CHECK(s == 1, "k%d: the prologue stages an 8-byte slot %d times", K, s);
}

int main() {
  static_assert(R::PITCH == 64 && R::SWIZZLED, "the swizzled two-piece row");
  for (int K : {3, 7, 11}) check_block(K);
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
  std::printf("geo32_layout_check: %ld read and %ld store instructions replayed: reads conflict-free, stores at most 2-way\n",
              n_reads, n_stores);
  return 0;
}
