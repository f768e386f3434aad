// ---------------------------------------------------------------------------------------
// Whole-ResBlock kernels (hifigan_generator.py:84-99 ResBlock1, :150-155 ResBlock2) in one launch.
// ResBlock1, kernel 3 (NCV = 6 convs, dilations d0..d2):
//   for m in 0..2:  xt = lrelu(convs1[m](lrelu(x)));  x = convs2[m](xt) + x;   z (+)= x
// ResBlock2, any kernel K in {3, 5, 7, 11} (NCV = 2 convs, dilations d0, d1):
//   for m in 0..1:  x = convs[m](lrelu(x)) + x;                                   z (+)= x
// Every conv runs on the same RP_W-column grid (column c <-> time t0 - LEAD + c): each conv loses
// its halo (K - 1) / 2 * d at the grid edges, so the valid columns shrink per conv (ResBlock1 k3
// with dilations 1, 3, 5: 11 per side; the first conv reads XO staged extra columns, the rest only
// the grid) while the kept ones, [LEAD, RP_W - LEAD), stay exact.  x lives in the accumulator
// layout in registers (the residual of every iteration), lrelu(x) and xt alternate in one LDS
// region as split B operands (X rows: column + XO, xt rows: column + (K - 1) / 2).  Columns
// outside the valid range or outside [0, T) are staged as zeros; in the f16x3 scheme the scale of
// every staged operand after the first is the workgroup's own power of two over its valid columns
// (exact and batch-invariant), x0 uses its producer's statistics.  One launch replaces three pair
// launches (ResBlock1) or two conv launches (ResBlock2): x is read once and z written once.
// ---------------------------------------------------------------------------------------
#pragma once
#include <type_traits>

#include "res3_layout.hpp"
#include "split_device.hpp"

#ifndef RES_PD_B1
#define RES_PD_B1 2  // weight prefetch depth of the whole-block and pair kernels in the bf16 scheme
#endif
#ifndef RES_STAGE_8R
#define RES_STAGE_8R 1  // x staging lane map of the pair / whole-block kernels (0: 4 rows x 4 quads)
#endif

namespace tts {

// ResBlock1 k3: X rows hold column + 5 (convs1 halo up to dilation 5); kept columns
// [R3_LEAD, RP_W - R3_LEAD): only the first conv sees the R3_XOFF staged extra columns, every
// later one loses d_m (+ 1) columns at the grid edge, 11 for dilations 1, 3, 5
#ifndef R3_XR_POL
#define R3_XR_POL 0  // cache policy of the residual re-read (A/B)
#endif
constexpr int R3_XOFF = 5;
constexpr int R3_LEAD = 12;
// ResBlock1 of kernel K (round 5: 7 and 11 at 32 / 64 channels): every conv's halo scales by
// (K - 1) / 2, so X rows hold column + 5 (K - 1) / 2 and the kept columns lose 12 (K - 1) / 2
// (K 7: 15 / 36, K 11: 25 / 60)
constexpr int r3_xoff(int K) { return R3_XOFF * ((K - 1) / 2); }
constexpr int r3_lead(int K) { return R3_LEAD * ((K - 1) / 2); }
// ResBlock2 kernel K: XO = LEAD = (K - 1) / 2 * the largest dilation it takes (K 3: 4, K 5: 6,
// K 7 / 11: 3; HiFiGAN-v3 [[1, 2], [2, 6], [3, 12]] up to kernel 5, YourTTS (1, 3) for 3, 7, 11)
constexpr int rb2_halo(int K) { return K == 3 ? 4 : (K == 5 ? 12 : (K == 7 ? 9 : 15)); }

// GEO 0: 256 columns, 4 waves side by side; GEO 1 / 2: 192 / 128 columns, 2 x 2 waves;
// GEO 3: 128 columns, 8 waves (4 row blocks x 2 column halves at C = 128, two waves per SIMD).
// GEO 4: the tiles of GEO 2 / 3 (128 columns, 2 x 2 waves; at C = 128 a wave owns 64 rows x 64
// columns) on the swizzled 64-byte rows of res3_layout.hpp and two waves per SIMD asked of the
// compiler.  At C = 128 the two-piece scheme then stages 8 x 138 x 64 = 70,656 B instead of the
// 88,320 B of the padded 80-byte rows, so two workgroups share a CU and drift out of phase: one
// runs MFMAs while the other sits in its prologue, epilogue or barriers.
// Measured (f16x3, per batch): C = 128 GEO 4 4.28 ms vs GEO 3 4.73 ms, bitwise the same output
// (profiles/ab_block_c128_2wg.txt; earlier, GEO 3 5.0 ms vs GEO 2 5.5 ms); 8-wave forms on the
// padded rows at C = 64 (256 columns, 85 KB: one workgroup per CU) and C = 32 (512 columns) were
// slower than GEO 2 / GEO 0 (+0.2 / +0.3 ms); the 4-wave 256-column form at C = 64 on swizzled rows
// (SW below, two workgroups per CU) is faster than GEO 2: 2.37 -> 2.26 ms per launch with the
// upsampling tail (profiles/ab_geo64_wide.txt).
// SW (C = 64, the two-piece scheme): GEO 0's tile (256 columns, 4 waves side by side, each 64 rows x
// 64 columns) on the swizzled rows, with everything GEO 4 does for its 64 x 64 wave tile: 4 x 266
// x 64 = 68,096 B where the padded rows take 85,120 B, so two workgroups share a CU, and 24 of 256
// columns are halo where the 128-column GEO 2 has 24 of 128.
// UP: the upsampling tail (ResBlock3Args::up_w), one more bias row in LDS
template <class S, int C, int GEO, int K = 3, int NCV = 6, int XO = R3_XOFF, int LEAD = R3_LEAD, bool UP = false,
          bool SW = false>
struct Res3Cfg {
  static_assert(!SW || (GEO == 0 && S::NP == 2), "SW: GEO 0's tile, two-piece rows");
  static constexpr bool SWZ = (GEO == 4 || SW) && S::NP == 2;  // swizzled 64-byte rows
  static constexpr bool W64 = GEO == 4 || SW;                  // a wave owns 64 rows x 64 columns
  static constexpr int RP_W = GEO == 0 ? 256 : (GEO == 1 ? 192 : 128);
  static constexpr int RP_BN = RP_W - 2 * LEAD;
  static constexpr int NW = GEO == 3 ? 8 : 4;     // waves per workgroup
  static constexpr int NT = 64 * NW;
  static constexpr int WN = GEO == 0 ? 4 : 2;
  static constexpr int WM = NW / WN;
  static constexpr int TM = C / 32 / WM;
  static constexpr int TN = RP_W / 32 / WN;
  static constexpr int NC = C / 16;
  static constexpr int PR = RP_W + 2 * XO;  // rows per group (X: RP_W + 2 XO, xt: RP_W + K - 1)
  // row pitch and the place of a 16-byte unit inside a row: every LDS address of the kernel's
  // staged operands is ROWS::off(row, unit), unit = half + 2 piece (+ 8 bytes for the second
  // channel quad of a unit in the prologue's 8-byte stores)
  using ROWS = Res3Rows<S::NP, SWZ>;
  static_assert(SWZ || ROWS::PITCH == S::ROWB, "the padded layout is the scheme's own row");
  static constexpr int LDSB = NC * PR * ROWS::PITCH;
  // with red and bsm: what a workgroup takes of the CU's 160 KB
  static constexpr int LDS_TOTAL = LDSB + 2 * NW * 4 + (NCV + UP) * C * 4;
  static_assert(!W64 || LDS_TOTAL <= 80 * 1024, "GEO 4 / SW: two workgroups per CU");
  static_assert(TM >= 1 && TM * WM * 32 == C && TN * WN * 32 == RP_W, "geometry");
};

// GEO 5 (C = 32, the two-piece scheme, ResBlock1): 512 columns, 4 waves side by side, each 32 rows x
// 128 columns (TM 1, TN 4), on the swizzled rows with everything GEO 4 / SW do for their 64 x 64 wave
// tile (W64: operand addresses per (group, tap), scalar-offset residual and z addressing, the last
// iteration peeled, two waves per SIMD): the same 64 accumulators and 64 residual registers per
// lane, 64 B operand registers.  2 x (512 + 2 XO) x 64 B of LDS: 66,816 / 69,376 / 71,936 B at kernels
// 3 / 7 / 11, two workgroups per CU; the kept columns are 488 / 440 / 392 of 512 where GEO 0 keeps
// 232 / 184 / 136 of 256.  Launched at kernels 7 / 11 (launch_res3_s); the kernel-7 block ran 1.92 ms
// per launch where three pairs took 2.45 ms (profiles/ab_geo32_wide.txt)
template <class S, int C, int K, int NCV, int XO, int LEAD, bool UP, bool SW>
struct Res3Cfg<S, C, 5, K, NCV, XO, LEAD, UP, SW> {
  static_assert(C == 32 && S::NP == 2 && NCV == 6 && !UP && !SW, "GEO 5: the 32-channel ResBlock1, two-piece rows");
  static constexpr bool SWZ = true;
  static constexpr bool W64 = true;  // the 256-register form of the kernel
  static constexpr int RP_W = 512;
  static constexpr int RP_BN = RP_W - 2 * LEAD;
  static constexpr int NW = 4;
  static constexpr int NT = 64 * NW;
  static constexpr int WN = 4;
  static constexpr int WM = 1;
  static constexpr int TM = 1;
  static constexpr int TN = RP_W / 32 / WN;
  static constexpr int NC = C / 16;
  static constexpr int PR = RP_W + 2 * XO;
  using ROWS = Res3Rows<S::NP, SWZ>;
  static constexpr int LDSB = NC * PR * ROWS::PITCH;
  static constexpr int LDS_TOTAL = LDSB + 2 * NW * 4 + NCV * C * 4;
  static_assert(LDS_TOTAL <= 80 * 1024, "GEO 5: two workgroups per CU");
  static_assert(RP_BN > 0 && TN * WN * 32 == RP_W, "geometry");
};

#ifndef RB3_W_B1
#define RB3_W_B1 0  // A/B: waves per SIMD asked of the bf16 scheme's whole-block kernels (0: as the others)
#endif
#ifndef RB3_W64
#define RB3_W64 2  // A/B build option: waves per SIMD requested for the 64-channel 128-column block
#endif
// PL: ResBlock3Args::planes (the bf16 scheme: 0, or bf16 x and z planes; x stays fp32 in registers)
template <class S, int C, int GEO, int K, int NCV, int XO, int LEAD, int PL = 0, bool UP = false, bool SW = false>
__global__ __launch_bounds__((Res3Cfg<S, C, GEO, K, NCV, XO, LEAD>::NT))
__attribute__((amdgpu_waves_per_eu(S::NP == 1 && RB3_W_B1 > 0 ? RB3_W_B1
                                                                : (C == 64 && GEO == 2 ? RB3_W64 : (C == 32 || GEO >= 3 || SW ? 2 : 1)))))
void resblock3_kernel(ResBlock3Args a) {
  constexpr bool XB = (PL & kPlaneXB16) != 0, YB = (PL & kPlaneYB16) != 0;
  using PX = PlaneT<XB>;
  using PY = PlaneT<YB>;
  using P = Res3Cfg<S, C, GEO, K, NCV, XO, LEAD, UP, SW>;
  using ROWS = typename P::ROWS;
  static_assert(NCV == 6 || NCV == 2, "ResBlock1 (6 convs) or ResBlock2 (2 convs)");
  static_assert(!UP || (NCV == 6 && S::SCALED && PL == 0), "the upsampling tail: ResBlock1, f16x3, fp32 planes");
  constexpr int NP = S::NP;
  constexpr bool H3 = S::SCALED;
  constexpr int TM = P::TM, TN = P::TN, NC = P::NC, PR = P::PR, RP_W = P::RP_W;
  constexpr int PD = S::NP == 1 ? RES_PD_B1 : 2;  // weight prefetch steps (bf16: its own, A/B)
  __shared__ __attribute__((aligned(16))) unsigned char smem[P::LDSB];
  constexpr int NT = P::NT;
  __shared__ float red[2][P::NW];  // double-buffered: consecutive tile_exp calls use different halves
  __shared__ float bsm[(NCV + UP) * C];  // the conv biases (read by every epilogue: LDS, not L2, latency)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int half = lane >> 5;
  const int l32 = lane & 31;
  const int wm = __builtin_amdgcn_readfirstlane(wave / P::WN);
  const int wn = wave % P::WN;
  const int mrow0 = wm * TM * 32;
  const int t0 = blockIdx.x * P::RP_BN;
  const int b = blockIdx.z;
  const int T = a.T;
  const int tx0 = t0 - LEAD;  // time of column 0
  const int xcol0 = wn * TN * 32 + l32;
  const unsigned avoff = (unsigned)lane * 16u;
  const unsigned chb = (unsigned)T * PX::ES;
  const rsrc_t rx = make_rsrc(plane_at<XB>(a.x, (size_t)b * C * T), (unsigned)C * chb);
  auto ldx = [&](unsigned off, auto pol_tag, unsigned soff = 0u) -> float {
    if constexpr (XB) return PX::ld(rx, off, soff);
    else return bload_x<decltype(pol_tag)::value>(rx, off, soff);
  };
  // GEO 4 / SW / GEO 5 (256 registers for a 64 x 64 or 32 x 128 wave tile) address the accumulator
  // layout's 16 channels of a lane as one per-lane offset (column and the lane's half) plus a wave-uniform scalar
  // offset per channel, instead of 16 per-lane offsets for each of the wave's TM x TN blocks
  constexpr bool SOFF = P::W64;

  // ---- prologue: lrelu(x0) pieces for columns [-XO, RP_W + XO) of every 16-channel group, and x0
  // itself in the acc layout.  Every load is issued before the first store (one HBM latency for
  // the whole window instead of one per group: at C = 128 that is 8 groups, 64 VGPRs of window)
  int ex = H3 ? amax_exp(a.amax_in, b) : 0;
  f32x16 xr[TM][TN];  // the running residual x (fp32), accumulator layout
  {
    const float xs = H3 ? ldexpf(1.f, -ex) : 1.f;
    constexpr int UG = (PR * 4 + NT - 1) / NT;  // units (row, quad) per group per thread
    constexpr int BPT = (C + NT - 1) / NT;
    float bl[NCV][BPT];
#pragma unroll
    for (int i = 0; i < NCV; ++i)
#pragma unroll
      for (int j = 0; j < BPT; ++j) {
        const int e = tid + j * NT;
        bl[i][j] = e < C ? a.bias[i][e] : 0.f;
      }
    float blu[BPT];  // UP: the upsampler's bias
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
      const int e = tid + j * NT;
      blu[j] = UP && e < C ? a.up_bias[e] : 0.f;
    }
    f32x4 xv[NC][UG];
#pragma unroll
    for (int g = 0; g < NC; ++g)
#pragma unroll
      for (int i = 0; i < UG; ++i) {
        const int u = tid + i * NT;
        const int q = RES_STAGE_8R ? quad_pos((u >> 3) & 3) : (u & 3);
        const int r = RES_STAGE_8R ? (u >> 5) * 8 + (u & 7) : (u >> 2);
        const int ts = tx0 - XO + r;
        const bool ok = r < PR && ts >= 0 && ts < T;
        const unsigned vo = (unsigned)(16 * g + 4 * q) * chb + (unsigned)ts * PX::ES;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          xv[g][i][j] = ldx(ok ? vo + (unsigned)j * chb : OOB_OFF, std::integral_constant<int, TTS_LDX_POL>{});
      }
    // x0 in the acc layout (the residual): the same bytes as the window, so read once the window
    // has landed (L2 hits; issued together, both missed L2: 2.4x the x plane in FETCH_SIZE).  It is
    // first needed in conv 1's epilogue, so its latency hides behind conv 1's MFMAs.
    auto load_xr = [&] {
#pragma unroll
      for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int n = 0; n < TN; ++n) {
          const int t = tx0 + xcol0 + n * 32;
          const bool tok = t >= 0 && t < T;
          const unsigned vlane = tok ? (unsigned)(4 * half) * chb + (unsigned)t * PX::ES : OOB_OFF;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int co = mrow0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if constexpr (SOFF)
              xr[m][n][r] = ldx(vlane, std::integral_constant<int, R3_XR_POL>{}, (unsigned)(co - 4 * half) * chb);
            else
              xr[m][n][r] = ldx(tok ? (unsigned)co * chb + (unsigned)t * PX::ES : OOB_OFF,
                                std::integral_constant<int, R3_XR_POL>{});
          }
        }
    };
#pragma unroll
    for (int g = 0; g < NC; ++g)
#pragma unroll
      for (int i = 0; i < UG; ++i) {
        const int u = tid + i * NT;
        const int q = RES_STAGE_8R ? quad_pos((u >> 3) & 3) : (u & 3);
        const int r = RES_STAGE_8R ? (u >> 5) * 8 + (u & 7) : (u >> 2);
        if (r < PR) {
          float v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v[j] = lrelu2(xv[g][i][j], 0.1f);
            if (H3) v[j] *= xs;
          }
          // channel quad q sits at position 4 quad_pos(q): unit quad_pos(q) / 2, its low or high 8 bytes
          const int qp = quad_pos(q);
          unsigned char* dst[NP];
#pragma unroll
          for (int p = 0; p < NP; ++p) dst[p] = smem + ROWS::off(g * PR + r, (qp >> 1) + 2 * p) + 8 * (qp & 1);
          split_store4<S>(dst, v[0], v[1], v[2], v[3]);
        }
      }
    __builtin_amdgcn_sched_barrier(0);  // keep the loads below the window's use
    load_xr();
#pragma unroll
    for (int i = 0; i < NCV; ++i)
#pragma unroll
      for (int j = 0; j < BPT; ++j) {
        const int e = tid + j * NT;
        if (e < C) bsm[i * C + e] = bl[i][j];
      }
    if constexpr (UP) {
#pragma unroll
      for (int j = 0; j < BPT; ++j) {
        const int e = tid + j * NT;
        if (e < C) bsm[NCV * C + e] = blu[j];
      }
    }
  }
  __syncthreads();

  f32x16 acc[TM][TN];
  f32x4 ar[PD + 1][TM][NP], bcur[TN][NP], bnext[TN][NP];
  rsrc_t ra[TM];
  // KT taps (the block's K; 2 for the upsampling tail) of the packed conv at wp
  auto conv_k = [&](const float* wp, int roff, int kstep, auto ktag) __attribute__((always_inline)) {
    constexpr int KT = decltype(ktag)::value;
    // swizzled rows: an operand address costs a few VALU per (g, k) and is no immediate offset.
    // Keep the convs2 call (roff 0, kstep 1 in every iteration) from having its 48 addresses
    // hoisted out of the iteration loop, where they would live across the whole kernel
    if constexpr (ROWS::SWIZZLED) asm volatile("" : "+s"(roff), "+s"(kstep));
#pragma unroll
    for (int m = 0; m < TM; ++m) ra[m] = make_rsrc(wp + ((size_t)(wm * TM + m) * NC * KT) * (NP * 256), 0xFFFFFFFFu);
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
      for (int n = 0; n < TN; ++n) acc[m][n] = f32x16{};
#pragma unroll
    for (int p = 0; p < PD; ++p)
#pragma unroll
      for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int q = 0; q < NP; ++q) ar[p][m][q] = bload4(ra[m], avoff, (unsigned)(p * NP + q) * 1024u);
    auto read_b = [&](int g, int k, f32x4 (*dst)[NP]) __attribute__((always_inline)) {
#pragma unroll
      for (int n = 0; n < TN; ++n) {
        // 32 n rows further on: the same unit map (res3_layout.hpp), so one address per (g, k)
        const int o = ROWS::off(g * PR + xcol0 + roff + k * kstep, half);
#pragma unroll
        for (int q = 0; q < NP; ++q)
          dst[n][q] = *reinterpret_cast<const f32x4*>(smem + ROWS::piece(o, q) + n * 32 * ROWS::PITCH);
      }
    };
    read_b(0, 0, bcur);
#pragma unroll
    for (int g = 0; g < NC; ++g) {
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        const int st = g * KT + k;
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
          for (int q = 0; q < NP; ++q)
            ar[PD][m][q] = bload4(ra[m], avoff, (unsigned)((st + PD) * NP + q) * 1024u);
        const bool more = (k + 1 < KT) || (g + 1 < NC);
        if (more) read_b((k + 1 < KT) ? g : g + 1, (k + 1 < KT) ? k + 1 : 0, bnext);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < S::NPROD; ++e)
#pragma unroll
          for (int m = 0; m < TM; ++m)
#pragma unroll
            for (int n = 0; n < TN; ++n)
              acc[m][n] = S::mfma(ar[0][m][S::PA[e]], bcur[n][S::PB[e]], acc[m][n]);
#pragma unroll
        for (int p = 0; p < PD; ++p)
#pragma unroll
          for (int m = 0; m < TM; ++m)
#pragma unroll
            for (int q = 0; q < NP; ++q) ar[p][m][q] = ar[p + 1][m][q];
        if (more) {
#pragma unroll
          for (int n = 0; n < TN; ++n)
#pragma unroll
            for (int q = 0; q < NP; ++q) bcur[n][q] = bnext[n][q];
        }
      }
    }
  };
  auto conv = [&](int wi, int roff, int kstep) __attribute__((always_inline)) {
    conv_k(a.w[wi], roff, kstep, std::integral_constant<int, K>{});
  };
  // block max of |v| over this workgroup (f16x3 scale exponent); every wave must call it.  The
  // red halves alternate per call, and the store_pieces barrier between two calls separates a
  // half's reads from its next writes, so one barrier per call suffices
  int red_half = 0;
  auto tile_exp = [&](float vmax) __attribute__((always_inline)) -> int {
    if (!H3) return 0;
    vmax = wave_max(vmax);
    if (lane == 0) red[red_half][wave] = vmax;
    __syncthreads();  // also: every wave is done reading the LDS region
    float mx = red[red_half][0];
#pragma unroll
    for (int w = 1; w < P::NW; ++w) mx = fmaxf(mx, red[red_half][w]);
    red_half ^= 1;
    int e = 0;
    if (mx > 0.f && mx < INFINITY) {
      int E;
      (void)frexpf(mx, &E);
      e = E - 14;
    }
    return e;
  };

  // acc-layout values (already zeroed where invalid) -> split pieces at LDS row column + roff;
  // rows of the region outside [roff, roff + RP_W) are zeroed
  auto store_pieces = [&](int roff, float scale) __attribute__((always_inline)) {
    if constexpr (ROWS::SWIZZLED) asm volatile("" : "+s"(roff));  // as in conv: addresses formed here
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
      for (int n = 0; n < TN; ++n)
#pragma unroll
        for (int gl = 0; gl < 2; ++gl) {
          const int o = ROWS::off(((mrow0 + m * 32) / 16 + gl) * PR + xcol0 + roff, half);
          unsigned char* dst[NP];
#pragma unroll
          for (int p = 0; p < NP; ++p) dst[p] = smem + ROWS::piece(o, p) + n * 32 * ROWS::PITCH;
          store_xt8<S>(dst, acc[m][n], 8 * gl, scale);
        }
    // edge rows: [0, roff) and [roff + RP_W, PR) of every group.  Whole rows are zeroed, so the
    // order of the units inside a row (ROWS::unit) does not matter here, only the pitch
    constexpr int ROWB = ROWS::PITCH;
    constexpr int EB = 2 * XO * ROWB;  // upper bound of edge bytes per group
    for (int e = tid * 16; e < NC * EB; e += NT * 16) {
      const int g = e / EB;
      const int o = e - g * EB;  // byte in the edge area: first roff rows, then the tail
      const int lead_b = roff * ROWB;
      const int tail_b = (PR - roff - RP_W) * ROWB;
      if (o < lead_b) *reinterpret_cast<f32x4*>(smem + g * PR * ROWB + o) = f32x4{};
      else if (o - lead_b < tail_b)
        *reinterpret_cast<f32x4*>(smem + (g * PR + roff + RP_W) * ROWB + (o - lead_b)) = f32x4{};
    }
  };

  constexpr int HK = (K - 1) / 2;
  int lo = -XO, hi = RP_W + XO;  // valid columns of the staged operand
  // conv ci adds the residual: x = conv(.) + x; the next conv's operand lrelu(x) goes to the X
  // rows (column + XO)
  auto residual_to_lds = [&](int ci) __attribute__((always_inline)) {
    const float sc = H3 ? ldexpf(1.f, ex + a.w_exp[ci]) : 1.f;
    const float* bs = bsm + ci * C;
    float vmax = 0.f;
#pragma unroll
    for (int m = 0; m < TM; ++m) {
      float bv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) bv[r] = bs[mrow0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half];
#pragma unroll
      for (int n = 0; n < TN; ++n) {
        const int col = xcol0 + n * 32;
        const int t = tx0 + col;
        const bool ok = col >= lo && col < hi && t >= 0 && t < T;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float x1 = (acc[m][n][r] * sc + bv[r]) + xr[m][n][r];  // x = conv(.) + x
          xr[m][n][r] = x1;
          const float v = ok ? lrelu2(x1, 0.1f) : 0.f;  // the next conv's operand
          acc[m][n][r] = v;
          vmax = fmaxf(vmax, fabsf(v));
        }
      }
    }
    const int e2 = tile_exp(vmax);
    if (!H3) __syncthreads();  // every wave done reading the region
    store_pieces(XO, H3 ? ldexpf(1.f, -e2) : 1.f);
    __syncthreads();
    ex = e2;
  };
  // the block's last conv: x_out = conv(.) + x -> MRF z (kept columns [LEAD, LEAD + RP_BN) only)
  auto final_to_z = [&](int ci) __attribute__((always_inline)) {
    const float sc = H3 ? ldexpf(1.f, ex + a.w_exp[ci]) : 1.f;
    const float* bs = bsm + ci * C;
    const unsigned chbz = (unsigned)T * PY::ES;
    const rsrc_t rz = make_rsrc(plane_at<YB>(a.z, (size_t)b * C * T), (unsigned)C * chbz);
    float vmax = 0.f;
#pragma unroll
    for (int m = 0; m < TM; ++m) {
      float bv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) bv[r] = bs[mrow0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half];
#pragma unroll
      for (int n = 0; n < TN; ++n) {
        const int col = xcol0 + n * 32;
        const int t = tx0 + col;
        const bool keep = col >= LEAD && col < LEAD + P::RP_BN && t >= 0 && t < T;
        unsigned vo[16], so[16];
        float zv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = mrow0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          if constexpr (SOFF) {
            vo[r] = keep ? (unsigned)(4 * half) * chbz + (unsigned)t * PY::ES : OOB_OFF;
            so[r] = (unsigned)(co - 4 * half) * chbz;
          } else {
            vo[r] = keep ? (unsigned)co * chbz + (unsigned)t * PY::ES : OOB_OFF;
            so[r] = 0u;
          }
          zv[r] = a.zmode >= 2 ? PY::ld(rz, vo[r], so[r]) : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = (acc[m][n][r] * sc + bv[r]) + xr[m][n][r];
          if (a.zmode == 2) v = zv[r] + v;
          else if (a.zmode == 3) v = (zv[r] + v) / a.zdiv;
          if (keep) vmax = fmaxf(vmax, fabsf(v));
          PY::st(rz, v, vo[r], so[r]);
        }
      }
    }
    if (H3 && a.amax_out) publish_amax(a.amax_out, b, vmax);
  };

  // UP, the block's last conv as the stage's last MRF launch: v = the MRF mean over the block's x
  // and the other branches' planes, in the association the z plane's writers use (zmode 2 then 3:
  // (x + p0) + p1, divided by zdiv), kept in registers; lrelu(v) is staged like every other
  // operand (the tile's own scale, zeros outside the valid columns and [0, T)) and the next
  // stage's x2 ConvTranspose1d runs on it as a K = 2 conv: row rho = 2 co + s of column mm reads
  // v[mm - 1], v[mm] and is sample 2 mm + s - 1 of channel co (convT_epilogue, U = 2).  Columns
  // mm in [t0, t0 + RP_BN) are this workgroup's, and mm = T is the last workgroup's as well: both
  // of its taps are valid there (one spare valid column on either side of the kept ones,
  // resblock3_up_supported)
  auto final_up = [&](int ci) __attribute__((always_inline)) {
    const float sc = ldexpf(1.f, ex + a.w_exp[ci]);
    const float* bs = bsm + ci * C;
    const int nzp = a.nzp;
    const float zdiv = a.zdiv;
    rsrc_t rp[2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
      rp[p] = make_rsrc(p < nzp ? a.zp[p] + (size_t)b * C * T : a.x, p < nzp ? (unsigned)C * chb : 0u);
    float vmax = 0.f;
#pragma unroll
    for (int m = 0; m < TM; ++m) {
      float bv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) bv[r] = bs[mrow0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half];
#pragma unroll
      for (int n = 0; n < TN; ++n) {
        const int col = xcol0 + n * 32;
        const int t = tx0 + col;
        // only the valid columns are staged below (the rest become zeros), so only they are gathered
        const bool tok = t >= 0 && t < T && col >= lo && col < hi;
        const unsigned vlane = tok ? (unsigned)(4 * half) * chb + (unsigned)t * 4u : OOB_OFF;
        // the other branches' values, one accumulator block at a time: 32 registers, where the
        // gathers of every block at once would not fit beside acc and x (GEO 4: 128 of 256)
        __builtin_amdgcn_sched_barrier(0);
        float pv[2][16];
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            pv[p][r] = bload(rp[p], vlane, (unsigned)(mrow0 + m * 32 + (r & 3) + 8 * (r >> 2)) * chb);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = (acc[m][n][r] * sc + bv[r]) + xr[m][n][r];
          if (nzp >= 1) v = v + pv[0][r];
          if (nzp >= 2) v = v + pv[1][r];
          // the branches' sum, formed here: left to itself the compiler sinks the additions into
          // the pass below and keeps all 128 gathered values alive until then (60 spilt at GEO 4)
          asm volatile("" : "+v"(v));
          xr[m][n][r] = v;  // the conv's accumulators are dead from here
        }
      }
    }
    // the mean and the staged value in a pass of its own: the division's temporaries then sit in
    // the accumulators' registers instead of beside them (GEO 4 spilt 58 registers otherwise)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
      for (int n = 0; n < TN; ++n) {
        const int col = xcol0 + n * 32;
        const int t = tx0 + col;
        const bool ok = col >= lo && col < hi && t >= 0 && t < T;
        __builtin_amdgcn_sched_barrier(0);  // 16 divisions in flight, not 64
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = xr[m][n][r];
          if (nzp >= 1) v = v / zdiv;
          v = ok ? lrelu2(v, 0.1f) : 0.f;
          acc[m][n][r] = v;
          vmax = fmaxf(vmax, fabsf(v));
        }
      }
    const int e2 = tile_exp(vmax);
    store_pieces(XO, ldexpf(1.f, -e2));
    __syncthreads();
    ex = e2;
    conv_k(a.up_w, XO - 1, 1, std::integral_constant<int, 2>{});  // taps at X rows column - 1 + k
    const float sc2 = ldexpf(1.f, ex + a.up_w_exp);
    const float* bu = bsm + NCV * C;
    const int To = 2 * T;
    const unsigned chby = (unsigned)To * 4u;
    const rsrc_t ry = make_rsrc(a.up_y + (size_t)b * (C / 2) * To, (unsigned)(C / 2) * chby);
    // column T is the last workgroup's alone: in the one before it, it can lie on the grid too,
    // but past the valid columns
    const bool last_wg = blockIdx.x == gridDim.x - 1;
    float umax = 0.f;
#pragma unroll
    for (int m = 0; m < TM; ++m) {
      float bv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) bv[r] = bu[mrow0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half];
#pragma unroll
      for (int n = 0; n < TN; ++n) {
        const int col = xcol0 + n * 32;
        const int mm = tx0 + col;
        const bool keep = col >= LEAD && mm <= T && (col < LEAD + P::RP_BN || (mm == T && last_wg));
        const int ts = 2 * mm - 1;  // registers r, r + 1 (r even): samples ts, ts + 1 of channel rho / 2
        const unsigned vl = (unsigned)(2 * half) * chby + (unsigned)ts * 4u;
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          const unsigned so = (unsigned)((mrow0 + m * 32) / 2 + ((r & 3) >> 1) + 4 * (r >> 2)) * chby;
          const float v0 = acc[m][n][r] * sc2 + bv[r];
          const float v1 = acc[m][n][r + 1] * sc2 + bv[r + 1];
          if (keep && ts >= 0 && ts + 1 < To) {
            umax = fmaxf(umax, fmaxf(fabsf(v0), fabsf(v1)));
            const f32x2 v = {v0, v1};
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_t, v), ry, (int)vl, (int)so, TTS_ST_POL);
          } else {
            // the pair straddles the plane's start (mm = 0) or end (mm = T)
            const bool k0 = keep && ts >= 0, k1 = keep && ts + 1 < To;
            if (k0) umax = fmaxf(umax, fabsf(v0));
            if (k1) umax = fmaxf(umax, fabsf(v1));
            bstore(ry, v0, k0 ? vl : OOB_OFF, so);
            bstore(ry, v1, k1 ? vl + 4u : OOB_OFF, so);
          }
        }
      }
    }
    if (a.up_amax) publish_amax(a.up_amax, b, umax);
  };

  if constexpr (NCV == 6) {
    // one ResBlock1 iteration; LAST 0: the last one is told at run time (one loop body), 1 / 2:
    // known not to be / to be the last
    auto iteration = [&](int it, auto last_tag) __attribute__((always_inline)) {
      constexpr int LAST = decltype(last_tag)::value;
      const int d = a.dil[it];
      // ---- convs1[it] on lrelu(x) (X rows = column + XO): taps at column + (k - HK) * d
      conv(2 * it, XO - HK * d, d);
      lo = max(lo + HK * d, 0);  // outputs exist on the grid [0, RP_W) only
      hi = min(hi - HK * d, RP_W);
      {
        const float sc = H3 ? ldexpf(1.f, ex + a.w_exp[2 * it]) : 1.f;
        const float* bs = bsm + (2 * it) * C;
        float vmax = 0.f;
#pragma unroll
        for (int m = 0; m < TM; ++m) {
          float bv[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) bv[r] = bs[mrow0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half];
#pragma unroll
          for (int n = 0; n < TN; ++n) {
            const int col = xcol0 + n * 32;
            const int t = tx0 + col;
            const bool ok = col >= lo && col < hi && t >= 0 && t < T;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              float v = lrelu2(acc[m][n][r] * sc + bv[r], 0.1f);
              v = ok ? v : 0.f;
              acc[m][n][r] = v;
              vmax = fmaxf(vmax, fabsf(v));
            }
          }
        }
        const int et = tile_exp(vmax);
        if (!H3) __syncthreads();  // every wave done reading X
        store_pieces(HK, H3 ? ldexpf(1.f, -et) : 1.f);  // xt rows = column + HK
        __syncthreads();
        ex = et;
      }
      // ---- convs2[it] on xt: taps at column + k - HK = xt rows column + k
      conv(2 * it + 1, 0, 1);
      lo += HK;
      hi -= HK;
      if (LAST == 1 || (LAST == 0 && it < 2)) residual_to_lds(2 * it + 1);
      else if constexpr (UP) final_up(2 * it + 1);
      else final_to_z(2 * it + 1);
    };
    if constexpr (P::W64 || UP) {
      // the 256-register form peels the last iteration: with the z epilogue inside the loop body
      // the compiler carries the residual x in two register sets and spills one block of it
#pragma unroll 1
      for (int it = 0; it < 2; ++it) iteration(it, std::integral_constant<int, 1>{});
      iteration(2, std::integral_constant<int, 2>{});
    } else {
#pragma unroll 1
      for (int it = 0; it < 3; ++it) iteration(it, std::integral_constant<int, 0>{});
    }
  } else {
#pragma unroll 1
    for (int it = 0; it < 2; ++it) {
      const int d = a.dil[it];
      // ---- convs[it] on lrelu(x) (X rows = column + XO): taps at column + (k - HK) * d
      conv(it, XO - HK * d, d);
      lo = max(lo + HK * d, 0);
      hi = min(hi - HK * d, RP_W);
      if (it == 0) residual_to_lds(0);
      else final_to_z(1);
    }
  }
}

}  // namespace tts

namespace tts {
// ResBlock2 launchers (one translation unit per split scheme: kernels_resblock2_{h3,b1,x6}.hip).
// Geometry: C = 32 256 columns, C = 64 128 columns (geo64 = 1: 192), C = 128 128 columns as 8
// waves (kernels 3 and 5 only: 7 and 11 take Winograd F(4,4) per conv at >= 128 channels).
// the launch of one whole-block instance, with its bf16-plane form when ResBlock3Args::planes asks
template <class S, int C, int GEO, int K, int NCV, int XO, int LEAD>
void launch_block_pl(const ResBlock3Args& a, dim3 grid, int nt, hipStream_t s) {
  if (a.planes != 0) {
    constexpr bool OK = std::is_same<S, SchemeB1>::value;
    TTS_REQUIRE(OK && a.planes == (kPlaneXB16 | kPlaneYB16), 3, "resblock block: bf16 planes need the bf16 scheme");
    if constexpr (OK)
      hipLaunchKernelGGL((resblock3_kernel<S, C, GEO, K, NCV, XO, LEAD, kPlaneXB16 | kPlaneYB16>), grid, dim3(nt), 0, s, a);
    return;
  }
  hipLaunchKernelGGL((resblock3_kernel<S, C, GEO, K, NCV, XO, LEAD>), grid, dim3(nt), 0, s, a);
}
template <class S, int C, int GEO, int K>
void launch_rb2_t(const ResBlock3Args& a, int B, hipStream_t s) {
  constexpr int H = rb2_halo(K);
  using P = Res3Cfg<S, C, GEO, K, 2, H, H>;
  dim3 grid(ceil_div(a.T, P::RP_BN), 1, B);
  launch_block_pl<S, C, GEO, K, 2, H, H>(a, grid, P::NT, s);
}
template <class S, int C, int GEO>
void launch_rb2_k(const ResBlock3Args& a, int B, int K, hipStream_t s) {
  if (K == 3) launch_rb2_t<S, C, GEO, 3>(a, B, s);
  else if (K == 5) launch_rb2_t<S, C, GEO, 5>(a, B, s);
  else if (K == 7) launch_rb2_t<S, C, GEO, 7>(a, B, s);
  else launch_rb2_t<S, C, GEO, 11>(a, B, s);
}
template <class S>
void launch_rb2_s(const ResBlock3Args& a, int B, int C, int K, int geo64, hipStream_t s) {
  if (C == 32) launch_rb2_k<S, 32, 0>(a, B, K, s);
  else if (C == 64) {
    if (geo64 == 1) launch_rb2_k<S, 64, 1>(a, B, K, s);
    else launch_rb2_k<S, 64, 2>(a, B, K, s);
  } else {
    if constexpr (S::ROWB <= 80) {
      if (K == 3) launch_rb2_t<S, 128, 3, 3>(a, B, s);
      else launch_rb2_t<S, 128, 3, 5>(a, B, s);
    } else {
      throw Error(3, "resblock2: 128 channels need a split scheme of at most 80-byte rows");
    }
  }
}
void launch_resblock2_h3(const ResBlock3Args& a, int B, int C, int K, int geo64, hipStream_t s);
void launch_resblock2_b1(const ResBlock3Args& a, int B, int C, int K, int geo64, hipStream_t s);
void launch_resblock2_x6(const ResBlock3Args& a, int B, int C, int K, int geo64, hipStream_t s);
}  // namespace tts
