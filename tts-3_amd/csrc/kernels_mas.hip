// Glow-TTS alignment on the device (gfx950): the text-to-mel log-likelihood matrix and Monotonic
// Alignment Search (GlowTTS.forward / inference_with_MAS, TTS/tts/models/glow_tts.py:193-316;
// maximum_path, TTS/tts/utils/helpers.py).
//
// mas_logp_kernel: logp[b][x][y] = sum_c(-0.5 log(2 pi) - ls[c][x]) + sum_c s[c][x] (-0.5 z[c][y]^2)
//   + sum_c (m[c][x] s[c][x]) z[c][y] + sum_c -0.5 m[c][x]^2 s[c][x],  s = exp(-2 ls)
// as one GEMM per item on v_mfma_f32_32x32x2_f32 with depth 2C: k-step c multiplies the A pair
// (s[c][x], m[c][x] s[c][x]) by the B pair (-0.5 z[c][y]^2, z[c][y]).  A lane of half h supplies
// element h of both pairs, built from three coalesced loads (no LDS: consecutive lanes read
// consecutive x / y of one channel row).  The two row constants are summed by the lane of row x on
// the way and added in the epilogue.  One arithmetic, fp32 throughout.
//
// mas_kernel: one workgroup per item; wave 0 runs the recurrence, all four waves fetch.  Lane l keeps V[x][y-1] of its XPT consecutive tokens x = l XPT + j
// in registers; column y needs V[x-1][y-1] of the lane below only for j = 0 (one DPP wave shift per
// column), so a column is XPT (max, add, compare) triples with no barrier inside a block of columns.
// Values are staged through LDS in blocks of CB columns with coalesced loads (a row segment of CB
// floats per group of lanes; the loads of the next four blocks are in flight in registers while a
// block is consumed, one barrier per block), never one strided 4-byte load per row per column.  V is not kept: the backtrack decision (x == y) || V[x][y-1] < V[x-1][y-1]
// is one bit per cell, collected per lane into a word per (token, 32-column chunk) and stored chunk
// by chunk ([chunk][token] words) in LDS, or in the workspace when an item's bits exceed
// MAS_BITS_LDS.  The backtrack walks the words with count-leading-zeros: one LDS read per token and
// per chunk, not one per frame (workspace mode: a chunk's words are staged into LDS with one coalesced
// read first).  It records the first frame of every token; durations are the differences, and the
// path is filled from those starts by a second, grid-wide kernel.
//
// Every cell is max(v_cur, v_prev) + value in fp32 as in the reference's loops, so the path equals a
// CPU evaluation of those loops exactly.  Items with t_x < 1, t_y < t_x, t_x > T_en or t_y > T_de (the
// reference reads out of bounds there) get an all-zero path and zero durations.
// Limits: T_en <= 1024 (MAS_MAX_TEN), value plane T_en T_de 4 bytes < 2 GiB, B <= 65535.
#include <algorithm>

#include "conv_device.hpp"
#include "mas.hpp"

namespace tts {

namespace {
constexpr float kMasNeg = -1e9f;
constexpr float kHalfLog2Pi = 0.91893853320467274178f;

// orders the wave's own LDS / global traffic (single-wave workgroup: no s_barrier needed)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// the value of lane l - 1 (lane 0: its own): DPP wave_shr:1, a VALU move with no LDS round trip
__device__ __forceinline__ float lane_below(float v) {
  const int i = __builtin_bit_cast(int, v);
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, 0x138, 0xF, 0xF, false));
}
}  // namespace

struct MasLogpArgs {
  const float* o_mean;
  const float* o_log_scale;  // NULL: zeros
  const float* z;
  float* logp;
  int C, T_en, T_de;
};

template <int TN>
__global__ __launch_bounds__(256) void mas_logp_kernel(MasLogpArgs a) {
  const int lane = threadIdx.x & 63;
  const int half = lane >> 5, l32 = lane & 31;
  const int b = blockIdx.z;
  const int x0 = (blockIdx.y * 4 + wave_id()) * 32;
  if (x0 >= a.T_en) return;  // wave-uniform; the kernel has no barrier
  const int y0 = blockIdx.x * (32 * TN);
  const int C = a.C, T_en = a.T_en, T_de = a.T_de;
  const bool has_ls = a.o_log_scale != nullptr;
  const size_t xo = (size_t)b * C * T_en, zo = (size_t)b * C * T_de;
  const rsrc_t rm = make_rsrc(a.o_mean + xo, (unsigned)C * (unsigned)T_en * 4u);
  const rsrc_t rl = make_rsrc(has_ls ? a.o_log_scale + xo : a.o_mean + xo, (unsigned)C * (unsigned)T_en * 4u);
  const rsrc_t rz = make_rsrc(a.z + zo, (unsigned)C * (unsigned)T_de * 4u);
  const int x = x0 + l32;
  const bool okx = x < T_en;
  const unsigned vx = okx ? (unsigned)x * 4u : OOB_OFF;
  unsigned vy[TN];
#pragma unroll
  for (int n = 0; n < TN; ++n) {
    const int y = y0 + n * 32 + l32;
    vy[n] = y < T_de ? (unsigned)y * 4u : OOB_OFF;
  }
  f32x16 acc[TN];
#pragma unroll
  for (int n = 0; n < TN; ++n) acc[n] = f32x16{};
  float c1 = 0.f, c4 = 0.f;  // row constants of token x (both halves hold the same)

  auto step = [&](float m, float ls, const float (&zv)[TN]) {
    const float sc = has_ls ? expf(-2.f * ls) : 1.f;
    const float ms = m * sc;
    c1 += -kHalfLog2Pi - ls;
    c4 += -0.5f * (m * m) * sc;
    // tails are zero-padded: a token row past T_en contributes nothing
    const float av = okx ? (half ? ms : sc) : 0.f;
#pragma unroll
    for (int n = 0; n < TN; ++n) {
      const float bv = half ? zv[n] : -0.5f * (zv[n] * zv[n]);
      acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[n], 0, 0, 0);
    }
  };

  constexpr int U = 4;  // channels whose loads are issued together
  int c = 0;
  for (; c + U <= C; c += U) {
    float m[U], ls[U], zv[U][TN];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      m[u] = bload(rm, vx, (unsigned)(c + u) * (unsigned)T_en * 4u);
      ls[u] = has_ls ? bload(rl, vx, (unsigned)(c + u) * (unsigned)T_en * 4u) : 0.f;
#pragma unroll
      for (int n = 0; n < TN; ++n) zv[u][n] = bload(rz, vy[n], (unsigned)(c + u) * (unsigned)T_de * 4u);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) step(m[u], ls[u], zv[u]);
  }
  for (; c < C; ++c) {
    float zv[TN];
    const float m = bload(rm, vx, (unsigned)c * (unsigned)T_en * 4u);
    const float ls = has_ls ? bload(rl, vx, (unsigned)c * (unsigned)T_en * 4u) : 0.f;
#pragma unroll
    for (int n = 0; n < TN; ++n) zv[n] = bload(rz, vy[n], (unsigned)c * (unsigned)T_de * 4u);
    step(m, ls, zv);
  }

  // epilogue: lane holds column l32 and rows (r & 3) + 8 (r >> 2) + 4 half of each 32x32 block
  const rsrc_t ry = make_rsrc(a.logp + (size_t)b * T_en * T_de, (unsigned)T_en * (unsigned)T_de * 4u);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
    const float k1 = __shfl(c1, row, 64), k4 = __shfl(c4, row, 64);
    const int xr = x0 + row;
#pragma unroll
    for (int n = 0; n < TN; ++n) {
      const int y = y0 + n * 32 + l32;
      const bool ok = xr < T_en && y < T_de;
      bstore(ry, (acc[n][r] + k4) + k1, ok ? ((unsigned)xr * (unsigned)T_de + (unsigned)y) * 4u : OOB_OFF, 0u);
    }
  }
}

void launch_mas_logp(const float* o_mean, const float* o_log_scale, const float* z, int B, int C, int T_en, int T_de,
                     float* logp, hipStream_t s) {
  TTS_REQUIRE(B <= 65535, 3, "glow_mas_logp: more than 65535 items");
  TTS_REQUIRE((int64_t)C * T_en * 4 < (int64_t)1 << 31 && (int64_t)C * T_de * 4 < (int64_t)1 << 31 &&
                  (int64_t)T_en * T_de * 4 < (int64_t)1 << 31,
              3, "glow_mas_logp: a per-item plane of 2 GiB or more");
  MasLogpArgs a{o_mean, o_log_scale, z, logp, C, T_en, T_de};
  constexpr int TN = 2;
  const dim3 grid(ceil_div(T_de, 32 * TN), ceil_div(T_en, 128), B);
  TTS_REQUIRE(grid.y <= 65535, 3, "glow_mas_logp: too many tokens");
  hipLaunchKernelGGL(mas_logp_kernel<TN>, grid, dim3(256), 0, s, a);
  TTS_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------
struct MasArgs {
  const float* value;   // [B][T_en][T_de]
  const float* mask;    // [B][T_en][T_de] or NULL
  const int64_t* t_x;   // [B]
  const int64_t* t_y;   // [B]
  int T_en, T_de;
  int nchunk;           // ceil(T_de / 32)
  unsigned* bits_ws;    // [B][nchunk][64 XPT] decision words, or NULL: they live in LDS
  int* starts;          // [B][T_en + 1] first frame of every token (starts[T_en] = t_y), or NULL
  float* dur;           // [B][T_en] or NULL
  float* log_dur;       // [B][T_en] or NULL
};

template <int XPT>
struct MasGeo {
  static constexpr int TP = 64 * XPT;                    // token rows, padded
  static constexpr int CB = XPT <= 2 ? 32 : 64 / XPT;    // columns per staged block (divides 32)
  static constexpr int R = (TP * CB) / 64;               // staged values per block / 64
  static constexpr int P = TP + 4;                       // LDS pitch of a staged column (floats)
  static constexpr int STAGE = 2 * CB * P;               // two blocks
  static constexpr int START = TP + 4;                   // start[TP + 1], padded
  static constexpr size_t lds_bytes(size_t bits_words) { return (size_t)(STAGE + START + TP + bits_words) * 4; }
};

template <int XPT, bool MASK>
__global__ __launch_bounds__(256) void mas_kernel(MasArgs a) {
  using G = MasGeo<XPT>;
  constexpr int TP = G::TP, CB = G::CB, P = G::P;
  constexpr int R4 = G::R / 4;  // staged values per thread and block
  constexpr int D = 4;          // blocks whose loads are in flight
  extern __shared__ __attribute__((aligned(16))) unsigned char mas_smem[];
  float* stage = reinterpret_cast<float*>(mas_smem);           // [2][CB][P]
  int* start = reinterpret_cast<int*>(stage + G::STAGE);       // [TP + 1]
  unsigned* bstage = reinterpret_cast<unsigned*>(start + G::START);  // [TP]: a chunk from the workspace
  unsigned* bits_lds = bstage + TP;                            // [nchunk][TP]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = wave_id();
  const int b = blockIdx.x;
  const int T_en = a.T_en, T_de = a.T_de;
  const int64_t tx64 = a.t_x[b], ty64 = a.t_y[b];
  const bool valid = tx64 >= 1 && ty64 >= tx64 && tx64 <= T_en && ty64 <= T_de;
  float* dur = a.dur ? a.dur + (size_t)b * T_en : nullptr;
  float* ldur = a.log_dur ? a.log_dur + (size_t)b * T_en : nullptr;
  int* gstart = a.starts ? a.starts + (size_t)b * (T_en + 1) : nullptr;
  if (!valid) {  // uniform: all-zero path and durations
    for (int x = tid; x <= T_en; x += 256) {
      if (gstart) gstart[x] = 0;
      if (x < T_en) {
        if (dur) dur[x] = 0.f;
        if (ldur) ldur[x] = 0.f;
      }
    }
    return;
  }
  const int tx = (int)tx64, ty = (int)ty64;
  const bool in_lds = a.bits_ws == nullptr;
  unsigned* bits = in_lds ? bits_lds : a.bits_ws + (size_t)b * a.nchunk * TP;

  const size_t plane = (size_t)b * T_en * T_de;
  const rsrc_t rv = make_rsrc(a.value + plane, (unsigned)T_en * (unsigned)T_de * 4u);
  const rsrc_t rk = make_rsrc((MASK ? a.mask : a.value) + plane, (unsigned)T_en * (unsigned)T_de * 4u);

  // block blk = columns [blk CB, blk CB + CB): element e = i 256 + tid is (row e / CB, column e % CB).
  // Only cells of [0, t_x) x [0, t_y) are read: no other cell reaches the path.
  auto load_block = [&](int blk, float (&pre)[R4]) {
#pragma unroll
    for (int i = 0; i < R4; ++i) {
      const int e = i * 256 + tid;
      const int r = e / CB, y = blk * CB + (e % CB);
      const unsigned off = (r < tx && y < ty) ? ((unsigned)r * (unsigned)T_de + (unsigned)y) * 4u : OOB_OFF;
      float v = bload(rv, off, 0u);
      if (MASK) v = v * bload(rk, off, 0u);  // the reference's value * mask
      pre[i] = v;
    }
  };
  auto store_block = [&](int buf, const float (&pre)[R4]) {
    float* sb = stage + buf * (CB * P);
#pragma unroll
    for (int i = 0; i < R4; ++i) {
      const int e = i * 256 + tid;
      sb[(e % CB) * P + e / CB] = pre[i];
    }
  };

  for (int x = tid; x <= TP; x += 256) start[x] = x == 0 ? 0 : ty;  // tokens >= t_x: empty at t_y

  // Block k waits in register set k % D until the iteration before its turn stores it to LDS.
  const int nblk = (ty + CB - 1) / CB;
  const int xb = lane * XPT;
  float pre[D][R4];
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (d < nblk) load_block(d, pre[d]);
  store_block(0, pre[0]);
  __syncthreads();
  float V[XPT];
  unsigned dw[XPT];
#pragma unroll
  for (int j = 0; j < XPT; ++j) {
    V[j] = 0.f;
    dw[j] = 0u;
  }
  // wave 0 runs the recurrence of block blk out of LDS while all four waves fetch
  auto consume = [&](int blk) {
    const bool more = blk + 1 < nblk;
    const float* sb = stage + (blk & 1) * (CB * P);
    const int ncol = min(CB, ty - blk * CB);
    auto column = [&](int c) {
      const int y = blk * CB + c;
      float val[XPT];
#pragma unroll
      for (int j = 0; j < XPT; ++j) val[j] = sb[c * P + xb + j];
      const float up = lane_below(V[XPT - 1]);
      const float p0 = lane == 0 ? (y == 0 ? 0.f : kMasNeg) : up;
      const unsigned bit = 1u << (y & 31);
#pragma unroll
      for (int j = XPT - 1; j >= 0; --j) {  // descending: V[j - 1] is still column y - 1's
        const int x = xb + j;
        const float vprev = j > 0 ? V[j - 1] : p0;
        const bool diag = x == y;
        const float vcur = diag ? kMasNeg : V[j];
        if (diag || V[j] < vprev) dw[j] |= bit;
        V[j] = fmaxf(vcur, vprev) + val[j];
      }
    };
    if (ncol == CB) {  // constant trip count: the LDS reads of the next columns move ahead of the chain
#pragma unroll
      for (int c = 0; c < CB; ++c) column(c);
    } else {
      for (int c = 0; c < ncol; ++c) column(c);
    }
    if ((((blk + 1) * CB) & 31) == 0 || !more) {  // a 32-column chunk is complete
      unsigned* cp = bits + (size_t)((blk * CB) >> 5) * TP + xb;
#pragma unroll
      for (int j = 0; j < XPT; ++j) {
        cp[j] = dw[j];
        dw[j] = 0u;
      }
    }
  };
  for (int blk0 = 0; blk0 < nblk; blk0 += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int blk = blk0 + d;
      if (blk < nblk) {  // uniform over the workgroup
        if (blk + D < nblk) load_block(blk + D, pre[d]);  // set d held block blk, in LDS since the last iteration
        if (wave == 0) consume(blk);
        if (blk + 1 < nblk) store_block((blk + 1) & 1, pre[(d + 1) % D]);
        __syncthreads();
      }
    }
  }
  if (wave != 0) return;  // the backtrack is one wave's work: wave-level ordering from here on
  if (!in_lds) __threadfence();

  // ---- backtrack, the same walk in every lane (uniform addresses; lane 0 records the starts).
  // In chunk ch token `index` switches to index - 1 at the highest set bit at or below the current
  // frame; that frame is the token's first.
  int index = tx - 1;
  for (int ch = (ty - 1) >> 5; ch >= 0 && index > 0; --ch) {
    const unsigned* cp;
    if (in_lds) {
      cp = bits + (size_t)ch * TP;
    } else {
      wave_sync();  // the previous chunk's reads are done
      const unsigned* g = bits + (size_t)ch * TP;
      for (int x = lane; x < TP; x += 64) bstage[x] = __hip_atomic_load(g + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      wave_sync();
      cp = bstage;
    }
    int yb = min(31, ty - 1 - ch * 32);
    unsigned w = cp[index];
    while (true) {
      const unsigned m = w & (0xFFFFFFFFu >> (31 - yb));
      if (!m) break;
      const int p = 31 - __clz((int)m);
      if (lane == 0) start[index] = ch * 32 + p;
      --index;
      if (index == 0 || p == 0) break;
      yb = p - 1;
      w = cp[index];
    }
  }
  wave_sync();
  for (int x = lane; x <= T_en; x += 64) {
    const int s0 = start[x];
    if (gstart) gstart[x] = s0;
    if (x < T_en) {
      const float d = (float)(start[x + 1] - s0);
      if (dur) dur[x] = d;
      if (ldur) ldur[x] = logf(1.f + d);
    }
  }
}

// path[b][x][y] = 1 for starts[b][x] <= y < starts[b][x + 1], else 0
__global__ __launch_bounds__(256) void mas_fill_kernel(const int* __restrict__ starts, float* __restrict__ path, int T_en,
                                                       int T_de) {
  const int b = blockIdx.z, x = blockIdx.y;
  const int s0 = starts[(size_t)b * (T_en + 1) + x], s1 = starts[(size_t)b * (T_en + 1) + x + 1];
  float* row = path + ((size_t)b * T_en + x) * T_de;
  for (int64_t y = (int64_t)blockIdx.x * 256 + threadIdx.x; y < T_de; y += (int64_t)gridDim.x * 256)
    row[y] = (y >= s0 && y < s1) ? 1.f : 0.f;
}

namespace {
template <int XPT>
void launch_mas_x(const MasArgs& a, int B, hipStream_t s) {
  const size_t lds = MasGeo<XPT>::lds_bytes(a.bits_ws ? 0 : (size_t)a.nchunk * MasGeo<XPT>::TP);
  TTS_REQUIRE(lds <= (size_t)160 * 1024, 1, "maximum_path: bad launch geometry");
  auto go = [&](auto kernel) {
    // above the default dynamic LDS limit: opt in (per function; cheap and idempotent)
    TTS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      160 * 1024));
    hipLaunchKernelGGL(kernel, dim3(B), dim3(256), lds, s, a);
  };
  if (a.mask) go(mas_kernel<XPT, true>);
  else go(mas_kernel<XPT, false>);
}
}  // namespace

void launch_maximum_path(const float* value, const float* mask, const int64_t* t_x, const int64_t* t_y, int B, int T_en,
                         int T_de, void* workspace, float* path, float* durations, float* log_dur, hipStream_t s) {
  TTS_REQUIRE(T_en <= MAS_MAX_TEN, 3, "maximum_path: more than " + std::to_string(MAS_MAX_TEN) + " tokens");
  TTS_REQUIRE((int64_t)T_en * T_de * 4 < (int64_t)1 << 31, 3, "maximum_path: a value plane of 2 GiB or more");
  TTS_REQUIRE(B <= 65535, 3, "maximum_path: more than 65535 items");
  MasArgs a{};
  a.value = value; a.mask = mask; a.t_x = t_x; a.t_y = t_y; a.T_en = T_en; a.T_de = T_de;
  a.nchunk = (T_de + 31) / 32;
  a.starts = static_cast<int*>(workspace);
  a.bits_ws = mas_bits_in_lds(T_en, T_de)
                  ? nullptr
                  : reinterpret_cast<unsigned*>(static_cast<unsigned char*>(workspace) + mas_starts_bytes(B, T_en));
  a.dur = durations; a.log_dur = log_dur;
  switch (mas_xpt(T_en)) {
    case 1: launch_mas_x<1>(a, B, s); break;
    case 2: launch_mas_x<2>(a, B, s); break;
    case 4: launch_mas_x<4>(a, B, s); break;
    case 8: launch_mas_x<8>(a, B, s); break;
    default: launch_mas_x<16>(a, B, s); break;
  }
  TTS_HIP_CHECK(hipGetLastError());
  if (path) {
    const unsigned gx = (unsigned)std::min<int64_t>(((int64_t)T_de + 1023) / 1024, 65535);
    hipLaunchKernelGGL(mas_fill_kernel, dim3(gx, T_en, B), dim3(256), 0, s, a.starts, path, T_en, T_de);
    TTS_HIP_CHECK(hipGetLastError());
  }
}

}  // namespace tts
