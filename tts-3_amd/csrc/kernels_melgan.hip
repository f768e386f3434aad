// MelGAN-family kernels (gfx950): the whole residual block, the tail (conv + tanh + PQMF synthesis),
// the input gather and the stand-alone PQMF synthesis.  Layouts and packing: melgan.hpp.
//
// Residual block (TTS/vocoder/layers/melgan.py ResidualStack), one launch:
//   out = Ws x + bs + W2 lrelu(W1 (*)_d reflpad(lrelu(x)) + b1) + b2
// as two GEMMs on the matrix cores with the split-precision operand schemes of split_device.hpp
// (rows = output channels, columns = time, depth = input channels x taps).  A workgroup of 4 waves
// owns kMelganBlockTile = 64 columns and every channel: wave w takes column block w & 1 and the row
// blocks (w >> 1) + 2 i.  The weights stream from L2 as ready fragments; the activations pass through
// LDS as rows of [piece][16 channels] (pitch S::ROWB), split while staging:
//   1. per 32-channel chunk: lrelu(x) for the tile's columns and d halo columns per side, the
//      reflection at the utterance ends resolved in the staging index map; GEMM 1 (depth 3 C)
//      accumulates in registers over the chunks
//   2. h = lrelu(acc + b1) goes to LDS split, for every channel
//   3. GEMM 2 (depth 2 C) over [h ; x] with [W2 | Ws]: first the h rows from LDS, then x staged raw
//      per 32-channel chunk; out = acc + (b2 + bs)
// x is read from HBM / L2 twice (activated with the halo, raw without), the output written once; h
// never leaves the workgroup.  Per output the steps and products run in one fixed order, so results do
// not depend on the batch size.
#include <algorithm>

#include "melgan.hpp"
#include "split_device.hpp"

namespace tts {

namespace {
constexpr int W = kMelganBlockTile;
constexpr int CG = 2;  // 16-channel groups per staged chunk
constexpr float kSlope = 0.2f;
}  // namespace

template <class S, int NI>
__global__ __launch_bounds__(256) void melgan_block_kernel(MelganBlockArgs a) {
  constexpr int NP = S::NP;
  constexpr int ROWB = S::ROWB;
  extern __shared__ __attribute__((aligned(16))) unsigned char melgan_smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = wave_id();
  const int half = lane >> 5;
  const int l32 = lane & 31;
  const int cb = wave & 1, rh = wave >> 1;
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * W;
  const int C = a.C, L = a.L, d = a.dil;
  const int G = (C + 15) >> 4, MB = (C + 31) >> 5;
  const int XR = W + 2 * d;  // staged rows of GEMM 1
  const int nch = (G + CG - 1) / CG;

  unsigned char* xbuf = melgan_smem;                  // [CG][XR][ROWB]
  unsigned char* hbuf = melgan_smem + CG * XR * ROWB;  // [G][W][ROWB]

  const rsrc_t rx = make_rsrc(a.x + (size_t)b * C * L, (unsigned)C * (unsigned)L * 4u);
  const rsrc_t ra1 = make_rsrc(a.a1, a.a1_bytes);
  const rsrc_t ra2 = make_rsrc(a.a2, a.a2_bytes);
  const unsigned avoff = (unsigned)lane * 16u;

  // rows [tfirst, tfirst + nrows) of channels [32 c, 32 c + 32) -> xbuf[gl][r], split
  auto stage = [&](int c, bool act, int nrows, int tfirst) {
    const int units = CG * 4 * nrows;
    for (int u = tid; u < units; u += 256) {
      const int q = u / nrows, r = u - q * nrows;
      int i = tfirst + r;
      i = i < 0 ? -i : i;                // left reflection (d < L)
      i = i >= L ? 2 * (L - 1) - i : i;  // right reflection; i < 0 now: past the padded plane
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ch = 32 * c + 4 * q + j;
        const float xv = bload(rx, (i >= 0 && ch < C) ? ((unsigned)ch * (unsigned)L + (unsigned)i) * 4u : OOB_OFF, 0u);
        v[j] = act ? lrelu2(xv, kSlope) : xv;
      }
      split_store4<S>(xbuf + ((q >> 2) * nrows + r) * ROWB + (q & 3) * 8, v[0], v[1], v[2], v[3]);
    }
  };

  int mb[NI];
  bool mbv[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    mb[i] = rh + 2 * i;
    mbv[i] = mb[i] < MB;
  }
  f32x16 acc[NI];
  f32x4 af[2][NI][NP];  // A fragments: this step's and the next's
  // A fragments of step s (steps per row block: nsteps); past the packed array the range check gives 0
  auto load_a = [&](f32x4 (&dst)[NI][NP], const rsrc_t& ra, int nsteps, int s) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int p = 0; p < NP; ++p)
        dst[i][p] = bload4(ra, mbv[i] ? avoff : OOB_OFF, (unsigned)((mb[i] * nsteps + s) * NP + p) * 1024u);
  };
  auto mma = [&](const f32x4 (&A)[NI][NP], const unsigned char* brow) {
    f32x4 bf[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) bf[p] = *reinterpret_cast<const f32x4*>(brow + 32 * p);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      if (mbv[i]) {
#pragma unroll
        for (int e = 0; e < S::NPROD; ++e) acc[i] = S::mfma(A[i][S::PA[e]], bf[S::PB[e]], acc[i]);
      }
    }
  };
  const int col = cb * 32 + l32;

  // ---- GEMM 1: h_pre = W1 (*)_d reflpad(lrelu(x)) ----
#pragma unroll
  for (int i = 0; i < NI; ++i) acc[i] = f32x16{};
  const int S1 = 3 * G;
  for (int c = 0; c < nch; ++c) {
    if (c > 0) __syncthreads();  // every wave is done with the previous chunk
    stage(c, true, XR, t0 - d);
    __syncthreads();
    const int ng = min(CG, G - CG * c);
    const int ns = 3 * ng;  // steps of this chunk: (group gl, tap k) = (j / 3, j % 3)
    load_a(af[0], ra1, S1, 3 * CG * c);
    for (int j = 0; j < ns; j += 2) {
      // two steps per iteration: the fragment ring returns to its start (no moves)
      load_a(af[1], ra1, S1, 3 * CG * c + j + 1);
      {
        const int gl = j / 3, k = j - 3 * gl;
        mma(af[0], xbuf + (gl * XR + col + k * d) * ROWB + 16 * half);
      }
      if (j + 1 < ns) {
        load_a(af[0], ra1, S1, 3 * CG * c + j + 2);
        const int gl = (j + 1) / 3, k = j + 1 - 3 * gl;
        mma(af[1], xbuf + (gl * XR + col + k * d) * ROWB + 16 * half);
      }
    }
  }

  // ---- h = lrelu(h_pre + b1) -> hbuf (registers 4 jj .. + 3 of a lane: 4 consecutive channels) ----
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    if (mbv[i]) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int g = mb[i] * 2 + (jj >> 1);
        if (g < G) {
          const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias1 + mb[i] * 32 + 8 * jj + 4 * half);
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = lrelu2(acc[i][4 * jj + r] + bv[r], kSlope);
          split_store4<S>(hbuf + (g * W + col) * ROWB + 16 * (jj & 1) + 8 * half, v[0], v[1], v[2], v[3]);
        }
      }
    }
  }
  __syncthreads();  // h complete; every wave is done with GEMM 1's last chunk

  // ---- GEMM 2: [W2 | Ws] [h ; x] ----
#pragma unroll
  for (int i = 0; i < NI; ++i) acc[i] = f32x16{};
  const int S2 = 2 * G;
  stage(0, false, W, t0);  // raw x, chunk 0: xbuf is free, the h steps below read hbuf only
  load_a(af[0], ra2, S2, 0);
  for (int j = 0; j < G; j += 2) {
    load_a(af[1], ra2, S2, j + 1);
    mma(af[0], hbuf + (j * W + col) * ROWB + 16 * half);
    if (j + 1 < G) {
      load_a(af[0], ra2, S2, j + 2);
      mma(af[1], hbuf + ((j + 1) * W + col) * ROWB + 16 * half);
    }
  }
  for (int c = 0; c < nch; ++c) {
    if (c > 0) {
      __syncthreads();
      stage(c, false, W, t0);
    }
    __syncthreads();
    const int ng = min(CG, G - CG * c);
    load_a(af[0], ra2, S2, G + CG * c);
    for (int j = 0; j < ng; j += 2) {
      load_a(af[1], ra2, S2, G + CG * c + j + 1);
      mma(af[0], xbuf + (j * W + col) * ROWB + 16 * half);
      if (j + 1 < ng) mma(af[1], xbuf + ((j + 1) * W + col) * ROWB + 16 * half);
    }
  }

  // ---- out = acc + (b2 + bs) ----
  const rsrc_t ry = make_rsrc(a.y + (size_t)b * C * L, (unsigned)C * (unsigned)L * 4u);
  const int t = t0 + col;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    if (mbv[i]) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mb[i] * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const float v = acc[i][r] + a.bias2[row];
        bstore(ry, v, (row < C && t < L) ? ((unsigned)row * (unsigned)L + (unsigned)t) * 4u : OOB_OFF, 0u);
      }
    }
  }
}

size_t melgan_block_lds(int mode, int C, int dil) {
  const int rowb = mode == MATH_BF16 ? SchemeB1::ROWB : SchemeX6::ROWB;
  return (size_t)(CG * (W + 2 * dil) + melgan_groups(C) * W) * rowb;
}

namespace {
template <class S>
void launch_block_s(const MelganBlockArgs& a, const dim3& grid, size_t lds, hipStream_t s) {
  auto go = [&](auto kernel) {
    TTS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      kMelganLdsLimit));
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, a);
  };
  switch ((melgan_mblocks(a.C) + 1) / 2) {
    case 1: go(melgan_block_kernel<S, 1>); break;
    case 2: go(melgan_block_kernel<S, 2>); break;
    case 3: go(melgan_block_kernel<S, 3>); break;
    default: go(melgan_block_kernel<S, 4>); break;
  }
}
}  // namespace

void launch_melgan_block(int mode, const MelganBlockArgs& a, int B, hipStream_t s) {
  TTS_REQUIRE(mode == MATH_FP32_X6 || mode == MATH_BF16, 3, "melgan block: math mode must be fp32x6 or bf16");
  TTS_REQUIRE(a.C >= 1 && a.C <= kMelganMaxC, 3, "melgan block: channels must lie in [1, 256]");
  TTS_REQUIRE(a.dil >= 1 && a.dil <= kMelganMaxDil, 3, "melgan block: dilation must lie in [1, 27]");
  TTS_REQUIRE(a.L > a.dil, 1, "melgan block: the reflection pad must be smaller than the plane it pads");
  TTS_REQUIRE((int64_t)a.C * a.L * 4 < (int64_t)1 << 31, 3, "melgan block: a batch item's plane exceeds 2 GiB");
  TTS_REQUIRE(B >= 1 && B <= 65535, 1, "melgan block: batch size must lie in [1, 65535]");
  TTS_REQUIRE(a.x != a.y, 1, "melgan block: the output must not alias the input");
  const size_t lds = melgan_block_lds(mode, a.C, a.dil);
  TTS_REQUIRE(lds <= (size_t)kMelganLdsLimit, 3, "melgan block: the tile does not fit the LDS");
  const dim3 grid((a.L + W - 1) / W, B);
  if (mode == MATH_BF16) launch_block_s<SchemeB1>(a, grid, lds, s);
  else launch_block_s<SchemeX6>(a, grid, lds, s);
  TTS_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------
// Input gather: replicate padding (inference) and the first conv's reflection padding
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void melgan_gather_kernel(const float* __restrict__ mel, int C, int T, int pad, int rp,
                                                            float* __restrict__ out) {
  const int L = T + 2 * pad, Lo = L + 2 * rp;
  const int64_t row = (int64_t)blockIdx.z * C + blockIdx.y;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < Lo; t += gridDim.x * 256) {
    int i = t - rp;
    i = i < 0 ? -i : i;
    i = i >= L ? 2 * (L - 1) - i : i;
    i = min(max(i - pad, 0), T - 1);
    out[row * Lo + t] = mel[row * T + i];
  }
}

void launch_melgan_gather(const float* mel, int B, int C, int T, int pad, int rp, float* out, hipStream_t s) {
  TTS_REQUIRE(C >= 1 && C <= 65535 && B >= 1 && B <= 65535, 1, "melgan: bad channel count or batch size");
  TTS_REQUIRE(rp < T + 2 * pad, 1, "melgan: the reflection pad must be smaller than the plane it pads");
  const int Lo = T + 2 * pad + 2 * rp;
  const int bx = std::min(1024, (Lo + 255) / 256);
  hipLaunchKernelGGL(melgan_gather_kernel, dim3(bx, C, B), dim3(256), 0, s, mel, C, T, pad, rp, out);
  TTS_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------
// Tail: lrelu(0.2) -> reflection pad (K - 1) / 2 -> conv K to CO channels -> tanh [-> PQMF synthesis]
// plain fp32 FMA.  A workgroup computes 256 columns of every output channel; with the PQMF, halo
// = ceil((taps / 2) / CO) of them per side are recomputed neighbours: the sub-bands stay in LDS.
// ---------------------------------------------------------------------------------------
constexpr int kTailMaxK = 11;
constexpr int kTailMaxTaps = 126;

// sum over the j with (n + j - taps/2) divisible by N: x(k, m) is sub-band k at index m (0 outside)
template <class F>
__device__ __forceinline__ float pqmf_sample(int n, int N, int taps, const float* g, F&& x) {
  const int h2 = taps >> 1;
  int j0 = (h2 - n) % N;
  j0 = j0 < 0 ? j0 + N : j0;
  float y = 0.f;
  for (int k = 0; k < N; ++k)
    for (int j = j0; j <= taps; j += N) y = fmaf(g[k * (taps + 1) + j], x(k, (n + j - h2) / N), y);
  return y * (float)N;
}

template <int CO>
__global__ __launch_bounds__(256) void melgan_tail_kernel(MelganTailArgs a) {
  constexpr int CH = 16;
  constexpr int XC = 256 + kTailMaxK - 1;
  __shared__ float xs[CH][XC];
  __shared__ float sb[CO][256];
  __shared__ float gl[CO * (kTailMaxTaps + 1)];
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int L = a.L, K = a.K, Cin = a.Cin, P = (K - 1) >> 1;
  const bool synth = a.g != nullptr;
  const int halo = synth ? ((a.taps >> 1) + CO - 1) / CO : 0;
  const int TW = 256 - 2 * halo;
  const int c0 = blockIdx.x * TW - halo;  // column of thread 0
  const int xc = 256 + K - 1;
  const float* xb = a.x + (size_t)b * Cin * L;
  if (synth)
    for (int i = tid; i < CO * (a.taps + 1); i += 256) gl[i] = a.g[i];

  float acc[CO];
#pragma unroll
  for (int co = 0; co < CO; ++co) acc[co] = 0.f;
  for (int ch0 = 0; ch0 < Cin; ch0 += CH) {
    const int nc = min(CH, Cin - ch0);
    if (ch0 > 0) __syncthreads();
    for (int u = tid; u < nc * xc; u += 256) {
      const int ch = u / xc, r = u - ch * xc;
      const int tt = c0 - P + r;
      int i = tt < 0 ? -tt : tt;
      i = i >= L ? 2 * (L - 1) - i : i;
      const bool ok = tt >= -P && tt < L + P;  // P < L: i lies in [0, L)
      xs[ch][r] = ok ? lrelu2(xb[(size_t)(ch0 + ch) * L + i], kSlope) : 0.f;
    }
    __syncthreads();
    for (int ch = 0; ch < nc; ++ch)
      for (int k = 0; k < K; ++k) {
        const float xv = xs[ch][tid + k];
#pragma unroll
        for (int co = 0; co < CO; ++co) acc[co] = fmaf(a.w[((size_t)co * Cin + ch0 + ch) * K + k], xv, acc[co]);
      }
  }
  const int c = c0 + tid;
  const bool valid = c >= 0 && c < L;
  float v[CO];
#pragma unroll
  for (int co = 0; co < CO; ++co) v[co] = tanhf(acc[co] + a.b[co]);
  if (!synth) {
    if (valid) {
#pragma unroll
      for (int co = 0; co < CO; ++co) a.y[((size_t)b * CO + co) * L + c] = v[co];
    }
    return;
  }
#pragma unroll
  for (int co = 0; co < CO; ++co) sb[co][tid] = valid ? v[co] : 0.f;
  __syncthreads();
  const int64_t n0 = (int64_t)CO * (c0 + halo);
  const int64_t NL = (int64_t)CO * L;
  float* yb = a.y + (size_t)b * NL;
  for (int o = tid; o < CO * TW; o += 256) {
    const int64_t n = n0 + o;
    if (n < NL) yb[n] = pqmf_sample((int)n, CO, a.taps, gl, [&](int k, int m) { return sb[k][m - c0]; });
  }
}

void launch_melgan_tail(const MelganTailArgs& a, int B, hipStream_t s) {
  TTS_REQUIRE(a.Co >= 1 && a.Co <= kMelganTailMaxCo, 3, "melgan tail: out_channels must lie in [1, 4]");
  TTS_REQUIRE(a.K % 2 == 1 && a.K <= kTailMaxK, 3, "melgan tail: the kernel size must be odd and <= 11");
  TTS_REQUIRE((a.K - 1) / 2 < a.L, 1, "melgan tail: the reflection pad must be smaller than the plane it pads");
  TTS_REQUIRE(!a.g || (a.taps >= 2 && a.taps % 2 == 0 && a.taps <= kTailMaxTaps && a.Co >= 2), 3,
              "melgan tail: the PQMF needs an even taps in [2, 126] and at least 2 bands");
  TTS_REQUIRE((int64_t)a.Co * a.L * 4 < (int64_t)1 << 31, 3, "melgan tail: the output exceeds 2 GiB per item");
  TTS_REQUIRE(B >= 1 && B <= 65535, 1, "melgan tail: batch size must lie in [1, 65535]");
  const int halo = a.g ? ((a.taps >> 1) + a.Co - 1) / a.Co : 0;
  const int TW = 256 - 2 * halo;
  const dim3 grid((a.L + TW - 1) / TW, B);
  switch (a.Co) {
    case 1: hipLaunchKernelGGL(melgan_tail_kernel<1>, grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL(melgan_tail_kernel<2>, grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL(melgan_tail_kernel<3>, grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL(melgan_tail_kernel<4>, grid, dim3(256), 0, s, a); break;
  }
  TTS_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------
// PQMF synthesis (TTS/vocoder/layers/pqmf.py) in its polyphase form, one output sample per thread
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pqmf_synthesis_kernel(const float* __restrict__ x, int N, int L,
                                                             const float* __restrict__ g, int taps,
                                                             float* __restrict__ y) {
  __shared__ float gl[8 * (kTailMaxTaps + 1)];
  for (int i = threadIdx.x; i < N * (taps + 1); i += 256) gl[i] = g[i];
  __syncthreads();
  const int b = blockIdx.y;
  const int64_t NL = (int64_t)N * L;
  const float* xb = x + (size_t)b * NL;
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < NL; n += (int64_t)gridDim.x * 256)
    y[(size_t)b * NL + n] = pqmf_sample((int)n, N, taps, gl, [&](int k, int m) {
      return (m >= 0 && m < L) ? xb[(size_t)k * L + m] : 0.f;
    });
}

void launch_pqmf_synthesis(const float* x, int B, int N, int L, const float* g, int taps, float* y, hipStream_t s) {
  TTS_REQUIRE(x && g && y, 1, "pqmf synthesis: NULL argument");
  TTS_REQUIRE(N >= 1 && N <= 8, 3, "pqmf synthesis: the number of bands must lie in [1, 8]");
  TTS_REQUIRE(taps >= 2 && taps % 2 == 0 && taps <= kTailMaxTaps, 3, "pqmf synthesis: taps must be even and lie in [2, 126]");
  TTS_REQUIRE(L >= 1 && B >= 1 && B <= 65535, 1, "pqmf synthesis: bad shape");
  TTS_REQUIRE((int64_t)N * L * 4 < (int64_t)1 << 31, 3, "pqmf synthesis: the output exceeds 2 GiB per item");
  const int64_t NL = (int64_t)N * L;
  const int bx = (int)std::min<int64_t>(65535, (NL + 255) / 256);
  hipLaunchKernelGGL(pqmf_synthesis_kernel, dim3(bx, B), dim3(256), 0, s, x, N, L, g, taps, y);
  TTS_HIP_CHECK(hipGetLastError());
}

}  // namespace tts
