// Kernels of the XTTS conditioning path (gfx950): GroupNorm over [B][C][T] planes, the perceiver's
// cross-attention over two key buffers, RMSNorm, the log-mel epilogue of wav_to_mel_cloning and
// the polyphase resampler, and the perceiver's products over its few latent columns with their bias /
// residual / GEGLU epilogues.  Interface: xtts_cond.hpp.  The encoder's products (and the perceiver's
// to_kv over the context) run on the 1x1 conv path and the encoder's self-attention on the flash kernel
// (kernels_fft_attn.hip).
// No atomics; every reduction runs in one fixed order (strided per-thread sums, then an LDS tree or a
// butterfly), so results are the same bits on every run, and a batch item is a grid index: row b does
// not depend on B.
#include <cmath>

#include "xtts_cond.hpp"

namespace tts {

namespace {
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
// reductions over the 256 threads of a workgroup, the same value in every thread (buf: 256 entries of LDS)
template <class T>
__device__ __forceinline__ T block_sum256(T v, T* buf) {
  const int tid = threadIdx.x;
  __syncthreads();  // buf may still be read from a previous call
  buf[tid] = v;
  __syncthreads();
#pragma unroll
  for (int n = 128; n >= 1; n >>= 1) {
    if (tid < n) buf[tid] += buf[tid + n];
    __syncthreads();
  }
  return buf[0];
}
__device__ __forceinline__ float block_max256(float v, float* buf) {
  const int tid = threadIdx.x;
  __syncthreads();
  buf[tid] = v;
  __syncthreads();
#pragma unroll
  for (int n = 128; n >= 1; n >>= 1) {
    if (tid < n) buf[tid] = fmaxf(buf[tid], buf[tid + n]);
    __syncthreads();
  }
  return buf[0];
}
}  // namespace

// --------------------------------------------------------------------------------------- GroupNorm
// One workgroup per (group, batch item): the group's C/G channels are one contiguous run of n floats.
// Pass 1 sums x, pass 2 sums (x - mean)^2 (never E[x^2] - E[x]^2), pass 3 writes.  The sums and the
// subtraction of the mean run in fp64: an fp32 mean of values near 100 is off by its rounding alone
// (4e-6), which would be the whole error budget of the normalised value.
constexpr int kGnThreads = 1024;  // 16 waves: the group's three passes are bound by loads in flight
__device__ __forceinline__ double gn_block_sum(double v, double* buf) {
  const int tid = threadIdx.x;
  __syncthreads();  // buf may still be read from a previous call
  buf[tid] = v;
  __syncthreads();
#pragma unroll
  for (int n = kGnThreads / 2; n >= 1; n >>= 1) {
    if (tid < n) buf[tid] += buf[tid + n];
    __syncthreads();
  }
  return buf[0];
}

__global__ __launch_bounds__(kGnThreads) void cond_groupnorm_kernel(const float* __restrict__ x,
                                                                    const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, int C, int T, int cpg,
                                                                    float eps, float* __restrict__ y) {
  __shared__ double buf[kGnThreads];
  const int g = blockIdx.x, b = blockIdx.y;
  const size_t base = ((size_t)b * C + (size_t)g * cpg) * T;
  const int n = cpg * T;
  const float* xg = x + base;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += kGnThreads) s += (double)xg[i];
  const double mean = gn_block_sum(s, buf) / (double)n;
  double q = 0.0;
  for (int i = threadIdx.x; i < n; i += kGnThreads) {
    const double d = (double)xg[i] - mean;
    q = fma(d, d, q);
  }
  const double var = gn_block_sum(q, buf) / (double)n;
  const double inv = 1.0 / sqrt(var + (double)eps);
  for (int i = threadIdx.x; i < n; i += kGnThreads) {
    const int c = g * cpg + i / T;
    const float v = (float)(((double)xg[i] - mean) * inv);
    y[base + i] = fmaf(v, gamma[c], beta[c]);
  }
}

void launch_cond_groupnorm(const float* x, const float* gamma, const float* beta, int B, int C, int T, int G, float eps,
                           float* y, hipStream_t s) {
  TTS_REQUIRE(x && gamma && beta && y, 1, "groupnorm: NULL argument");
  TTS_REQUIRE(B >= 1 && C >= 1 && T >= 1 && G >= 1 && C % G == 0, 1, "groupnorm: bad shape");
  TTS_REQUIRE(B <= 65535 && (int64_t)C * T * 4 < (int64_t)1 << 31, 3,
              "groupnorm: at most 65535 batch items, each plane below 2 GiB");
  hipLaunchKernelGGL(cond_groupnorm_kernel, dim3(G, B), dim3(kGnThreads), 0, s, x, gamma, beta, C, T, C / G, eps, y);
  TTS_HIP_CHECK(hipGetLastError());
}

// --------------------------------------------------------------------------------- cross-attention
// One workgroup per (latent query, head, batch item), 4 waves.  The L + T keys come from two buffers,
// the latents' first and the context's behind them: the concatenation is never written.
//   1. scores s_j = (q dh^-0.5) . k_j, one key per thread and pass (coalesced along the key axis), to LDS
//   2. max and sum of exp over the keys (LDS trees), p_j = exp(s_j - max) in place
//   3. channel d of the output on wave d mod 4: lanes stride over the keys, butterfly sum, / sum
// fp32 throughout (32 queries against a few hundred keys: launch-bound, not worth the matrix cores).
__global__ __launch_bounds__(256) void cond_cross_attn_kernel(const float* __restrict__ q, const float* __restrict__ kvl,
                                                              const float* __restrict__ kvc, int H, int dh, int L, int T,
                                                              float* __restrict__ out) {
  extern __shared__ float cx_smem[];
  float* buf = cx_smem;        // [256]
  float* qs = cx_smem + 256;   // [dh]
  float* sc = qs + dh;         // [L + T]
  const int l = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int inner = H * dh, nk = L + T;
  const float scale = 1.f / sqrtf((float)dh);
  for (int d = tid; d < dh; d += 256) qs[d] = q[((size_t)b * inner + h * dh + d) * L + l] * scale;
  __syncthreads();
  // rows of this head: k at h dh + d, v at inner + h dh + d
  const float* kl = kvl + ((size_t)b * 2 * inner + h * dh) * L;
  const float* kc = kvc + ((size_t)b * 2 * inner + h * dh) * T;
  float mx = -INFINITY;
  for (int j = tid; j < nk; j += 256) {
    float a = 0.f;
    if (j < L) {
      for (int d = 0; d < dh; ++d) a = fmaf(qs[d], kl[(size_t)d * L + j], a);
    } else {
      for (int d = 0; d < dh; ++d) a = fmaf(qs[d], kc[(size_t)d * T + (j - L)], a);
    }
    sc[j] = a;
    mx = fmaxf(mx, a);
  }
  mx = block_max256(mx, buf);
  float sum = 0.f;
  for (int j = tid; j < nk; j += 256) {
    const float p = expf(sc[j] - mx);
    sc[j] = p;
    sum += p;
  }
  sum = block_sum256(sum, buf);  // its barriers also publish p
  const float inv = 1.f / sum;
  const float* vl = kl + (size_t)inner * L;
  const float* vc = kc + (size_t)inner * T;
  for (int d = wave; d < dh; d += 4) {
    float a = 0.f;
    for (int j = lane; j < nk; j += 64)
      a = fmaf(sc[j], j < L ? vl[(size_t)d * L + j] : vc[(size_t)d * T + (j - L)], a);
    a = wave_sum(a);
    if (lane == 0) out[((size_t)b * inner + h * dh + d) * L + l] = a * inv;
  }
}

void launch_cond_cross_attn(const float* q, const float* kv_lat, const float* kv_ctx, int B, int H, int dh, int L, int T,
                            float* out, hipStream_t s) {
  TTS_REQUIRE(q && kv_lat && kv_ctx && out, 1, "cross attention: NULL argument");
  TTS_REQUIRE(B >= 1 && H >= 1 && dh >= 1 && L >= 1 && T >= 1, 1, "cross attention: bad shape");
  TTS_REQUIRE(L <= kCondMaxLatents && dh <= 256 && L + T <= kCondMaxKeys && B <= 65535 && H <= 65535, 3,
              "cross attention: at most " + std::to_string(kCondMaxLatents) + " latents, head size <= 256, at most " +
                  std::to_string(kCondMaxKeys) + " keys");
  TTS_REQUIRE((int64_t)2 * H * dh * T * 4 < (int64_t)1 << 31, 3, "cross attention: a context plane exceeds 2 GiB");
  const size_t lds = (size_t)(256 + dh + L + T) * sizeof(float);
  hipLaunchKernelGGL(cond_cross_attn_kernel, dim3(L, H, B), dim3(256), lds, s, q, kv_lat, kv_ctx, H, dh, L, T, out);
  TTS_HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------ perceiver products
// out[b][r][l] = epilogue(sum_k W[r][k] x[b][k][l]) over the L <= 64 latent columns: the perceiver's
// products have 32 B columns in all, a quarter of a conv tile's columns and 8 workgroups for a 1024-row
// matrix, and are bound by streaming W once.  Here the lanes run along k, so W streams as stored (row-major,
// coalesced 4-byte loads: a row of K = 2730 or 341 floats has no 16-byte alignment and K has a tail; bf16
// mode: the matrix is stored as bf16 and widened on load).  A workgroup of 4 waves owns 8 rows (GEGLU: 4
// row pairs r, I + r) and 32 columns; per chunk of 256 k it stages x[256][32] in LDS (rows of 36 floats:
// the lanes' 16-byte reads fall on distinct banks), and every wave runs its 2 rows: lane j adds
// W[r][k0 + 64 i + j] x[k0 + 64 i + j][0..32) into 2 x 32 accumulators.  At the end the 64 sums of a wave
// are reduced over its lanes by a butterfly that halves the values per lane at every step (63 exchanges),
// which leaves value (row, column) on lane 32 row + column: one fixed order, no atomics.
// Epilogues: + bias; + bias + residual; GEGLU gelu_erf(gate + b[I + r]) (a + b[r]).
constexpr int kSkKC = 256, kSkRows = 8, kSkXP = 36;
enum { kSkEpiBias = 0, kSkEpiRes = 1, kSkEpiGeglu = 2 };
struct CondSkinnyArgs {
  const void* w;      // [R][K] fp32, or bf16
  const float* bias;  // [R] or nullptr
  const float* x;     // [B][K][L]
  const float* res;   // [B][R][L] (kSkEpiRes)
  float* out;         // [B][R][L] (GEGLU: [B][I][L])
  int R, K, L, I;
};

template <bool BF, int EPI>
__global__ __launch_bounds__(256) void cond_skinny_kernel(CondSkinnyArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[kSkKC * kSkXP];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b = blockIdx.z, c0 = blockIdx.y * 32;
  const int L = a.L, K = a.K;
  const int Rt = EPI == kSkEpiGeglu ? a.I : a.R;
  // this wave's two matrix rows (a row past the end reads nothing and writes nothing)
  int row[2];
  if constexpr (EPI == kSkEpiGeglu) {
    row[0] = blockIdx.x * 4 + wave;
    row[1] = row[0] + a.I;
  } else {
    row[0] = blockIdx.x * kSkRows + 2 * wave;
    row[1] = row[0] + 1;
  }
  const bool live[2] = {row[0] < Rt, EPI == kSkEpiGeglu ? row[0] < Rt : row[1] < Rt};
  const float* xb = a.x + (size_t)b * K * L;
  auto wload = [&](size_t i) {
    if constexpr (BF) return __uint_as_float((unsigned)static_cast<const unsigned short*>(a.w)[i] << 16);
    else return static_cast<const float*>(a.w)[i];
  };
  float acc[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) acc[i] = 0.f;
  for (int k0 = 0; k0 < K; k0 += kSkKC) {
    __syncthreads();  // every wave is done with the previous chunk
#pragma unroll 4
    for (int i = 0; i < kSkKC * 32 / 256; ++i) {
      const int e = i * 256 + t, kk = e >> 5, c = e & 31;
      xs[kk * kSkXP + c] = (c0 + c < L && k0 + kk < K) ? xb[(size_t)(k0 + kk) * L + c0 + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kSkKC / 64; ++i) {
      const int kk = i * 64 + lane, k = k0 + kk;
      float w[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) w[r] = (live[r] && k < K) ? wload((size_t)row[r] * K + k) : 0.f;
      const f32x4* xr = reinterpret_cast<const f32x4*>(xs + kk * kSkXP);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const f32x4 xv = xr[q];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[32 * r + 4 * q + j] = fmaf(w[r], xv[j], acc[32 * r + 4 * q + j]);
      }
    }
  }
  // butterfly with halving: after the step of mask m, a lane with (lane & m) set keeps the upper half
#pragma unroll
  for (int n = 32, m = 32; n >= 1; n >>= 1, m >>= 1) {
    const bool up = (lane & m) != 0;
#pragma unroll
    for (int i = 0; i < n; ++i) {
      const float lo = acc[i], hi = acc[i + n];
      const float other = __shfl_xor(up ? lo : hi, m);
      acc[i] = (up ? hi : lo) + other;
    }
  }
  const float v = acc[0];  // value (lane >> 5, lane & 31)
  const int col = c0 + (lane & 31);
  if constexpr (EPI == kSkEpiGeglu) {
    const float g = __shfl(v, (lane & 31) + 32);
    if (lane < 32 && live[0] && col < L) {
      const float av = v + a.bias[row[0]], gv = g + a.bias[row[1]];
      a.out[((size_t)b * Rt + row[0]) * L + col] = 0.5f * gv * (1.f + erff(gv * 0.70710678118654752f)) * av;
    }
  } else {
    const int r = lane >> 5;
    if (live[r] && col < L) {
      const size_t o = ((size_t)b * Rt + row[r]) * L + col;
      float y = v + (a.bias ? a.bias[row[r]] : 0.f);
      if constexpr (EPI == kSkEpiRes) y += a.res[o];
      a.out[o] = y;
    }
  }
}

namespace {
template <bool BF, int EPI>
void launch_cond_skinny_e(const CondSkinnyArgs& a, const dim3& grid, hipStream_t s) {
  hipLaunchKernelGGL((cond_skinny_kernel<BF, EPI>), grid, dim3(256), 0, s, a);
}
template <bool BF>
void launch_cond_skinny_b(int epi, const CondSkinnyArgs& a, const dim3& grid, hipStream_t s) {
  if (epi == kSkEpiGeglu) launch_cond_skinny_e<BF, kSkEpiGeglu>(a, grid, s);
  else if (epi == kSkEpiRes) launch_cond_skinny_e<BF, kSkEpiRes>(a, grid, s);
  else launch_cond_skinny_e<BF, kSkEpiBias>(a, grid, s);
}
}  // namespace

void launch_cond_product(const void* w, bool bf16, const float* bias, const float* x, const float* res, int B, int R,
                         int K, int L, int geglu, float* out, hipStream_t s) {
  TTS_REQUIRE(w && x && out, 1, "perceiver product: NULL argument");
  TTS_REQUIRE(B >= 1 && R >= 1 && K >= 1 && L >= 1, 1, "perceiver product: bad shape");
  TTS_REQUIRE(!geglu || (bias && R % 2 == 0 && !res), 1, "perceiver product: GEGLU needs a bias and an even row count");
  TTS_REQUIRE(L <= kCondMaxLatents && B <= 65535 && (int64_t)R * K < (int64_t)1 << 31 &&
                  (int64_t)K * L * 4 < (int64_t)1 << 31 && (int64_t)R * L * 4 < (int64_t)1 << 31,
              3, "perceiver product: at most " + std::to_string(kCondMaxLatents) + " columns, matrices below 2^31 entries");
  TTS_REQUIRE(out != x && out != res, 1, "perceiver product: the output must not alias an input");
  CondSkinnyArgs a{w, bias, x, res, out, R, K, L, geglu ? R / 2 : 0};
  const int Rt = geglu ? R / 2 : R;
  const int per = geglu ? 4 : kSkRows;  // rows (GEGLU: row pairs) of one workgroup
  const dim3 grid((Rt + per - 1) / per, (L + 31) / 32, B);
  const int epi = geglu ? kSkEpiGeglu : (res ? kSkEpiRes : kSkEpiBias);
  if (bf16) launch_cond_skinny_b<true>(epi, a, grid, s);
  else launch_cond_skinny_b<false>(epi, a, grid, s);
  TTS_HIP_CHECK(hipGetLastError());
}

// --------------------------------------------------------------------------------------- broadcast
__global__ __launch_bounds__(256) void cond_broadcast_kernel(const float* __restrict__ x, int n, float* __restrict__ y) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[(size_t)blockIdx.y * n + i] = x[i];
}

void launch_cond_broadcast(const float* x, int B, int64_t n, float* y, hipStream_t s) {
  TTS_REQUIRE(x && y, 1, "broadcast: NULL argument");
  TTS_REQUIRE(B >= 1 && n >= 1, 1, "broadcast: bad shape");
  TTS_REQUIRE(B <= 65535 && n < (int64_t)1 << 31, 3, "broadcast: shape outside the limits");
  hipLaunchKernelGGL(cond_broadcast_kernel, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, s, x, (int)n, y);
  TTS_HIP_CHECK(hipGetLastError());
}

// ----------------------------------------------------------------------------------------- RMSNorm
__global__ __launch_bounds__(256) void cond_rmsnorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                           int E, int L, float* __restrict__ y) {
  __shared__ float buf[256];
  const int l = blockIdx.x, b = blockIdx.y;
  const float* xb = x + (size_t)b * E * L + l;
  float q = 0.f;
  for (int c = threadIdx.x; c < E; c += 256) {
    const float v = xb[(size_t)c * L];
    q = fmaf(v, v, q);
  }
  const float norm = sqrtf(block_sum256(q, buf));
  const float k = sqrtf((float)E) / fmaxf(norm, 1e-12f);
  for (int c = threadIdx.x; c < E; c += 256) y[((size_t)b * E + c) * L + l] = xb[(size_t)c * L] * k * gamma[c];
}

void launch_cond_rmsnorm(const float* x, const float* gamma, int B, int E, int L, float* y, hipStream_t s) {
  TTS_REQUIRE(x && gamma && y, 1, "rmsnorm: NULL argument");
  TTS_REQUIRE(B >= 1 && E >= 1 && L >= 1, 1, "rmsnorm: bad shape");
  TTS_REQUIRE(B <= 65535 && L <= 65535 && (int64_t)E * L * 4 < (int64_t)1 << 31, 3, "rmsnorm: shape outside the limits");
  hipLaunchKernelGGL(cond_rmsnorm_kernel, dim3(L, B), dim3(256), 0, s, x, gamma, E, L, y);
  TTS_HIP_CHECK(hipGetLastError());
}

// ----------------------------------------------------------------------------------------- log-mel
// One thread per (band, frame).  The filterbank's columns are triangles: band m is nonzero on the bins
// [range[2 m], range[2 m + 1]) only (found on the host from fb itself), so a thread walks a few dozen bins,
// k ascending, instead of all n_fft / 2 + 1; the skipped products are exact zeros, the sum is the same.
__global__ __launch_bounds__(256) void cond_logmel_kernel(const float* __restrict__ P, int K, int M, int T,
                                                          const float* __restrict__ fb, const int* __restrict__ range,
                                                          const float* __restrict__ norms, float* __restrict__ mel) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int m = blockIdx.y, b = blockIdx.z;
  if (t >= T) return;
  const float* pb = P + (size_t)b * K * T;
  const int k0 = max(range[2 * m], 0), k1 = min(range[2 * m + 1], K);
  float acc = 0.f;
  for (int k = k0; k < k1; ++k) acc = fmaf(fb[(size_t)k * M + m], pb[(size_t)k * T + t], acc);
  mel[((size_t)b * M + m) * T + t] = logf(fmaxf(acc, 1e-5f)) / norms[m];
}

void launch_cond_logmel(const float* P, int B, int K, int M, int T, const float* fb, const int* range,
                        const float* norms, float* mel, hipStream_t s) {
  TTS_REQUIRE(P && fb && range && norms && mel, 1, "log-mel: NULL argument");
  TTS_REQUIRE(B >= 1 && B <= 65535 && K >= 1 && M >= 1 && M <= 65535 && T >= 1, 1, "log-mel: bad spectrogram shape");
  hipLaunchKernelGGL(cond_logmel_kernel, dim3((T + 255) / 256, M, B), dim3(256), 0, s, P, K, M, T, fb, range, norms, mel);
  TTS_HIP_CHECK(hipGetLastError());
}

// --------------------------------------------------------------------------------------- resampler
// One output sample per thread: frame f = i / n, phase p = i mod n, the 2 w + o taps in ascending
// order.  The lanes of a wave share a frame (or two), so the input reads are broadcasts and the table
// reads (transposed, [tap][phase]) are coalesced.  The sum runs in fp64 and is rounded once.
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ x, int64_t N,
                                                       const float* __restrict__ table, int o, int n, int w, int64_t Nout,
                                                       float* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= Nout) return;
  const float* xb = x + (size_t)blockIdx.y * N;
  const int64_t f = i / n;
  const int p = (int)(i - f * n);
  const int taps = 2 * w + o;
  const int64_t s0 = f * o - w;  // input index of tap 0
  double acc = 0.0;
  for (int k = 0; k < taps; ++k) {
    const int64_t src = s0 + k;
    if (src >= 0 && src < N) acc = fma((double)table[(size_t)k * n + p], (double)xb[src], acc);
  }
  y[(size_t)blockIdx.y * Nout + i] = (float)acc;
}

void launch_resample(const float* x, int B, int64_t N, const float* table, int o, int n, int w, int64_t Nout, float* y,
                     hipStream_t s) {
  TTS_REQUIRE(x && table && y, 1, "resample: NULL argument");
  TTS_REQUIRE(B >= 1 && N >= 1 && Nout >= 1 && o >= 1 && n >= 1 && w >= 1, 1, "resample: bad shape");
  TTS_REQUIRE(B <= 65535 && N < (int64_t)1 << 31 && Nout < (int64_t)1 << 31, 3,
              "resample: at most 65535 rows of fewer than 2^31 samples");
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)((Nout + 255) / 256), B), dim3(256), 0, s, x, N, table, o, n, w, Nout,
                     y);
  TTS_HIP_CHECK(hipGetLastError());
}

}  // namespace tts
