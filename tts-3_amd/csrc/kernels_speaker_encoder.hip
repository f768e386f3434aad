// Small kernels of the ResNet speaker encoder (gfx950): pre-emphasis, mel filterbank, log + instance
// norm, the squeeze-and-excitation gate and its application, attentive pooling, the projection and
// the L2 norm.  All plain fp32; every reduction runs in one fixed order (strided per-lane sums, then a
// butterfly or an LDS tree), so results are the same bits on every run and do not depend on B.
// The convs are kernels_conv2d.hip, the STFT kernels_stft.hip.
#include <algorithm>

#include "speaker_encoder.hpp"

namespace tts {

namespace {
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ float wave_maxf(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}
// sum over the 256 threads of a workgroup, the same value in every thread (buf: 256 floats of LDS)
__device__ __forceinline__ float block_sum256(float v, float* buf) {
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
}  // namespace

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void spk_preemph_kernel(const float* __restrict__ x, int64_t N,
                                                          const float* __restrict__ filt, float* __restrict__ y) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const float* xb = x + (size_t)blockIdx.y * N;
  const float prev = n > 0 ? xb[n - 1] : xb[N > 1 ? 1 : 0];
  y[(size_t)blockIdx.y * N + n] = fmaf(filt[0], prev, filt[1] * xb[n]);
}

void launch_spk_preemph(const float* x, int B, int64_t N, const float* filt, float* y, hipStream_t s) {
  TTS_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && N < (int64_t)1 << 31, 1, "speaker encoder: bad wav shape");
  hipLaunchKernelGGL(spk_preemph_kernel, dim3((unsigned)((N + 255) / 256), B), dim3(256), 0, s, x, N, filt, y);
  TTS_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------
constexpr int kMelTile = 16;  // mel bands per thread
__global__ __launch_bounds__(256) void spk_mel_kernel(const float* __restrict__ P, int K, int M, int T,
                                                      const float* __restrict__ fb, float* __restrict__ mel) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int m0 = blockIdx.y * kMelTile;
  const int b = blockIdx.z;
  const float* pb = P + (size_t)b * K * T;
  float acc[kMelTile];
#pragma unroll
  for (int j = 0; j < kMelTile; ++j) acc[j] = 0.f;
  for (int k = 0; k < K; ++k) {
    const float p = t < T ? pb[(size_t)k * T + t] : 0.f;
#pragma unroll
    for (int j = 0; j < kMelTile; ++j) acc[j] = fmaf(m0 + j < M ? fb[(size_t)k * M + m0 + j] : 0.f, p, acc[j]);
  }
  if (t < T) {
#pragma unroll
    for (int j = 0; j < kMelTile; ++j)
      if (m0 + j < M) mel[((size_t)b * M + m0 + j) * T + t] = acc[j];
  }
}

void launch_spk_mel(const float* P, int B, int K, int M, int T, const float* fb, float* mel, hipStream_t s) {
  TTS_REQUIRE(B >= 1 && B <= 65535 && K >= 1 && M >= 1 && T >= 1, 1, "speaker encoder: bad spectrogram shape");
  hipLaunchKernelGGL(spk_mel_kernel, dim3((T + 255) / 256, (M + kMelTile - 1) / kMelTile, B), dim3(256), 0, s, P, K, M, T,
                     fb, mel);
  TTS_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void spk_instnorm_kernel(const float* __restrict__ x, int T, int log_in,
                                                           float* __restrict__ y) {
  __shared__ float buf[256];
  const size_t row = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * T;
  const float* xr = x + row;
  auto f = [&](int t) {
    const float v = xr[t];
    return log_in ? logf(v + 1e-6f) : v;
  };
  float s = 0.f;
  for (int t = threadIdx.x; t < T; t += 256) s += f(t);
  const float mean = block_sum256(s, buf) / (float)T;
  float q = 0.f;
  for (int t = threadIdx.x; t < T; t += 256) {
    const float d = f(t) - mean;
    q = fmaf(d, d, q);
  }
  const float var = block_sum256(q, buf) / (float)T;
  const float inv = 1.f / sqrtf(var + 1e-5f);
  for (int t = threadIdx.x; t < T; t += 256) y[row + t] = (f(t) - mean) * inv;
}

void launch_spk_instnorm(const float* x, int B, int M, int T, int log_in, float* y, hipStream_t s) {
  TTS_REQUIRE(B >= 1 && B <= 65535 && M >= 1 && T >= 1, 1, "speaker encoder: bad feature shape");
  hipLaunchKernelGGL(spk_instnorm_kernel, dim3(M, B), dim3(256), 0, s, x, T, log_in, y);
  TTS_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------
// One workgroup per batch item: wave w pools channels w, w + 4, ... (lane-strided sums of the conv's
// partial sums, then the butterfly), then fc.0 + relu on C / 8 threads and fc.2 + sigmoid on C threads.
__global__ __launch_bounds__(256) void spk_se_gate_kernel(const float* __restrict__ pool, int C, int n, float inv_count,
                                                          const float* __restrict__ w0, const float* __restrict__ b0,
                                                          const float* __restrict__ w2, const float* __restrict__ b2,
                                                          float* __restrict__ gate) {
  __shared__ float mean[TTS_SPK_MAX_FILTERS];
  __shared__ float hid[TTS_SPK_MAX_FILTERS / 8];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Cr = C >> 3;
  for (int c = wave; c < C; c += 4) {
    const float* p = pool + ((size_t)b * C + c) * n;
    float s = 0.f;
    for (int i = lane; i < n; i += 64) s += p[i];
    s = wave_sum(s);
    if (lane == 0) mean[c] = s * inv_count;
  }
  __syncthreads();
  if (tid < Cr) {
    float h = b0[tid];
    for (int c = 0; c < C; ++c) h = fmaf(w0[(size_t)tid * C + c], mean[c], h);
    hid[tid] = fmaxf(h, 0.f);
  }
  __syncthreads();
  if (tid < C) {
    float z = b2[tid];
    for (int j = 0; j < Cr; ++j) z = fmaf(w2[(size_t)tid * Cr + j], hid[j], z);
    gate[(size_t)b * C + tid] = 1.f / (1.f + expf(-z));
  }
}

void launch_spk_se_gate(const float* pool, int B, int C, int n, float count, const float* w0, const float* b0,
                        const float* w2, const float* b2, float* gate, hipStream_t s) {
  TTS_REQUIRE(C >= 8 && C % 8 == 0 && C <= TTS_SPK_MAX_FILTERS, 3,
              "speaker encoder: SE channels must be a multiple of 8 in [8, 256]");
  TTS_REQUIRE(B >= 1 && n >= 1 && count >= 1.f, 1, "speaker encoder: bad SE shape");
  hipLaunchKernelGGL(spk_se_gate_kernel, dim3(B), dim3(256), 0, s, pool, C, n, 1.f / count, w0, b0, w2, b2, gate);
  TTS_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void spk_se_apply_kernel(const float* __restrict__ h, const float* __restrict__ res,
                                                           const float* __restrict__ gate, int64_t P,
                                                           float* __restrict__ out) {
  const size_t plane = (size_t)blockIdx.z * gridDim.y + blockIdx.y;
  const float g = gate[plane];
  const size_t base = plane * (size_t)P;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = (int64_t)blockIdx.x * 1024 + k * 256 + threadIdx.x;
    if (i < P) out[base + i] = fmaxf(fmaf(h[base + i], g, res[base + i]), 0.f);
  }
}

void launch_spk_se_apply(const float* h, const float* res, const float* gate, int B, int C, int64_t P, float* out,
                         hipStream_t s) {
  TTS_REQUIRE(B >= 1 && B <= 65535 && C >= 1 && C <= 65535 && P >= 1 && P < (int64_t)1 << 31, 1,
              "speaker encoder: bad SE plane shape");
  hipLaunchKernelGGL(spk_se_apply_kernel, dim3((unsigned)((P + 1023) / 1024), C, B), dim3(256), 0, s, h, res, gate, P, out);
  TTS_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------
// One wave per (b, d) row; 4 rows per workgroup.
__global__ __launch_bounds__(256) void spk_pool_kernel(const float* __restrict__ x, const float* __restrict__ att, int D,
                                                       int T, int asp, float* __restrict__ pooled) {
  const int lane = threadIdx.x & 63;
  const int d = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int b = blockIdx.y;
  if (d >= D) return;  // wave-uniform
  const size_t row = ((size_t)b * D + d) * T;
  float m = -INFINITY;
  for (int t = lane; t < T; t += 64) m = fmaxf(m, att[row + t]);
  m = wave_maxf(m);
  float z = 0.f;
  for (int t = lane; t < T; t += 64) z += expf(att[row + t] - m);
  z = wave_sum(z);
  const float iz = 1.f / z;
  float mu = 0.f;
  for (int t = lane; t < T; t += 64) mu = fmaf(x[row + t], expf(att[row + t] - m) * iz, mu);
  mu = wave_sum(mu);
  const int DP = asp ? 2 * D : D;
  if (lane == 0) pooled[(size_t)b * DP + d] = mu;
  if (asp) {
    // sum_t w (x - mu)^2 = sum_t w x^2 - mu^2 (sum_t w = 1), without the cancellation
    float v = 0.f;
    for (int t = lane; t < T; t += 64) {
      const float c = x[row + t] - mu;
      v = fmaf(c * c, expf(att[row + t] - m) * iz, v);
    }
    v = wave_sum(v);
    if (lane == 0) pooled[(size_t)b * DP + D + d] = sqrtf(fmaxf(v, 1e-5f));
  }
}

void launch_spk_pool(const float* x, const float* att, int B, int D, int T, int asp, float* pooled, hipStream_t s) {
  TTS_REQUIRE(B >= 1 && B <= 65535 && D >= 1 && T >= 1, 1, "speaker encoder: bad pooling shape");
  hipLaunchKernelGGL(spk_pool_kernel, dim3((D + 3) / 4, B), dim3(256), 0, s, x, att, D, T, asp, pooled);
  TTS_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------
// One wave per output (b, j); 4 outputs per workgroup.
__global__ __launch_bounds__(256) void spk_fc_kernel(const float* __restrict__ p, int K, int J, const float* __restrict__ w,
                                                     const float* __restrict__ bias, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int b = blockIdx.y;
  if (j >= J) return;  // wave-uniform
  const float* pr = p + (size_t)b * K;
  const float* wr = w + (size_t)j * K;
  float s = 0.f;
  for (int k = lane; k < K; k += 64) s = fmaf(wr[k], pr[k], s);
  s = wave_sum(s);
  if (lane == 0) out[(size_t)b * J + j] = s + bias[j];
}

void launch_spk_fc(const float* p, int B, int K, int J, const float* w, const float* bias, float* out, hipStream_t s) {
  TTS_REQUIRE(B >= 1 && B <= 65535 && K >= 1 && J >= 1, 1, "speaker encoder: bad projection shape");
  hipLaunchKernelGGL(spk_fc_kernel, dim3((J + 3) / 4, B), dim3(256), 0, s, p, K, J, w, bias, out);
  TTS_HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void spk_l2norm_kernel(float* __restrict__ out, int J) {
  __shared__ float buf[256];
  float* r = out + (size_t)blockIdx.x * J;
  float q = 0.f;
  for (int j = threadIdx.x; j < J; j += 256) q = fmaf(r[j], r[j], q);
  const float nrm = fmaxf(sqrtf(block_sum256(q, buf)), 1e-12f);
  for (int j = threadIdx.x; j < J; j += 256) r[j] = r[j] / nrm;
}

void launch_spk_l2norm(float* out, int B, int J, hipStream_t s) {
  TTS_REQUIRE(B >= 1 && J >= 1, 1, "speaker encoder: bad embedding shape");
  hipLaunchKernelGGL(spk_l2norm_kernel, dim3(B), dim3(256), 0, s, out, J);
  TTS_HIP_CHECK(hipGetLastError());
}

}  // namespace tts
