// ForwardTTS (FastPitch) glue kernels on gfx950: the unmasked token embedding, the encoder's mask
// and speaker add, the FastPitch duration rule, the pitch embedding and the positional encoding.
// All activations are [B][C][T] fp32; these are small memory-bound launches (plain fp32).
//
// Reference (Coqui TTS 0.22.0): TTS/tts/models/forward_tts.py (format_durations, _forward_encoder,
// _forward_pitch_predictor, _forward_decoder), TTS/tts/layers/generic/pos_encoding.py.
#include "forward_tts.hpp"

namespace tts {

// x[b][c][t] = emb[tok[b][t]][c] (every column: the reference's encoder sees the padded tokens'
// embeddings too); mask[b][t] = t < len[b]
__global__ void __launch_bounds__(256) ftts_embed_kernel(const int64_t* __restrict__ tok, const int64_t* __restrict__ len,
                                                         const float* __restrict__ emb, float* __restrict__ x,
                                                         float* __restrict__ mask, int H, int T, int num_chars) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * 64 + (threadIdx.x & 63);
  const int cq = threadIdx.x >> 6;
  if (t >= T) return;
  int64_t id = tok[(size_t)b * T + t];
  // the reference raises IndexError on an out-of-range id: clamp instead of reading out of bounds
  id = id < 0 ? 0 : (id >= num_chars ? num_chars - 1 : id);
  const float* e = emb + (size_t)id * H;
  float* xo = x + (size_t)b * H * T + t;
  for (int c = cq; c < H; c += 4) xo[(size_t)c * T] = e[c];
  if (cq == 0) mask[(size_t)b * T + t] = (int64_t)t < len[b] ? 1.f : 0.f;
}

void launch_ftts_embed(const int64_t* tok, const int64_t* len, const float* emb, float* x, float* mask, int B, int H,
                       int T, int num_chars, hipStream_t s) {
  TTS_REQUIRE(B >= 1 && B <= 65535, 1, "forward_tts: batch size must lie in [1, 65535]");
  hipLaunchKernelGGL(ftts_embed_kernel, dim3(ceil_div(T, 64), B), dim3(256), 0, s, tok, len, emb, x, mask, H, T,
                     num_chars);
  TTS_HIP_CHECK(hipGetLastError());
}

// y[b][c][t] = x[b][c][t] * mask[b][t] + emb_g[spk[b]][c]   (encoder(...) * x_mask + g; no table: + 0)
__global__ void __launch_bounds__(256) ftts_mask_add_kernel(const float* __restrict__ x, const float* __restrict__ mask,
                                                            const float* __restrict__ table,
                                                            const int64_t* __restrict__ spk, float* __restrict__ y, int C,
                                                            int T, int num_speakers) {
  const int b = blockIdx.z, c = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  float g = 0.f;
  if (table) {
    int64_t id = spk[b];
    id = id < 0 ? 0 : (id >= num_speakers ? num_speakers - 1 : id);
    g = table[(size_t)id * C + c];
  }
  const size_t i = ((size_t)b * C + c) * T + t;
  y[i] = x[i] * mask[(size_t)b * T + t] + g;
}

void launch_ftts_mask_add(const float* x, const float* mask, const float* table, const int64_t* spk, float* y, int B,
                          int C, int T, int num_speakers, hipStream_t s) {
  TTS_REQUIRE(B <= 65535 && C <= 65535, 1, "forward_tts: bad channel count or batch size");
  hipLaunchKernelGGL(ftts_mask_add_kernel, dim3(ceil_div(T, 256), C, B), dim3(256), 0, s, x, mask, table, spk, y, C, T,
                     num_speakers);
  TTS_HIP_CHECK(hipGetLastError());
}

// format_durations (forward_tts.py): o_dr = (exp(o_dr_log) - 1) * x_mask * length_scale;
// o_dr[o_dr < 1] = 1; o_dr = round(o_dr) (torch.round: half to even = rintf), then times the token
// mask (a padded token gets no frames; with the reference's all-ones mask nothing changes).
// given != nullptr: those durations instead.  y_len[b] = sum (exact in fp32 below 2^24).
__global__ void __launch_bounds__(256) ftts_durations_kernel(const float* __restrict__ dlog, const float* __restrict__ xm,
                                                             const float* __restrict__ given, float* __restrict__ dur,
                                                             int64_t* __restrict__ y_len, int T, float length_scale) {
  __shared__ float part[4];
  const int b = blockIdx.x;
  float s = 0.f;
  for (int t = threadIdx.x; t < T; t += 256) {
    const size_t i = (size_t)b * T + t;
    float d;
    if (given) {
      d = given[i];
    } else {
      const float m = xm[i];
      const float raw = (expf(dlog[i]) - 1.f) * m * length_scale;
      d = rintf(raw < 1.f ? 1.f : raw) * m;
    }
    dur[i] = d;
    s += d;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) y_len[b] = (int64_t)(part[0] + part[1] + part[2] + part[3]);
}

void launch_ftts_durations(const float* dlog, const float* xm, const float* given, float* dur, int64_t* y_len, int B,
                           int T, float length_scale, hipStream_t s) {
  hipLaunchKernelGGL(ftts_durations_kernel, dim3(B), dim3(256), 0, s, dlog, xm, given, dur, y_len, T, length_scale);
  TTS_HIP_CHECK(hipGetLastError());
}

// x[b][c][t] += bias[c] + sum_j w[c][j] pitch[b][t - (k-1)/2 + j]   (o_en + pitch_emb(o_pitch), zero padding)
__global__ void __launch_bounds__(256) ftts_pitch_emb_kernel(const float* __restrict__ pitch, const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ x, int C,
                                                             int T, int k) {
  const int b = blockIdx.z, c = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const int p = (k - 1) / 2;
  float v = 0.f;
  for (int j = 0; j < k; ++j) {
    const int ts = t - p + j;
    if (ts >= 0 && ts < T) v = fmaf(w[c * k + j], pitch[(size_t)b * T + ts], v);
  }
  x[((size_t)b * C + c) * T + t] += v + bias[c];
}

void launch_ftts_pitch_emb(const float* pitch, const float* w, const float* bias, float* x, int B, int C, int T, int k,
                           hipStream_t s) {
  hipLaunchKernelGGL(ftts_pitch_emb_kernel, dim3(ceil_div(T, 256), C, B), dim3(256), 0, s, pitch, w, bias, x, C, T, k);
  TTS_HIP_CHECK(hipGetLastError());
}

// PositionalEncoding.forward: x = x * scale + pe[c][t] * mask[b][t]   (pe: [C][pe_len])
__global__ void __launch_bounds__(256) ftts_posenc_kernel(float* __restrict__ x, const float* __restrict__ pe,
                                                          const float* __restrict__ mask, int C, int T, int pe_len,
                                                          float scale) {
  const int b = blockIdx.z, c = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const size_t i = ((size_t)b * C + c) * T + t;
  x[i] = x[i] * scale + pe[(size_t)c * pe_len + t] * mask[(size_t)b * T + t];
}

void launch_ftts_posenc(float* x, const float* pe, const float* mask, int B, int C, int T, int pe_len, float scale,
                        hipStream_t s) {
  TTS_REQUIRE(T <= pe_len, 1, "forward_tts: more frames than the positional encoding holds");
  hipLaunchKernelGGL(ftts_posenc_kernel, dim3(ceil_div(T, 256), C, B), dim3(256), 0, s, x, pe, mask, C, T, pe_len,
                     scale);
  TTS_HIP_CHECK(hipGetLastError());
}

}  // namespace tts
