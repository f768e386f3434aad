// Tacotron2 kernels: the skinny recurrent product with the LSTM cell (or a bias) as its epilogue, the
// location-sensitive attention step, the stop / bookkeeping / next-prenet step, and the glue around the
// conv path (embedding, speaker columns, inputs_layer, plane transposes, tanh, residual).
//
// Every dependency between phases of a decoder step is a kernel boundary: no kernel waits on another
// workgroup, and every loop bound is a launch argument.  Utterances whose done[b] is set are skipped by
// every kernel, so steps enqueued past the end of the last utterance change nothing.
#include "tacotron2.hpp"

namespace tts {

namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// ---------------------------------------------------------------------------- skinny product
// One workgroup: 16 packed rows (an LSTM's 4 units x 4 gates) against [x0 | x1 | x2] for BT batch columns.
// Thread (u = tid & 3, ks = tid >> 2) loads the 4 rows 4u .. 4u + 3 of column k = ks, ks + 64, ... as one
// 16-byte (bf16: 8-byte) load: a wave reads 1 KiB of consecutive weights per instruction, and each
// weight is read once.  x is staged through LDS in chunks of kChunkFloats / BT columns.  The 64
// k-slices are then summed in a fixed order (16 slices of a wave in sequence, the four waves in
// sequence), so column b's result does not depend on BT.
constexpr int kChunkFloats = 8192;  // 32 KiB of LDS, reused for the partial sums

template <int BT, bool BF16W>
__global__ __launch_bounds__(256) void skinny_kernel(SkinnyArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[kChunkFloats];
  const int tid = threadIdx.x, u = tid & 3, ks = tid >> 2, dir = blockIdx.z, rb = blockIdx.x;
  float acc[4][BT];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int b = 0; b < BT; ++b) acc[g][b] = 0.f;

  const int KC = kChunkFloats / BT;  // a multiple of 64
  const float* x0 = a.x[dir][0];
  const float* x1 = a.x[dir][1];
  const float* x2 = a.x[dir][2];
  const int n0 = a.n[0], n01 = a.n[0] + a.n[1];
  const size_t wbase = (size_t)rb * a.Kp * kSkinnyRows;
  for (int k0 = 0; k0 < a.Kp; k0 += KC) {
    const int kc = min(KC, a.Kp - k0);
    __syncthreads();
    if (BT >= 4) {  // segments start on 16-byte boundaries: whole float4s
      for (int i = tid; i < kc * BT / 4; i += 256) {
        const int k = k0 + (4 * i) / BT, bq = (4 * i) % BT;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < a.K) {
          const float* src = k < n0 ? x0 + (size_t)k * BT : (k < n01 ? x1 + (size_t)(k - n0) * BT : x2 + (size_t)(k - n01) * BT);
          v = *reinterpret_cast<const float4*>(src + bq);
        }
        reinterpret_cast<float4*>(smem)[i] = v;
      }
    } else {
      for (int i = tid; i < kc * BT; i += 256) {
        const int k = k0 + i / BT, b = i % BT;
        float v = 0.f;
        if (k < a.K) {
          if (k < n0) v = x0[(size_t)k * BT + b];
          else if (k < n01) v = x1[(size_t)(k - n0) * BT + b];
          else v = x2[(size_t)(k - n01) * BT + b];
        }
        smem[i] = v;
      }
    }
    __syncthreads();
#pragma clang loop unroll_count(BT <= 8 ? 8 : 4)
    for (int kk = ks; kk < kc; kk += 64) {
      float w[4];
      if (BF16W) {
        const uint2 p = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(a.w[dir]) + wbase +
                                                        (size_t)(k0 + kk) * kSkinnyRows + 4 * u);
        w[0] = __uint_as_float(p.x << 16);
        w[1] = __uint_as_float(p.x & 0xffff0000u);
        w[2] = __uint_as_float(p.y << 16);
        w[3] = __uint_as_float(p.y & 0xffff0000u);
      } else {
        const float4 p = *reinterpret_cast<const float4*>(static_cast<const float*>(a.w[dir]) + wbase +
                                                          (size_t)(k0 + kk) * kSkinnyRows + 4 * u);
        w[0] = p.x; w[1] = p.y; w[2] = p.z; w[3] = p.w;
      }
      const float* xs = smem + kk * BT;
#pragma unroll
      for (int b = 0; b < BT; ++b) {
        const float xv = xs[b];
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g][b] = fmaf(w[g], xv, acc[g][b]);
      }
    }
  }

  // partial sums through LDS, one wave at a time: part[ks16][row16][BT]; thread (u2, b2) of the first
  // 4 BT threads sums its 4 rows
  const int wave = tid >> 6, ksw = ks & 15;
  const int u2 = tid / BT, b2 = tid % BT;  // epilogue owner of (unit u2, column b2), tid < 4 BT
  float tot[4] = {0.f, 0.f, 0.f, 0.f};
  for (int wv = 0; wv < 4; ++wv) {
    __syncthreads();
    if (wave == wv) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int b = 0; b < BT; ++b) smem[(ksw * kSkinnyRows + 4 * u + g) * BT + b] = acc[g][b];
    }
    __syncthreads();
    if (tid < 4 * BT) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float s = 0.f;
        for (int q = 0; q < 16; ++q) s += smem[(q * kSkinnyRows + 4 * u2 + g) * BT + b2];
        tot[g] += s;
      }
    }
  }
  if (tid >= 4 * BT || b2 >= a.B) return;
  const int b = b2;
  if (a.done && a.done[b]) return;

  if (!a.lstm) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int row = rb * kSkinnyRows + 4 * u2 + g;
      if (row < a.R) a.out[(size_t)b * a.ldo + row] = tot[g] + (a.bias[dir] ? a.bias[dir][row] : 0.f);
    }
    return;
  }
  const int H = a.H, unit = rb * kLstmUnitBlock + u2;
  int t = 0;
  if (a.pre || a.y) {
    const int len = a.len ? (int)min((int64_t)a.T, max((int64_t)0, a.len[b])) : a.T;
    if (a.step >= len) return;
    t = dir == 0 ? a.step : len - 1 - a.step;
  }
  float z[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    z[g] = tot[g] + (a.bias[dir] ? a.bias[dir][4 * unit + g] : 0.f);
    if (a.pre) z[g] += a.pre[((size_t)b * a.ndir * 4 * H + (size_t)dir * 4 * H + (size_t)g * H + unit) * a.T + t];
  }
  const float ig = sigmoidf_(z[0]), fg = sigmoidf_(z[1]), gg = tanhf(z[2]), og = sigmoidf_(z[3]);
  float* c = a.c[dir] + (size_t)unit * BT + b;
  const float cn = fmaf(fg, *c, ig * gg);
  const float hn = og * tanhf(cn);
  *c = cn;
  a.h_out[dir][(size_t)unit * BT + b] = hn;
  if (a.y) a.y[((size_t)b * a.T + t) * a.ldy + dir * H + unit] = hn;
}

template <int BT>
void launch_skinny_bt(const SkinnyArgs& a, hipStream_t s) {
  const int blocks = a.lstm ? a.H / kLstmUnitBlock : ceil_div(a.R, kSkinnyRows);
  const dim3 grid(blocks, 1, a.ndir);
  if (a.bf16) hipLaunchKernelGGL((skinny_kernel<BT, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((skinny_kernel<BT, false>), grid, dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------- block reductions
// fixed tree over the workgroup's 1024 values: the result does not depend on anything but the values
constexpr int kWgThreads = 1024;
__device__ __forceinline__ float block_sum(float v, float* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = kWgThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}
__device__ __forceinline__ float block_max(float v, float* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = kWgThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
    __syncthreads();
  }
  return red[0];
}

// ---------------------------------------------------------------------------- attention step
// One workgroup of 1024 threads per utterance.
//   0. pq = Wq q: a wave per row, four rows in flight, lanes along k, butterfly sum
//   per tile of 128 encoder positions, thread (position tl, split sp of 8):
//   1. location features f[i][t] = sum_c,j loc_w[i][c][j] [aw ; aw_cum][c][t + j - pad], i = sp, sp + 8, ...
//      (the window of 31 positions in registers, the weights as broadcast LDS reads)
//   2. e[t] = v_b + sum_sp sum_{r = sp, sp + 8, ...} v[r] tanh(pq[r] + processed_inputs[r][t] + loc_d[r] . f[.][t])
//      (the 8 partial sums through LDS, added in order); masked positions get probability exactly 0
//   then sigmoid(e) / sum or softmax over all of T (weights kept in LDS), aw_cum_out = aw_cum_in + a, the
//   alignment row, and context[d] = sum_t a[t] inputs[t][d] (threads over d, t in 4 interleaved parts
//   added in order).
constexpr int kAttnSplit = kWgThreads / kT2AttnTile;  // 8
constexpr int kLocRow = 32;                           // a location-conv row (kT2MaxLocK taps) padded
__global__ __launch_bounds__(kWgThreads) void t2_attention_kernel(T2AttnArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (a.done[b]) return;
  __shared__ float scratch[kT2MaxF * kT2AttnTile];  // q (phase 0), then f[i][tl], then the context parts
  __shared__ float pq[kT2MaxA], vv[kT2MaxA];
  // rows padded with zeros to 32 floats: a thread reads them as 16-byte broadcasts against registers
  __shared__ __attribute__((aligned(16))) float wl[kT2MaxF * 2 * kLocRow];
  __shared__ __attribute__((aligned(16))) float wd[kT2MaxA * kT2MaxF];
  __shared__ float aws[2][kT2AttnTile + kT2MaxLocK - 1];
  __shared__ float ep[kAttnSplit][kT2AttnTile];
  __shared__ float as[TTS_TACOTRON2_MAX_TOKENS];
  __shared__ float red[kWgThreads];
  static_assert(kT2MaxQ <= kT2MaxF * kT2AttnTile, "q is staged in the feature buffer");
  const int T = a.T, A = a.A, F = a.F, Kl = a.Kl, Q = a.Q, pad = (a.Kl - 1) / 2;
  const int len = a.len ? (int)min((int64_t)T, max((int64_t)0, a.len[b])) : T;
  for (int i = tid; i < Q; i += kWgThreads) scratch[i] = a.query[(size_t)i * a.BT + b];
  for (int i = tid; i < A; i += kWgThreads) vv[i] = a.v[i];
  for (int i = tid; i < kT2MaxF * 2 * kLocRow; i += kWgThreads) {
    const int row = i / kLocRow, j = i % kLocRow;
    wl[i] = (row < 2 * F && j < Kl) ? a.loc_w[row * Kl + j] : 0.f;
  }
  for (int i = tid; i < kT2MaxA * kT2MaxF; i += kWgThreads) {
    const int r = i / kT2MaxF, f = i % kT2MaxF;
    wd[i] = (r < A && f < F) ? a.loc_d[r * F + f] : 0.f;
  }
  __syncthreads();
  {
    const int wave = tid >> 6, lane = tid & 63;
    for (int r0 = wave; r0 < A; r0 += 64) {  // rows r0, r0 + 16, r0 + 32, r0 + 48
      float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
      for (int k = lane; k < Q; k += 64) {
        const float qv = scratch[k];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (r0 + 16 * j < A) s[j] = fmaf(a.wq[(size_t)(r0 + 16 * j) * Q + k], qv, s[j]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        for (int m = 32; m > 0; m >>= 1) s[j] += __shfl_xor(s[j], m, 64);
        if (lane == 0 && r0 + 16 * j < A) pq[r0 + 16 * j] = s[j];
      }
    }
  }
  const float vb = a.v_bias[0];
  const float* aw_in = a.aw_in + (size_t)b * T;
  const float* awc_in = a.awc_in + (size_t)b * T;
  const float* pinp = a.pinp + (size_t)b * A * T;
  const int tl = tid & (kT2AttnTile - 1);
  const int sp = __builtin_amdgcn_readfirstlane(tid / kT2AttnTile);  // the same for a whole wave

  float lmax = -INFINITY, lsum = 0.f;
  for (int t0 = 0; t0 < T; t0 += kT2AttnTile) {
    __syncthreads();  // pq and the previous tile's f / ep are done with
    for (int i = tid; i < kT2AttnTile + kT2MaxLocK - 1; i += kWgThreads) {  // the whole buffer: finite values
      const int t = t0 + i - pad;
      const bool in = t >= 0 && t < T;
      aws[0][i] = in ? aw_in[t] : 0.f;
      aws[1][i] = in ? awc_in[t] : 0.f;
    }
    __syncthreads();
    {
      float win[2][kLocRow];  // this position's window of [aw ; aw_cum]; taps past Kl meet zero weights
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int j = 0; j < kLocRow; ++j) win[c][j] = j < kT2MaxLocK ? aws[c][tl + j] : 0.f;
      for (int i = sp; i < kT2MaxF; i += kAttnSplit) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int j = 0; j < kLocRow; ++j) s = fmaf(wl[(i * 2 + c) * kLocRow + j], win[c][j], s);
        scratch[i * kT2AttnTile + tl] = s;  // features at or past F are 0
      }
    }
    const int t = t0 + tl;
    float pv[kT2MaxA / kAttnSplit];
#pragma unroll
    for (int j = 0; j < kT2MaxA / kAttnSplit; ++j) {
      const int r = sp + kAttnSplit * j;
      pv[j] = (r < A && t < len) ? pinp[(size_t)r * T + t] : 0.f;
    }
    __syncthreads();
    float fr[kT2MaxF];
#pragma unroll
    for (int i = 0; i < kT2MaxF; ++i) fr[i] = scratch[i * kT2AttnTile + tl];
    float pe = 0.f;
#pragma unroll
    for (int j = 0; j < kT2MaxA / kAttnSplit; ++j) {
      const int r = sp + kAttnSplit * j;
      if (r < A) {
        float s = pq[r] + pv[j];
#pragma unroll
        for (int i = 0; i < kT2MaxF; ++i) s = fmaf(wd[r * kT2MaxF + i], fr[i], s);
        pe = fmaf(vv[r], tanhf(s), pe);
      }
    }
    ep[sp][tl] = pe;
    __syncthreads();
    if (sp == 0 && t < T) {
      float p = 0.f;  // masked positions: probability exactly 0
      if (t < len) {
        float e = vb;
#pragma unroll
        for (int q = 0; q < kAttnSplit; ++q) e += ep[q][tl];
        if (a.softmax) {
          p = e;
          lmax = fmaxf(lmax, e);
        } else {
          p = sigmoidf_(e);
          lsum += p;
        }
      }
      as[t] = p;
    }
  }
  if (a.softmax) {
    const float m = block_max(lmax, red);
    for (int t = tid; t < T; t += kWgThreads) {
      float p = 0.f;
      if (t < len) {
        p = expf(as[t] - m);
        lsum += p;
      }
      as[t] = p;
    }
  }
  const float sum = block_sum(lsum, red);
  const float inv = sum > 0.f ? 1.f / sum : 0.f;
  float* align = a.align + ((size_t)b * a.S + a.step) * T;
  for (int t = tid; t < T; t += kWgThreads) {
    const float p = as[t] * inv;
    as[t] = p;
    a.aw_out[(size_t)b * T + t] = p;
    a.awc_out[(size_t)b * T + t] = awc_in[t] + p;
    align[t] = p;
  }
  const float* inp = a.inputs + (size_t)b * T * a.D;
  const int dl = tid & 255, ts = tid >> 8;
  for (int d0 = 0; d0 < a.D; d0 += 256) {
    __syncthreads();  // as[] is complete; the previous parts are consumed
    const int d = d0 + dl;
    float s = 0.f;
    if (d < a.D) {
#pragma unroll 16
      for (int t = ts; t < len; t += 4) s = fmaf(as[t], inp[(size_t)t * a.D + d], s);
    }
    scratch[ts * 256 + dl] = s;
    __syncthreads();
    if (ts == 0 && d < a.D)
      a.ctx[(size_t)d * a.BT + b] = ((scratch[dl] + scratch[256 + dl]) + scratch[512 + dl]) + scratch[768 + dl];
  }
}

// ---------------------------------------------------------------------------- stop, bookkeeping, next prenet
// One workgroup of 1024 threads per utterance: it owns the whole projected row of its utterance, so the
// next step's prenet needs no other workgroup.  A prenet layer: thread (output p, part ks of 4) sums its
// interleaved quarter of the inputs; the parts are added in order.
__device__ __forceinline__ void prenet_layer(const float* wt, const float* x, int n_in, int P, float* part, float* y,
                                             int64_t y_stride) {
  const int tid = threadIdx.x, pl = tid & 255, ks = tid >> 8;
  for (int p0 = 0; p0 < P; p0 += 256) {
    const int p = p0 + pl;
    float v = 0.f;
    if (p < P) {
#pragma unroll 8
      for (int k = ks; k < n_in; k += 4) v = fmaf(wt[(size_t)k * P + p], x[k], v);
    }
    __syncthreads();
    part[ks * 256 + pl] = v;
    __syncthreads();
    if (ks == 0 && p < P)
      y[(size_t)p * y_stride] = fmaxf(((part[pl] + part[256 + pl]) + part[512 + pl]) + part[768 + pl], 0.f);
  }
  __syncthreads();
}

__global__ __launch_bounds__(kWgThreads) void t2_stop_prenet_kernel(T2StopArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (a.done[b]) return;
  __shared__ float outs[kT2MaxOut];
  __shared__ float h0[kT2MaxP];
  __shared__ float red[kWgThreads];
  const int Cr = a.C * a.r, Q = a.Q, P = a.P;
  const float* row = a.dec_out + ((size_t)b * a.S + a.step) * Cr;
  for (int i = tid; i < Cr; i += kWgThreads) outs[i] = row[i];
  __syncthreads();
  float s = 0.f;
  for (int k = tid; k < Q; k += kWgThreads) s = fmaf(a.stop_w[k], a.hd[(size_t)k * a.BT + b], s);
  for (int j = tid; j < Cr; j += kWgThreads) s = fmaf(a.stop_w[Q + j], outs[j], s);
  const float stop = sigmoidf_(block_sum(s, red) + a.stop_b[0]);
  __syncthreads();
  // prenet of the last frame of this step: relu(W1 relu(W0 memory)), no bias
  prenet_layer(a.w0t, outs + (a.r - 1) * a.C, a.C, P, red, h0, 1);
  prenet_layer(a.w1t, h0, P, P, red, a.prenet + b, a.BT);
  if (tid == 0) {
    a.stop_tokens[(size_t)b * a.S + a.step] = stop;
    if ((a.step >= 1 && stop > a.threshold) || a.step + 1 >= a.max_steps) {
      a.done[b] = 1;
      a.steps[b] = a.step + 1;
      if (atomicAdd(&a.counters[0], 1) + 1 == a.B) a.counters[1] = 1;
    }
  }
}

// ---------------------------------------------------------------------------- glue
__global__ void t2_embed_kernel(const int64_t* tok, const float* emb, float* x, int E, int T, int num_chars) {
  const int b = blockIdx.z, e = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  int64_t id = tok[(size_t)b * T + t];
  if (id < 0 || id >= num_chars) id = 0;  // out of range: the padding row
  x[((size_t)b * E + e) * T + t] = emb[(size_t)id * E + e];
}

__global__ void t2_speaker_kernel(const int64_t* ids, const float* table, int num_speakers, const float* vec,
                                  float* inputs, int T, int E, int W) {
  const int b = blockIdx.y, t = blockIdx.x;
  const float* src = vec + (size_t)b * W;
  if (ids) {
    int64_t id = ids[b];
    if (id < 0 || id >= num_speakers) id = 0;
    src = table + (size_t)id * W;
  }
  for (int j = threadIdx.x; j < W; j += blockDim.x) inputs[((size_t)b * T + t) * (E + W) + E + j] = src[j];
}

__global__ void t2_processed_inputs_kernel(const float* inputs, const float* wt, float* pinp, int T, int D, int A) {
  const int b = blockIdx.y, t = blockIdx.x;
  const float* row = inputs + ((size_t)b * T + t) * D;
  for (int r = threadIdx.x; r < A; r += blockDim.x) {
    float s = 0.f;
    for (int d = 0; d < D; ++d) s = fmaf(wt[(size_t)d * A + r], row[d], s);
    pinp[((size_t)b * A + r) * T + t] = s;
  }
}

__global__ void t2_to_planes_kernel(const float* dec, const int* steps, int r, float* x, float* mask, int C, int L,
                                    int64_t dec_bstride) {
  const int b = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= L) return;
  const float* src = dec + (size_t)b * dec_bstride + (size_t)t * C;
  for (int c = 0; c < C; ++c) x[((size_t)b * C + c) * L + t] = src[c];
  mask[(size_t)b * L + t] = t < steps[b] * r ? 1.f : 0.f;
}

__global__ void t2_tanh_kernel(float* x, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] = tanhf(x[i]);
}

__global__ void t2_residual_out_kernel(const float* dec, const float* post, const float* mask, float* out, int C, int L,
                                       int64_t dec_bstride) {
  const int b = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= L) return;
  const float m = mask[(size_t)b * L + t];
  const float* src = dec + (size_t)b * dec_bstride + (size_t)t * C;
  float* dst = out + ((size_t)b * L + t) * C;
  for (int c = 0; c < C; ++c) dst[c] = (src[c] + post[((size_t)b * C + c) * L + t]) * m;
}

__global__ void t2_transpose_kernel(const float* src, float* dst, int rows, int cols, int lds, int ldd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (c < cols) dst[(size_t)c * ldd + r] = src[(size_t)r * lds + c];
}

}  // namespace

int skinny_batch_tile(int B) {
  int bt = 1;
  while (bt < B) bt *= 2;
  return bt;
}

void launch_skinny(const SkinnyArgs& a, hipStream_t s) {
  TTS_REQUIRE(a.B >= 1 && a.B <= kSkinnyMaxBatch, 3,
              "batch must lie in [1, " + std::to_string(kSkinnyMaxBatch) + "]");
  TTS_REQUIRE(a.BT == skinny_batch_tile(a.B) && a.Kp == skinny_kp(a.K) && a.K == a.n[0] + a.n[1] + a.n[2], 2,
              "internal: skinny product arguments");
  TTS_REQUIRE(!a.lstm || (a.H >= kLstmUnitBlock && a.H % kLstmUnitBlock == 0), 3,
              "LSTM: the hidden size must be a multiple of " + std::to_string(kLstmUnitBlock));
  switch (a.BT) {
    case 1: launch_skinny_bt<1>(a, s); break;
    case 2: launch_skinny_bt<2>(a, s); break;
    case 4: launch_skinny_bt<4>(a, s); break;
    case 8: launch_skinny_bt<8>(a, s); break;
    case 16: launch_skinny_bt<16>(a, s); break;
    default: launch_skinny_bt<32>(a, s); break;
  }
  TTS_HIP_CHECK(hipGetLastError());
}

void launch_t2_attention(const T2AttnArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(t2_attention_kernel, dim3(a.B), dim3(kWgThreads), 0, s, a);
  TTS_HIP_CHECK(hipGetLastError());
}

void launch_t2_stop_prenet(const T2StopArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(t2_stop_prenet_kernel, dim3(a.B), dim3(kWgThreads), 0, s, a);
  TTS_HIP_CHECK(hipGetLastError());
}

void launch_t2_embed(const int64_t* tok, const float* emb, float* x, int B, int E, int T, int num_chars, hipStream_t s) {
  hipLaunchKernelGGL(t2_embed_kernel, dim3(ceil_div(T, 64), E, B), dim3(64), 0, s, tok, emb, x, E, T, num_chars);
  TTS_HIP_CHECK(hipGetLastError());
}

void launch_t2_speaker(const int64_t* ids, const float* table, int num_speakers, const float* vec, float* inputs, int B,
                       int T, int E, int W, hipStream_t s) {
  hipLaunchKernelGGL(t2_speaker_kernel, dim3(T, B), dim3(64), 0, s, ids, table, num_speakers, vec, inputs, T, E, W);
  TTS_HIP_CHECK(hipGetLastError());
}

void launch_t2_processed_inputs(const float* inputs, const float* wt, float* pinp, int B, int T, int D, int A,
                                hipStream_t s) {
  hipLaunchKernelGGL(t2_processed_inputs_kernel, dim3(T, B), dim3(128), 0, s, inputs, wt, pinp, T, D, A);
  TTS_HIP_CHECK(hipGetLastError());
}

void launch_t2_to_planes(const float* dec, const int* steps, int r, float* x, float* mask, int B, int C, int L,
                         int64_t dec_bstride, hipStream_t s) {
  hipLaunchKernelGGL(t2_to_planes_kernel, dim3(ceil_div(L, 64), B), dim3(64), 0, s, dec, steps, r, x, mask, C, L,
                     dec_bstride);
  TTS_HIP_CHECK(hipGetLastError());
}

void launch_t2_tanh(float* x, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(t2_tanh_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n);
  TTS_HIP_CHECK(hipGetLastError());
}

void launch_t2_residual_out(const float* dec, const float* post, const float* mask, float* out, int B, int C, int L,
                            int64_t dec_bstride, hipStream_t s) {
  hipLaunchKernelGGL(t2_residual_out_kernel, dim3(ceil_div(L, 64), B), dim3(64), 0, s, dec, post, mask, out, C, L,
                     dec_bstride);
  TTS_HIP_CHECK(hipGetLastError());
}

void launch_t2_transpose(const float* src, float* dst, int rows, int cols, int lds, int ldd, hipStream_t s) {
  hipLaunchKernelGGL(t2_transpose_kernel, dim3(ceil_div(cols, 64), rows), dim3(64), 0, s, src, dst, rows, cols, lds,
                     ldd);
  TTS_HIP_CHECK(hipGetLastError());
}

}  // namespace tts
