// XTTS GPT kernels: the decode-step product with a LayerNorm prologue and its epilogues, single-query
// attention over the KV cache, the logits -> token step with its bookkeeping, and the input rows.
//
// A step is a chain of launches on one stream; every dependency is a kernel boundary, no kernel waits
// on another workgroup, and every loop bound is a launch argument.  Utterances whose skip[b] / done[b]
// is set are left untouched by every kernel, so steps enqueued past the last end change nothing.
// Every reduction runs in an order fixed by the sizes alone: column b of a batch is bitwise the
// column of a batch of one, and a repeated call returns the same bits.
#include "xtts_gpt.hpp"

#include <climits>

namespace tts {

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ float gelu_new(float v) {
  return 0.5f * v * (1.f + tanhf(0.7978845608028654f * (v + 0.044715f * v * v * v)));
}

// ---------------------------------------------------------------------------- decode-step product
// The skinny product of kernels_tacotron2.hip (16 packed rows per workgroup, thread (u, ks) streams
// the rows 4u .. 4u + 3 of columns ks, ks + 64, ..., the 64 k-slices summed in a fixed order) on one
// input vector, which passes through up to two LayerNorms while it is staged.  Every workgroup
// recomputes the statistics of all BT columns: 64 slices of k per column whatever BT is, summed in
// order, the variance from the centred values.
constexpr int kChunkFloats = 8192;
constexpr int kLnSlices = 64;

template <int BT, class F>
__device__ __forceinline__ void ln_stats(F&& val, int K, float* part, float* mean, float* rstd) {
  const int tid = threadIdx.x;
  for (int pass = 0; pass < 2; ++pass) {
    for (int p = tid; p < kLnSlices * BT; p += 256) {
      const int sl = p / BT, b = p % BT;
      const float mu = pass ? mean[b] : 0.f;
      float s = 0.f;
      for (int k = sl; k < K; k += kLnSlices) {
        const float v = val(k, b) - mu;
        s += pass ? v * v : v;
      }
      part[p] = s;
    }
    __syncthreads();
    if (tid < BT) {
      float s = 0.f;
      for (int q = 0; q < kLnSlices; ++q) s += part[q * BT + tid];
      if (pass) rstd[tid] = 1.f / sqrtf(s / (float)K + kGptLnEps);
      else mean[tid] = s / (float)K;
    }
    __syncthreads();
  }
}

template <int BT, bool BF16W>
__global__ __launch_bounds__(256) void gpt_skinny_kernel(GptSkinnyArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[kChunkFloats];
  __shared__ float mean[2][kGptMaxBatch], rstd[2][kGptMaxBatch];
  const int tid = threadIdx.x, u = tid & 3, ks = tid >> 2, rb = blockIdx.x;
  const int nln = a.nln;
  auto v0 = [&](int k, int b) { return a.x[(size_t)k * BT + b]; };
  auto v1 = [&](int k, int b) { return fmaf((v0(k, b) - mean[0][b]) * rstd[0][b], a.ln_g[0][k], a.ln_b[0][k]); };
  auto v2 = [&](int k, int b) { return fmaf((v1(k, b) - mean[1][b]) * rstd[1][b], a.ln_g[1][k], a.ln_b[1][k]); };
  if (nln >= 1) ln_stats<BT>(v0, a.K, smem, mean[0], rstd[0]);
  if (nln >= 2) ln_stats<BT>(v1, a.K, smem, mean[1], rstd[1]);
  if (a.lat && rb == 0) {
    for (int i = tid; i < a.K * BT; i += 256) {
      const int k = i / BT, b = i % BT;
      if (b >= a.B || (a.skip && a.skip[b])) continue;
      if (a.lat_n && a.lat_step >= a.lat_n[b] - 2) continue;
      a.lat[(size_t)b * a.ld_lat + k] = nln == 2 ? v2(k, b) : (nln == 1 ? v1(k, b) : v0(k, b));
    }
  }
  if (a.lat_only) return;  // the whole (single) workgroup

  float acc[4][BT];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int b = 0; b < BT; ++b) acc[g][b] = 0.f;
  const int KC = kChunkFloats / BT;  // a multiple of 64
  const size_t wbase = (size_t)rb * a.Kp * kSkinnyRows;
  for (int k0 = 0; k0 < a.Kp; k0 += KC) {
    const int kc = min(KC, a.Kp - k0);
    __syncthreads();
    for (int i = tid; i < kc * BT; i += 256) {
      const int k = k0 + i / BT, b = i % BT;
      float v = 0.f;
      if (k < a.K) v = nln == 2 ? v2(k, b) : (nln == 1 ? v1(k, b) : v0(k, b));
      smem[i] = v;
    }
    __syncthreads();
#pragma clang loop unroll_count(BT <= 8 ? 8 : 4)
    for (int kk = ks; kk < kc; kk += 64) {
      float w[4];
      if (BF16W) {
        const uint2 p = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(a.w) + wbase +
                                                        (size_t)(k0 + kk) * kSkinnyRows + 4 * u);
        w[0] = __uint_as_float(p.x << 16);
        w[1] = __uint_as_float(p.x & 0xffff0000u);
        w[2] = __uint_as_float(p.y << 16);
        w[3] = __uint_as_float(p.y & 0xffff0000u);
      } else {
        const float4 p = *reinterpret_cast<const float4*>(static_cast<const float*>(a.w) + wbase +
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
  const int u2 = tid / BT, b2 = tid % BT;
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
  if (a.skip && a.skip[b]) return;
  const int pos = (a.base ? a.base[b] : 0) + a.off;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int row = rb * kSkinnyRows + 4 * u2 + g;
    if (row >= a.R) continue;
    const float v = tot[g] + a.bias[row];
    if (a.epi == kGptEpiQkv) {
      const int sec = row / a.E, c = row - sec * a.E;
      if (sec == 0) a.q[(size_t)b * a.E + c] = v;
      else if (pos >= 0 && pos < a.cap) (sec == 1 ? a.kc : a.vc)[((size_t)b * a.cap + pos) * a.E + c] = v;
    } else if (a.epi == kGptEpiResidual) {
      a.out[(size_t)row * BT + b] += v;
    } else if (a.epi == kGptEpiGelu) {
      a.out[(size_t)row * BT + b] = gelu_new(v);
    } else {
      a.logits[(size_t)b * a.ld_logits + row] = v;
      if (a.logits2) a.logits2[(size_t)b * a.ld_logits2 + row] = v;
    }
  }
}

template <int BT>
void launch_gpt_skinny_bt(const GptSkinnyArgs& a, hipStream_t s) {
  const dim3 grid(a.lat_only ? 1 : ceil_div(a.R, kSkinnyRows));
  if (a.bf16) hipLaunchKernelGGL((gpt_skinny_kernel<BT, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((gpt_skinny_kernel<BT, false>), grid, dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------- decode attention
// One workgroup of kGptAttnWaves waves per (head, utterance).  Wave w takes the key tiles w, w + 8, ...
// of 64 keys: a lane scores one key (q . k in d order), the wave keeps a running (max, sum, output)
// with the output's dk columns over the lanes, and the waves' states are merged in wave order.
template <int DK>
__global__ __launch_bounds__(64 * kGptAttnWaves) void gpt_decode_attn_kernel(GptAttnArgs a) {
  constexpr int R = DK > 64 ? DK / 64 : 1;
  constexpr int kVB = 16;  // V rows in flight per lane; divides kGptAttnTile
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (a.skip && a.skip[b]) return;
  const int len = min(a.cap, (a.base ? a.base[b] : 0) + a.off + 1);
  if (len <= 0) return;
  __shared__ __attribute__((aligned(16))) float qs[DK];
  __shared__ float wm[kGptAttnWaves], wl[kGptAttnWaves], wo[kGptAttnWaves][DK];
  if (tid < DK) qs[tid] = a.q[(size_t)b * a.E + h * DK + tid];
  __syncthreads();
  const float scale = 1.f / sqrtf((float)DK);
  const float* K = a.kc + (size_t)b * a.cap * a.E + h * DK;
  const float* V = a.vc + (size_t)b * a.cap * a.E + h * DK;
  float m = -INFINITY, l = 0.f, o[R];
#pragma unroll
  for (int r = 0; r < R; ++r) o[r] = 0.f;
  for (int j0 = wave * kGptAttnTile; j0 < len; j0 += kGptAttnTile * kGptAttnWaves) {
    const int j = j0 + lane;
    const bool valid = j < len;
    float sc = -INFINITY;
    if (valid) {
      const float4* kr = reinterpret_cast<const float4*>(K + (size_t)j * a.E);
      float acc = 0.f;
#pragma unroll 8
      for (int d = 0; d < DK / 4; ++d) {
        const float4 kv = kr[d];
        acc = fmaf(kv.x, qs[4 * d], acc);
        acc = fmaf(kv.y, qs[4 * d + 1], acc);
        acc = fmaf(kv.z, qs[4 * d + 2], acc);
        acc = fmaf(kv.w, qs[4 * d + 3], acc);
      }
      sc = acc * scale;
    }
    float mt = sc;
    for (int x = 32; x > 0; x >>= 1) mt = fmaxf(mt, __shfl_xor(mt, x, 64));
    const float mn = fmaxf(m, mt);
    const float p = valid ? expf(sc - mn) : 0.f;
    float lt = p;
    for (int x = 32; x > 0; x >>= 1) lt += __shfl_xor(lt, x, 64);
    const float alpha = expf(m - mn);  // 0 on the first tile (m = -inf)
    l = fmaf(l, alpha, lt);
    m = mn;
#pragma unroll
    for (int r = 0; r < R; ++r) o[r] *= alpha;
    // the V rows of kVB keys are loaded before any of them is used: the loads are independent, and
    // one at a time each would pay the whole memory latency (the sum's order stays key by key)
    const int nv = min(kGptAttnTile, len - j0);
    for (int jj0 = 0; jj0 < nv; jj0 += kVB) {
      float vv[R][kVB];
#pragma unroll
      for (int u = 0; u < kVB; ++u)
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int d = lane + 64 * r;
          vv[r][u] = (jj0 + u < nv && d < DK) ? V[(size_t)(j0 + jj0 + u) * a.E + d] : 0.f;
        }
#pragma unroll
      for (int u = 0; u < kVB; ++u) {
        const float pj = __shfl(p, jj0 + u, 64);  // keys at or past nv: p = 0
#pragma unroll
        for (int r = 0; r < R; ++r) o[r] = fmaf(pj, vv[r][u], o[r]);
      }
    }
  }
  if (lane == 0) {
    wm[wave] = m;
    wl[wave] = l;
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (lane + 64 * r < DK) wo[wave][lane + 64 * r] = o[r];
  __syncthreads();
  if (tid < DK) {
    float M = wm[0];
    for (int w = 1; w < kGptAttnWaves; ++w) M = fmaxf(M, wm[w]);
    float L = 0.f, O = 0.f;
    for (int w = 0; w < kGptAttnWaves; ++w) {
      const float f = expf(wm[w] - M);  // a wave without a tile: exp(-inf) = 0
      L = fmaf(wl[w], f, L);
      O = fmaf(wo[w][tid], f, O);
    }
    a.out[(size_t)(h * DK + tid) * a.BT + b] = O / L;
  }
}

// ---------------------------------------------------------------------------- logits -> token
// One workgroup of 1024 threads per utterance.  The processors in the HF order: repetition penalty,
// temperature, top-k, top-p, then a draw by inverse CDF in token order.  Probabilities are
// exp(l - max) as 2^-40 fixed point in 64-bit integers, so every sum of them is exact and every
// selection is a radix select over integer histograms: the k-th largest logit (mass 1 per token), the
// top-p boundary (probability mass in ascending logit order) and the drawn token (mass in id order).
constexpr int kSampleThreads = 1024;

__device__ __forceinline__ unsigned float_key(float v) {  // unsigned order = float order
  const unsigned bits = __float_as_uint(v + 0.f);         // -0 -> +0
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

__device__ __forceinline__ u64 shfl_up64(u64 v, int d) {
  const int lo = __shfl_up((int)(unsigned)v, d, 64), hi = __shfl_up((int)(unsigned)(v >> 32), d, 64);
  return ((u64)(unsigned)hi << 32) | (unsigned)lo;
}

struct SelectShared {
  u64 hist[256];
  u64 below;
  int bin;
};

// The smallest key kappa with mass{i : key(i) <= kappa} > thr, or found = false when the whole mass is
// <= thr.  Four passes over the key bytes, most significant first.
template <class KeyF, class MassF>
__device__ unsigned radix_select(int n, KeyF&& key, MassF&& mass, u64 thr, SelectShared& sh, bool& found) {
  const int tid = threadIdx.x;
  unsigned prefix = 0;
  u64 below = 0;
  found = true;
  for (int shift = 24; shift >= 0; shift -= 8) {
    const unsigned himask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
    if (tid < 256) sh.hist[tid] = 0;
    if (tid == 0) sh.bin = -1;
    __syncthreads();
    for (int i = tid; i < n; i += kSampleThreads) {
      const unsigned k = key(i);
      if ((k & himask) != prefix) continue;
      const u64 mv = mass(i);
      if (mv) atomicAdd(&sh.hist[(k >> shift) & 255u], mv);  // integer sums: exact in any order
    }
    __syncthreads();
    if (tid < 64) {  // the first wave scans the 256 bins, four per lane
      u64 hv[4], loc = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        hv[t] = sh.hist[4 * tid + t];
        loc += hv[t];
      }
      u64 incl = loc;
      for (int d = 1; d < 64; d <<= 1) {
        const u64 t = shfl_up64(incl, d);
        if (tid >= d) incl += t;
      }
      const u64 hit = __ballot(below + incl > thr);
      if (hit != 0 && tid == __ffsll((long long)hit) - 1) {
        u64 c = below + incl - loc;
        int t = 0;
        while (t < 3 && c + hv[t] <= thr) c += hv[t++];
        sh.bin = 4 * tid + t;
        sh.below = c;
      }
    }
    __syncthreads();
    const int bin = sh.bin;
    if (bin < 0) {  // only on the first pass: below a chosen bin the mass always exceeds thr
      found = false;
      __syncthreads();
      return 0xffffffffu;
    }
    below = sh.below;
    prefix |= (unsigned)bin << shift;
    __syncthreads();
  }
  return prefix;
}

__device__ __forceinline__ u64 block_sum64(u64 v, u64* slot) {
  __syncthreads();
  if (threadIdx.x == 0) *slot = 0;
  __syncthreads();
  if (v) atomicAdd(slot, v);
  __syncthreads();
  return *slot;
}

__global__ __launch_bounds__(kSampleThreads) void gpt_sample_kernel(GptSampleArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, V = a.V;
  if (a.done && a.done[b]) return;
  __shared__ float lg[kGptMaxVocab];
  __shared__ unsigned char pen[kGptMaxVocab];
  __shared__ u64 red[kSampleThreads];
  __shared__ SelectShared sel;
  __shared__ u64 slot;
  __shared__ int tok_sh;
  int* codes = a.codes + (size_t)b * a.S;

  // 1. repetition penalty over {1, start_audio} and the codes so far
  for (int i = tid; i < V; i += kSampleThreads) pen[i] = (i == 1 || i == a.start_audio) ? 1 : 0;
  __syncthreads();
  for (int s = tid; s < a.step; s += kSampleThreads) {
    const int c = codes[s];
    if (c >= 0 && c < V) pen[c] = 1;
  }
  __syncthreads();
  for (int i = tid; i < V; i += kSampleThreads) {
    float v = a.logits[(size_t)b * V + i];
    if (pen[i]) v = v < 0.f ? v * a.penalty : v / a.penalty;
    if (a.u) v = v / a.temperature;  // 2.
    lg[i] = v;
  }
  __syncthreads();
  // the largest logit, the lowest id on ties
  u64 best = 0;
  for (int i = tid; i < V; i += kSampleThreads) {
    const u64 pk = ((u64)float_key(lg[i]) << 32) | (u64)(0xffffffffu - (unsigned)i);
    best = pk > best ? pk : best;
  }
  red[tid] = best;
  __syncthreads();
  for (int s = kSampleThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid + s] > red[tid] ? red[tid + s] : red[tid];
    __syncthreads();
  }
  const int imax = (int)(0xffffffffu - (unsigned)(red[0] & 0xffffffffu));
  const unsigned kmax = (unsigned)(red[0] >> 32);
  int tok = imax;

  if (a.u) {
    const float lmax = lg[imax];
    bool found;
    // 3. top-k: tokens below the k-th largest logit go
    if (a.top_k > 0 && a.top_k < V) {
      const unsigned kk = radix_select(
          V, [&](int i) { return float_key(lg[i]); }, [&](int) { return (u64)1; }, (u64)(V - a.top_k), sel, found);
      for (int i = tid; i < V; i += kSampleThreads)
        if (float_key(lg[i]) < kk) lg[i] = -INFINITY;
      __syncthreads();
    }
    auto massf = [&](int i) { return (u64)((double)expf(lg[i] - lmax) * 1099511627776.0); };  // 2^40
    // 4. top-p: in ascending order, tokens whose cumulative probability is <= 1 - top_p go
    if (a.top_p < 1.f) {
      u64 loc = 0;
      for (int i = tid; i < V; i += kSampleThreads) loc += massf(i);
      const u64 total = block_sum64(loc, &slot);
      const u64 thr = (u64)((double)total * (1.0 - (double)a.top_p));
      const unsigned kp = radix_select(V, [&](int i) { return float_key(lg[i]); }, massf, thr, sel, found);
      for (int i = tid; i < V; i += kSampleThreads) {
        const unsigned k = float_key(lg[i]);
        if (k < kp && k != kmax) lg[i] = -INFINITY;  // the largest always stays
      }
      __syncthreads();
    }
    // 5, 6. softmax over what is left, inverse CDF in token order
    u64 loc = 0;
    for (int i = tid; i < V; i += kSampleThreads) loc += massf(i);
    const u64 Z = block_sum64(loc, &slot);
    const float uv = a.u[(size_t)b * a.ldu + a.u_off];
    u64 target = (u64)((double)uv * (double)Z);
    if (target >= Z) target = Z - 1;
    const unsigned kt = radix_select(V, [&](int i) { return (unsigned)i; }, massf, target, sel, found);
    tok = found ? (int)kt : imax;
  }

  if (tid == 0) {
    codes[a.step] = tok;
    int ended = 0;
    if (a.done && (tok == a.stop_audio || a.step + 1 >= a.max_steps)) {
      a.done[b] = 1;
      a.n[b] = a.step + 1;
      if (atomicAdd(&a.counters[0], 1) + 1 == a.B) a.counters[1] = 1;
      ended = 1;
    }
    tok_sh = ended ? -1 : tok;
  }
  __syncthreads();
  if (!a.mel_emb || tok_sh < 0) return;
  const float* e = a.mel_emb + (size_t)tok_sh * a.E;
  const float* pp = a.mel_pos + (size_t)(a.step + 1) * a.E;
  for (int k = tid; k < a.E; k += kSampleThreads) a.x[(size_t)k * a.BT + b] = e[k] + pp[k];
}

// ---------------------------------------------------------------------------- input rows
__global__ __launch_bounds__(256) void gpt_embed_kernel(GptEmbedArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, t = a.t, E = a.E;
  const float *row0, *row1 = nullptr;
  if (!a.mel) {
    const int L = a.text_len ? (int)min((int64_t)a.T, max((int64_t)0, a.text_len[b])) : a.T;
    const int plen = a.P + L + 2;
    if (tid == 0) {
      a.plen[b] = plen;
      a.skip[b] = t >= plen;
    }
    if (t >= plen) return;
    if (t < a.P) {
      row0 = a.cond + ((size_t)b * a.P + t) * E;
    } else {
      const int i = t - a.P;
      int64_t tok = i == 0 ? a.start_text : (i == L + 1 ? a.stop_text : a.text[(size_t)b * a.T + i - 1]);
      tok = min((int64_t)a.n_text - 1, max((int64_t)0, tok));
      row0 = a.text_emb + (size_t)tok * E;
      row1 = a.text_pos + (size_t)i * E;
    }
  } else {
    const int nb = a.codes ? min(a.S, max(0, a.n[b])) : 0;
    const bool none = a.codes && t >= nb + 2;
    if (tid == 0 && a.skip) a.skip[b] = none;
    if (none) return;
    int tok = t == 0 ? a.start_audio : (t <= nb ? a.codes[(size_t)b * a.S + t - 1] : a.stop_audio);
    tok = min(a.n_audio - 1, max(0, tok));
    row0 = a.mel_emb + (size_t)tok * E;
    row1 = a.mel_pos + (size_t)t * E;
  }
  for (int k = tid; k < E; k += 256) a.x[(size_t)k * a.BT + b] = row0[k] + (row1 ? row1[k] : 0.f);
}

// ---------------------------------------------------------------------------- whole-sequence pass
// Glue of the prefill and the latent pass on the conv path: planes are [B][C][T], position t of
// utterance b being row t of its own sequence [prefix | mel rows], zeros at and past its length.
constexpr int kSeqT = 64;  // positions per workgroup (the lanes), 4 channel slices over the waves

__global__ __launch_bounds__(256) void gpt_seq_embed_kernel(GptSeqEmbedArgs a) {
  const int b = blockIdx.y, tid = threadIdx.x, t = blockIdx.x * kSeqT + (tid & 63), cs = tid >> 6, E = a.E;
  int plen;
  if (!a.from_pre) {
    const int L = a.text_len ? (int)min((int64_t)a.Ttext, max((int64_t)0, a.text_len[b])) : a.Ttext;
    plen = a.P + L + 2;
  } else {
    plen = a.plen[b];
  }
  const int nb = a.codes ? min(a.S, max(0, a.n[b])) : 0;
  const int total = plen + (a.codes ? min(a.rows, nb + 2) : 0);
  if (blockIdx.x == 0 && tid == 0) {
    a.plen[b] = plen;
    a.klen[b] = total;
  }
  if (t >= a.T) return;
  const float *row0 = nullptr, *row1 = nullptr;
  if (t < plen) {
    if (a.from_pre) {
      row0 = a.pre + ((size_t)b * a.pre_rows + t) * E;
    } else if (t < a.P) {
      row0 = a.cond + ((size_t)b * a.P + t) * E;
    } else {
      const int i = t - a.P, L = plen - a.P - 2;
      int64_t tok = i == 0 ? a.start_text : (i == L + 1 ? a.stop_text : a.text[(size_t)b * a.Ttext + i - 1]);
      tok = min((int64_t)a.n_text - 1, max((int64_t)0, tok));
      row0 = a.text_emb + (size_t)tok * E;
      row1 = a.text_pos + (size_t)i * E;
    }
  } else if (t < total) {
    const int s = t - plen;
    int tok = s == 0 ? a.start_audio : (s <= nb ? a.codes[(size_t)b * a.S + s - 1] : a.stop_audio);
    tok = min(a.n_audio - 1, max(0, tok));
    row0 = a.mel_emb + (size_t)tok * E;
    row1 = a.mel_pos + (size_t)s * E;
  }
  const bool save = !a.from_pre && a.pre && t < plen && t < a.pre_rows;
  for (int k = cs; k < E; k += 4) {
    const float v = row0 ? row0[k] + (row1 ? row1[k] : 0.f) : 0.f;
    a.x[((size_t)b * E + k) * a.T + t] = v;
    if (save) a.pre[((size_t)b * a.pre_rows + t) * E + k] = v;
  }
}

// y[b][c][t] = LayerNorm over c of x[b][.][t]; a position's channels in 4 interleaved slices summed in
// order, the variance from the centred values; y may be x
__global__ __launch_bounds__(256) void gpt_seq_layernorm_kernel(const float* x, const float* gamma, const float* beta,
                                                                float* y, int C, int T) {
  __shared__ float part[4][kSeqT], mean[kSeqT], rstd[kSeqT];
  const int b = blockIdx.y, tid = threadIdx.x, tl = tid & 63, t = blockIdx.x * kSeqT + tl, cs = tid >> 6;
  const float* xb = x + (size_t)b * C * T;
  float* yb = y + (size_t)b * C * T;
  const bool in = t < T;
  for (int pass = 0; pass < 2; ++pass) {
    const float mu = pass ? mean[tl] : 0.f;
    float s = 0.f;
    if (in)
      for (int c = cs; c < C; c += 4) {
        const float v = xb[(size_t)c * T + t] - mu;
        s += pass ? v * v : v;
      }
    part[cs][tl] = s;
    __syncthreads();
    if (tid < kSeqT) {
      const float tot = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
      if (pass) rstd[tid] = 1.f / sqrtf(tot / (float)C + kGptLnEps);
      else mean[tid] = tot / (float)C;
    }
    __syncthreads();
  }
  if (!in) return;
  for (int c = cs; c < C; c += 4)
    yb[(size_t)c * T + t] = fmaf((xb[(size_t)c * T + t] - mean[tl]) * rstd[tl], gamma[c], beta[c]);
}

__global__ __launch_bounds__(256) void gpt_seq_gelu_kernel(float* x, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = gelu_new(x[i]);
}

// cache rows from the planes: kc[b][t][c] = qkv[b][E + c][t], vc[b][t][c] = qkv[b][2E + c][t], t < klen[b]
__global__ __launch_bounds__(256) void gpt_seq_kv_kernel(const float* qkv, const int64_t* klen, float* kc, float* vc,
                                                         int E, int T, int cap) {
  __shared__ float tile[64][65];
  const int b = blockIdx.z, t0 = blockIdx.x * 64, c0 = blockIdx.y * 64, tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  const int len = (int)min((int64_t)min(T, cap), klen[b]);
  for (int sec = 1; sec <= 2; ++sec) {
    __syncthreads();
    for (int r = w; r < 64; r += 4)  // channel c0 + r, position t0 + l
      tile[r][l] = (c0 + r < E && t0 + l < T) ? qkv[((size_t)b * 3 * E + (size_t)sec * E + c0 + r) * T + t0 + l] : 0.f;
    __syncthreads();
    float* dst = sec == 1 ? kc : vc;
    for (int r = w; r < 64; r += 4)  // position t0 + r, channel c0 + l
      if (t0 + r < len && c0 + l < E) dst[((size_t)b * cap + t0 + r) * E + c0 + l] = tile[l][r];
  }
}

// the hidden state of mel position s as a step input: x[k][b] = h[b][k][plen_b + s]
__global__ __launch_bounds__(256) void gpt_seq_column_kernel(const float* h, const int* plen, const int* n, int S, int s,
                                                             int E, int T, int BT, float* x, int* skip) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nb = min(S, max(0, n[b])), t = plen[b] + s;
  const bool none = s >= nb + 2 || t >= T;
  if (tid == 0) skip[b] = none;
  if (none) return;
  for (int k = tid; k < E; k += 256) x[(size_t)k * BT + b] = h[((size_t)b * E + k) * T + t];
}

}  // namespace

void launch_gpt_seq_embed(const GptSeqEmbedArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(gpt_seq_embed_kernel, dim3(ceil_div(a.T, kSeqT), a.B), dim3(256), 0, s, a);
  TTS_HIP_CHECK(hipGetLastError());
}

void launch_gpt_seq_layernorm(const float* x, const float* gamma, const float* beta, float* y, int B, int C, int T,
                              hipStream_t s) {
  hipLaunchKernelGGL(gpt_seq_layernorm_kernel, dim3(ceil_div(T, kSeqT), B), dim3(256), 0, s, x, gamma, beta, y, C, T);
  TTS_HIP_CHECK(hipGetLastError());
}

void launch_gpt_seq_gelu(float* x, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(gpt_seq_gelu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n);
  TTS_HIP_CHECK(hipGetLastError());
}

void launch_gpt_seq_kv(const float* qkv, const int64_t* klen, float* kc, float* vc, int B, int E, int T, int cap,
                       hipStream_t s) {
  hipLaunchKernelGGL(gpt_seq_kv_kernel, dim3(ceil_div(T, 64), ceil_div(E, 64), B), dim3(256), 0, s, qkv, klen, kc, vc, E,
                     T, cap);
  TTS_HIP_CHECK(hipGetLastError());
}

void launch_gpt_seq_column(const float* h, const int* plen, const int* n, int S, int s_, int B, int E, int T, int BT,
                           float* x, int* skip, hipStream_t s) {
  hipLaunchKernelGGL(gpt_seq_column_kernel, dim3(B), dim3(256), 0, s, h, plen, n, S, s_, E, T, BT, x, skip);
  TTS_HIP_CHECK(hipGetLastError());
}

void launch_gpt_skinny(const GptSkinnyArgs& a, hipStream_t s) {
  TTS_REQUIRE(a.B >= 1 && a.B <= kGptMaxBatch, 3, "batch must lie in [1, " + std::to_string(kGptMaxBatch) + "]");
  TTS_REQUIRE(a.BT == skinny_batch_tile(a.B) && a.Kp == skinny_kp(a.K) && a.nln >= 0 && a.nln <= 2 && a.out != a.x, 2,
              "internal: GPT skinny product arguments");
  switch (a.BT) {
    case 1: launch_gpt_skinny_bt<1>(a, s); break;
    case 2: launch_gpt_skinny_bt<2>(a, s); break;
    case 4: launch_gpt_skinny_bt<4>(a, s); break;
    case 8: launch_gpt_skinny_bt<8>(a, s); break;
    case 16: launch_gpt_skinny_bt<16>(a, s); break;
    default: launch_gpt_skinny_bt<32>(a, s); break;
  }
  TTS_HIP_CHECK(hipGetLastError());
}

void launch_gpt_decode_attn(const GptAttnArgs& a, hipStream_t s) {
  TTS_REQUIRE(a.B >= 1 && a.B <= kGptMaxBatch && a.heads >= 1 && a.heads * a.dk == a.E && a.cap >= 1, 2,
              "internal: GPT attention arguments");
  const dim3 grid(a.heads, a.B), block(64 * kGptAttnWaves);
  switch (a.dk) {
    case 32: hipLaunchKernelGGL(gpt_decode_attn_kernel<32>, grid, block, 0, s, a); break;
    case 64: hipLaunchKernelGGL(gpt_decode_attn_kernel<64>, grid, block, 0, s, a); break;
    case 128: hipLaunchKernelGGL(gpt_decode_attn_kernel<128>, grid, block, 0, s, a); break;
    default: throw Error(3, "XTTS GPT: the head size must be 32, 64 or 128");
  }
  TTS_HIP_CHECK(hipGetLastError());
}

void launch_gpt_sample(const GptSampleArgs& a, hipStream_t s) {
  TTS_REQUIRE(a.V >= 2 && a.V <= kGptMaxVocab, 3,
              "XTTS GPT: at most " + std::to_string(kGptMaxVocab) + " audio tokens (and at least 2)");
  TTS_REQUIRE(a.B >= 1 && a.step >= 0 && a.step < a.S, 2, "internal: GPT sample arguments");
  hipLaunchKernelGGL(gpt_sample_kernel, dim3(a.B), dim3(kSampleThreads), 0, s, a);
  TTS_HIP_CHECK(hipGetLastError());
}

void launch_gpt_embed(const GptEmbedArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(gpt_embed_kernel, dim3(a.B), dim3(256), 0, s, a);
  TTS_HIP_CHECK(hipGetLastError());
}

}  // namespace tts
