// Multi-head self-attention of the FFTransformer layers (ForwardTTS / FastPitch) on gfx950:
// online-softmax ("flash") attention on v_mfma_f32_32x32x16_bf16.  Interface: fft_attn.hpp.
//
// Reference (Coqui TTS 0.22.0): TTS/tts/layers/generic/transformer.py, self_attn =
// nn.MultiheadAttention: scores (q dk^-0.5)^T k, -inf under the key padding mask, softmax over keys.
//
// One workgroup = kMhaTile (64) queries of one head of one utterance, 4 waves.  Wave w owns query
// block qb = w & 1 (32 queries, one per lane column) and the depth half dh = w >> 1:
//   - of the score product it sums the 16-channel k-steps 2 i + dh (its Q fragments stay in
//     registers for the whole kernel, scaled by dk^-0.5 log2 e and split once),
//   - of O it owns the 32-channel row blocks 2 i + dh (dk x 64 fp32 over the workgroup: 96
//     accumulator registers per lane at dk = 384).
// Per tile of 32 keys:
//   1. K[32 keys][dk] goes to LDS split into the scheme's bf16 pieces; S^T[key][query] partial
//      sums = K Q on the MFMA (A = K rows, B = Q): the key lands in the accumulator registers,
//      the query on the lane.  The two depth halves exchange their partial tiles through LDS
//      (4 KiB per wave) and add them; both waves of a pair then hold the same scores.
//   2. masked keys (>= key_len, which also covers the keys past T of the last tile) become -inf;
//      running max / sum per query in fp32 (16 registers + one cross-half shuffle), p = exp2(s - m),
//      O *= exp2(m_old - m).
//   3. V[dk][32 keys] replaces K in the same LDS buffer; O^T += V P^T with the score accumulator
//      itself as the B operand: registers 8 s .. 8 s + 7 of a lane are k-step s, element j being key
//      16 s + 8 (j >> 2) + 4 (lane >> 5) + (j & 3); the V image is staged in that key order.
// K and V pass through registers on their way to LDS, loaded early and written late: this tile's V
// loads are in flight during the score product, the next tile's K loads during the softmax and the
// second product (at one wave per SIMD nothing else hides their latency).
// The scores never leave the workgroup, no buffer holds a whole score row (no limit on T), and
// every sum runs in one fixed order, so a batch item's result does not depend on the batch.
// key_len is clamped to [0, T]; an item with no key (length 0) writes zeros.
//
// Math: SchemeX6 (three exact bf16 pieces per fp32 operand - Q, K, P and V -, the six products with
// i + j <= 2 into one accumulator, smallest first) or SchemeB1 (single bf16 products).
#include "fft_attn.hpp"
#include "split_device.hpp"

namespace tts {

namespace {
constexpr int KT = 32;  // keys per tile
constexpr float kLog2e = 1.4426950408889634f;
}  // namespace

struct MhaArgs {
  const float* qkv;
  const int64_t* key_len;
  float* out;
  int E, T;
  float qscale;  // dk^-0.5 log2 e
};

template <class S>
__device__ __forceinline__ void split_frag(const float (&v)[8], f32x4 (&f)[S::NP]) {
  unsigned w[4][S::NP];
#pragma unroll
  for (int k = 0; k < 4; ++k) S::split2(v[2 * k], v[2 * k + 1], w[k]);
#pragma unroll
  for (int p = 0; p < S::NP; ++p) f[p] = __builtin_bit_cast(f32x4, u32x4_t{w[0][p], w[1][p], w[2][p], w[3][p]});
}

// CAUSAL: query i attends to the keys j <= i only (and j < key_len).  A workgroup stops after the key
// tile that holds its last query's diagonal (tiles wholly above the diagonal are skipped) and masks
// the keys above each query's own diagonal like padded keys: their probability is exactly 0, so
// nothing at a position > i reaches the output of position i.
template <class S, int DK, bool CAUSAL = false>
__global__ __launch_bounds__(256) void mha_kernel(MhaArgs a) {
  constexpr int NP = S::NP;
  constexpr int ROWB = S::ROWB;
  constexpr int NB = DK / 32;         // 32-channel blocks of the head
  constexpr int NKS = NB;             // score k-steps of one wave (half of DK / 16)
  constexpr int NOB = (NB + 1) / 2;   // O row blocks of one wave (the last may be absent)
  constexpr int TILEB = 2 * DK * ROWB;  // K image [DK / 16][32 keys][ROWB] = V image [2][DK][ROWB]
  extern __shared__ __attribute__((aligned(16))) unsigned char mha_smem[];
  unsigned char* tile = mha_smem;
  float* sx = reinterpret_cast<float*>(mha_smem + TILEB);  // [4 waves][16][64]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = wave_id();
  const int half = lane >> 5;
  const int l32 = lane & 31;
  const int qb = wave & 1, dh = wave >> 1;
  const int h = blockIdx.y, b = blockIdx.z;
  const int T = a.T, E = a.E;
  const int qi = blockIdx.x * kMhaTile + qb * 32 + l32;  // this lane's query
  const unsigned uT = (unsigned)T;
  const unsigned rowq = (unsigned)(h * DK), rowk = (unsigned)(E + h * DK), rowv = (unsigned)(2 * E + h * DK);

  const rsrc_t rx = make_rsrc(a.qkv + (size_t)b * 3 * E * T, 3u * (unsigned)E * uT * 4u);
  int klen = T;
  if (a.key_len) {
    const int64_t kl = a.key_len[b];
    klen = kl < 0 ? 0 : (kl < (int64_t)T ? (int)kl : T);
  }

  // ---- Q fragments: B operand, element j of k-step ks = channel 16 ks + 8 half + j ----
  f32x4 qf[NKS][NP];
#pragma unroll
  for (int i = 0; i < NKS; ++i) {
    const int ks = 2 * i + dh;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned ch = rowq + (unsigned)(16 * ks + 8 * half + j);
      v[j] = bload(rx, qi < T ? (ch * uT + (unsigned)qi) * 4u : OOB_OFF, 0u) * a.qscale;
    }
    split_frag<S>(v, qf[i]);
  }

  f32x16 o[NOB];
#pragma unroll
  for (int i = 0; i < NOB; ++i) o[i] = f32x16{};
  float m_run = -INFINITY, l_run = 0.f;

  // K / V staging through registers, issue early / write late: a thread moves NU units of 4 values
  // per tile.  K unit: 4 channels of one key -> rows [16-channel group][key]; V unit: 4 keys of one
  // channel -> rows [k-step][channel], the keys of a k-step in operand order.
  constexpr int NU = DK / 32;
  // registers for the next K tile as well; fp32x6 at dk = 384 holds 144 of Q fragments: V only
  constexpr bool PFK = NP == 1 || DK <= 256;
  constexpr int NVP = PFK ? NU : NU / 2;  // V units loaded early (the rest at their store)
  auto kload = [&](int k0, int i, float (&v)[4]) {
    const int u = tid + 256 * i;
    const int q4 = u >> 5, t = k0 + (u & 31);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      v[j] = bload(rx, t < T ? ((rowk + (unsigned)(4 * q4 + j)) * uT + (unsigned)t) * 4u : OOB_OFF, 0u);
  };
  auto kstore = [&](int i, const float (&v)[4]) {
    const int u = tid + 256 * i;
    const int q4 = u >> 5, r = u & 31;
    split_store4<S>(tile + ((q4 >> 2) * KT + r) * ROWB + (q4 & 3) * 8, v[0], v[1], v[2], v[3]);
  };
  auto vload = [&](int k0, int i, float (&v)[4]) {
    const int u = tid + 256 * i;
    const int d = u >> 3, qd = u & 7;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = k0 + 4 * qd + j;
      v[j] = bload(rx, t < T ? ((rowv + (unsigned)d) * uT + (unsigned)t) * 4u : OOB_OFF, 0u);
    }
  };
  auto vstore = [&](int i, const float (&v)[4]) {
    const int u = tid + 256 * i;
    const int d = u >> 3, qd = u & 7;
    const int st = qd >> 2, aa = (qd >> 1) & 1, hh = qd & 1;
    split_store4<S>(tile + (st * DK + d) * ROWB + (2 * hh + aa) * 8, v[0], v[1], v[2], v[3]);
  };
  float vr[NVP][4];
  float kr[PFK ? NU : 1][4];
  (void)kr;
  if constexpr (PFK) {
#pragma unroll
    for (int i = 0; i < NU; ++i) kload(0, i, kr[i]);
  }

  const int kend = CAUSAL ? min(klen, ((int)blockIdx.x + 1) * kMhaTile) : klen;
  for (int k0 = 0; k0 < kend; k0 += KT) {
    // ---- K tile -> LDS ----
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      if constexpr (PFK) {
        kstore(i, kr[i]);
      } else {
        float v[4];
        kload(k0, i, v);
        kstore(i, v);
      }
    }
    // this tile's V: in flight during the score product
#pragma unroll
    for (int i = 0; i < NVP; ++i) vload(k0, i, vr[i]);
    __syncthreads();

    // ---- S^T partial = K Q over this wave's k-steps ----
    f32x16 sc = f32x16{};
#pragma unroll
    for (int i = 0; i < NKS; ++i) {
      const int ks = 2 * i + dh;
      const unsigned char* row = tile + (ks * KT + l32) * ROWB + 16 * half;
      f32x4 kf[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) kf[p] = *reinterpret_cast<const f32x4*>(row + 32 * p);
#pragma unroll
      for (int e = 0; e < S::NPROD; ++e) sc = S::mfma(kf[S::PA[e]], qf[i][S::PB[e]], sc);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) sx[(wave * 16 + r) * 64 + lane] = sc[r];
    __syncthreads();  // partial tiles visible; every wave is done with the K image

    // ---- V tile -> LDS (over K): rows [k-step][channel], the keys of a k-step in operand order ----
#pragma unroll
    for (int i = 0; i < NVP; ++i) vstore(i, vr[i]);
#pragma unroll
    for (int i = NVP; i < NU; ++i) {
      float v[4];
      vload(k0, i, v);
      vstore(i, v);
    }
    // the next tile's K: in flight during the softmax and the second product (past T: zeros)
    if constexpr (PFK) {
#pragma unroll
      for (int i = 0; i < NU; ++i) kload(k0 + KT, i, kr[i]);
    }

    // ---- scores of the pair, mask, online softmax ----
    float mt = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      // one order of the two halves' sum in both waves of the pair
      const float s0 = dh == 0 ? sc[r] : sx[((wave ^ 2) * 16 + r) * 64 + lane];
      const float s1 = dh == 0 ? sx[((wave ^ 2) * 16 + r) * 64 + lane] : sc[r];
      const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      sc[r] = (key < klen && (!CAUSAL || key <= qi)) ? s0 + s1 : -INFINITY;
      mt = fmaxf(mt, sc[r]);
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32));
    // key k0 < klen is in every query's tile: the new maximum is finite (causal: key 0 is in every
    // query's first tile, and a later tile wholly above a query's diagonal leaves its maximum alone)
    const float m_new = fmaxf(m_run, mt);
    const float alpha = exp2f(m_run - m_new);  // first tile: exp2(-inf) = 0
    m_run = m_new;
    float ls = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      sc[r] = exp2f(sc[r] - m_new);  // masked keys: exactly 0
      ls += sc[r];
    }
    ls += __shfl_xor(ls, 32);
    l_run = l_run * alpha + ls;
#pragma unroll
    for (int i = 0; i < NOB; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[i][r] *= alpha;

    // P^T fragments: the accumulator as the B operand of the next product
    f32x4 pf[2][NP];
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = sc[8 * st + j];
      split_frag<S>(v, pf[st]);
    }
    __syncthreads();  // V image complete

    // ---- O^T += V P^T ----
#pragma unroll
    for (int i = 0; i < NOB; ++i) {
      const int ob = 2 * i + dh;
      if (ob < NB) {
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          const unsigned char* row = tile + (st * DK + ob * 32 + l32) * ROWB + 16 * half;
          f32x4 vf[NP];
#pragma unroll
          for (int p = 0; p < NP; ++p) vf[p] = *reinterpret_cast<const f32x4*>(row + 32 * p);
#pragma unroll
          for (int e = 0; e < S::NPROD; ++e) o[i] = S::mfma(vf[S::PA[e]], pf[st][S::PB[e]], o[i]);
        }
      }
    }
    __syncthreads();  // every wave is done with the V image and the exchanged tiles
  }

  // ---- out = O / l ----
  const rsrc_t ry = make_rsrc(a.out + (size_t)b * E * T, (unsigned)E * uT * 4u);
  // no key at all (key_len 0: the loop above never ran, O = 0 and l = 0): zeros, not 0 / 0
  const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
#pragma unroll
  for (int i = 0; i < NOB; ++i) {
    const int ob = 2 * i + dh;
    if (ob < NB) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const unsigned ch = rowq + (unsigned)(ob * 32 + (r & 3) + 8 * (r >> 2) + 4 * half);
        bstore(ry, o[i][r] * inv, qi < T ? (ch * uT + (unsigned)qi) * 4u : OOB_OFF, 0u);
      }
    }
  }
}

bool mha_head_size_ok(int dk) { return dk == 32 || dk == 64 || dk == 128 || dk == 192 || dk == 256 || dk == 384; }

namespace {
constexpr int kMhaLdsLimit = 160 * 1024;

template <class S, int DK, bool CAUSAL = false>
void launch_mha_k(const MhaArgs& a, const dim3& grid, hipStream_t s) {
  constexpr size_t lds = (size_t)2 * DK * S::ROWB + 4 * 16 * 64 * sizeof(float);
  static_assert(lds <= (size_t)kMhaLdsLimit, "the tile does not fit the LDS");
  auto kernel = mha_kernel<S, DK, CAUSAL>;
  if (lds > 64 * 1024)
    TTS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds));
  hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, a);
}

template <class S>
void launch_mha_s(int dk, const MhaArgs& a, const dim3& grid, hipStream_t s) {
  switch (dk) {
    case 32: launch_mha_k<S, 32>(a, grid, s); break;
    case 64: launch_mha_k<S, 64>(a, grid, s); break;
    case 128: launch_mha_k<S, 128>(a, grid, s); break;
    case 192: launch_mha_k<S, 192>(a, grid, s); break;
    case 256: launch_mha_k<S, 256>(a, grid, s); break;
    default: launch_mha_k<S, 384>(a, grid, s); break;
  }
}

template <class S>
void launch_mha_causal_s(int dk, const MhaArgs& a, const dim3& grid, hipStream_t s) {
  switch (dk) {
    case 32: launch_mha_k<S, 32, true>(a, grid, s); break;
    case 64: launch_mha_k<S, 64, true>(a, grid, s); break;
    default: launch_mha_k<S, 128, true>(a, grid, s); break;
  }
}
}  // namespace

void launch_mha_causal(int mode, const float* qkv, const int64_t* key_len, float* out, int B, int E, int heads, int T,
                       hipStream_t s) {
  TTS_REQUIRE(mode == MATH_FP32_X6 || mode == MATH_BF16, 3, "mha: math mode must be fp32x6 or bf16");
  TTS_REQUIRE(B >= 1 && E >= 1 && heads >= 1 && T >= 1, 1, "mha: bad shape");
  TTS_REQUIRE(E % heads == 0, 1, "mha: the channels must divide into the heads");
  const int dk = E / heads;
  TTS_REQUIRE(E <= kMhaCausalMaxE && (dk == 32 || dk == 64 || dk == 128), 3,
              "causal mha: head size must be one of 32, 64, 128 with at most 2048 channels");
  TTS_REQUIRE(B <= 65535 && heads <= 65535, 3, "mha: batch size and heads must lie in [1, 65535]");
  TTS_REQUIRE((int64_t)3 * E * T * 4 < (int64_t)1 << 31, 3, "mha: a batch item's qkv plane exceeds 2 GiB");
  TTS_REQUIRE(qkv != out, 1, "mha: the output must not alias the input");
  MhaArgs a{qkv, key_len, out, E, T, kLog2e / sqrtf((float)dk)};
  const dim3 grid((T + kMhaTile - 1) / kMhaTile, heads, B);
  if (mode == MATH_BF16) launch_mha_causal_s<SchemeB1>(dk, a, grid, s);
  else launch_mha_causal_s<SchemeX6>(dk, a, grid, s);
  TTS_HIP_CHECK(hipGetLastError());
}

template <class S>
void launch_mha_wide_s(int dk, const MhaArgs& a, const dim3& grid, hipStream_t s) {
  switch (dk) {
    case 32: launch_mha_k<S, 32>(a, grid, s); break;
    case 64: launch_mha_k<S, 64>(a, grid, s); break;
    default: launch_mha_k<S, 128>(a, grid, s); break;
  }
}

// The non-causal kernel past launch_mha's 512 channels (the XTTS conditioning encoder: 1024 channels in
// 16 heads): the same instantiations, so a shape both accept gives the same bits.
void launch_mha_wide(int mode, const float* qkv, const int64_t* key_len, float* out, int B, int E, int heads, int T,
                     hipStream_t s) {
  TTS_REQUIRE(mode == MATH_FP32_X6 || mode == MATH_BF16, 3, "mha: math mode must be fp32x6 or bf16");
  TTS_REQUIRE(B >= 1 && E >= 1 && heads >= 1 && T >= 1, 1, "mha: bad shape");
  TTS_REQUIRE(E % heads == 0, 1, "mha: the channels must divide into the heads");
  const int dk = E / heads;
  TTS_REQUIRE(E <= kMhaCausalMaxE && (dk == 32 || dk == 64 || dk == 128), 3,
              "wide mha: head size must be one of 32, 64, 128 with at most 2048 channels");
  TTS_REQUIRE(B <= 65535 && heads <= 65535, 3, "mha: batch size and heads must lie in [1, 65535]");
  TTS_REQUIRE((int64_t)3 * E * T * 4 < (int64_t)1 << 31, 3, "mha: a batch item's qkv plane exceeds 2 GiB");
  TTS_REQUIRE(qkv != out, 1, "mha: the output must not alias the input");
  MhaArgs a{qkv, key_len, out, E, T, kLog2e / sqrtf((float)dk)};
  const dim3 grid((T + kMhaTile - 1) / kMhaTile, heads, B);
  if (mode == MATH_BF16) launch_mha_wide_s<SchemeB1>(dk, a, grid, s);
  else launch_mha_wide_s<SchemeX6>(dk, a, grid, s);
  TTS_HIP_CHECK(hipGetLastError());
}

void launch_mha(int mode, const float* qkv, const int64_t* key_len, float* out, int B, int E, int heads, int T,
                hipStream_t s) {
  TTS_REQUIRE(mode == MATH_FP32_X6 || mode == MATH_BF16, 3, "mha: math mode must be fp32x6 or bf16");
  TTS_REQUIRE(B >= 1 && E >= 1 && heads >= 1 && T >= 1, 1, "mha: bad shape");
  TTS_REQUIRE(E % heads == 0, 1, "mha: the channels must divide into the heads");
  TTS_REQUIRE(E <= kMhaMaxE && mha_head_size_ok(E / heads), 3,
              "mha: head size must be one of 32, 64, 128, 192, 256, 384 with at most 512 channels");
  TTS_REQUIRE(B <= 65535 && heads <= 65535, 3, "mha: batch size and heads must lie in [1, 65535]");
  TTS_REQUIRE((int64_t)3 * E * T * 4 < (int64_t)1 << 31, 3, "mha: a batch item's qkv plane exceeds 2 GiB");
  TTS_REQUIRE(qkv != out, 1, "mha: the output must not alias the input");
  const int dk = E / heads;
  MhaArgs a{qkv, key_len, out, E, T, kLog2e / sqrtf((float)dk)};
  const dim3 grid((T + kMhaTile - 1) / kMhaTile, heads, B);
  if (mode == MATH_BF16) launch_mha_s<SchemeB1>(dk, a, grid, s);
  else launch_mha_s<SchemeX6>(dk, a, grid, s);
  TTS_HIP_CHECK(hipGetLastError());
}

}  // namespace tts
