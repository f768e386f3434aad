// Conv2d 3x3 (pad 1) / 1x1 (pad 0), stride 1 or 2, on the matrix cores (gfx950), one launch per conv
// with its epilogue fused:  y = scale act(conv(x) + bias) + shift,  act = relu or the identity.
// Layouts and packing: conv2d.hpp.
//
// Output row fo of the conv is a GEMM over the KS input rows s fo + kf - P: rows = output channels,
// columns = output time, depth = input channels x KS x KS taps, with the split-precision operand
// schemes of split_device.hpp (fp32x6: fp32-faithful; bf16).  A workgroup of 4 waves owns one output
// row, kConv2dTile = 64 output columns and a group of up to 256 output channels (every channel of the
// trunk's convs; the head's 1x1 conv back to C3 F' channels takes several groups): wave w takes column
// block w & 1 and the 32-channel row blocks 8 rg + (w >> 1) + 2 i of its group rg.  The weights stream
// from L2 as ready fragments.  The
// activations pass through LDS per 32-channel chunk as rows of [piece][16 channels] (pitch S::ROWB),
// split while staging: KS input rows of (64 - 1) s + KS columns each, the zero padding at the plane
// border resolved in the staging index map (an out-of-plane element is a range-checked load: 0).
// The B fragment of output column c and tap (kf, kt) is staged row kf, column s c + kt: no im2col
// copy exists anywhere.  Per output the steps and products run in one fixed order, so results
// depend on neither the batch size nor the launch.
//
// Squeeze-and-excitation pooling (Conv2dArgs::pool): the epilogue also leaves, per (b, channel), the
// sum of the workgroup's outputs of each 32-column block, reduced over the lanes by a fixed butterfly
// and stored to a slot of its own ([b][channel][fo][column block]): no atomics, so the pooled mean
// the gate kernel forms from them in a fixed order is the same bits on every run and for every B.
#include <algorithm>

#include "conv2d.hpp"
#include "split_device.hpp"

namespace tts {

namespace {
constexpr int W = kConv2dTile;
constexpr int CG = 2;  // 16-channel groups per staged chunk
}  // namespace

template <class S, int NI, int KS>
__global__ __launch_bounds__(256) void conv2d_kernel(Conv2dArgs a) {
  constexpr int NP = S::NP;
  constexpr int ROWB = S::ROWB;
  constexpr int KK = KS * KS;
  constexpr int P = (KS - 1) / 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char conv2d_smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = wave_id();
  const int half = lane >> 5;
  const int l32 = lane & 31;
  const int cb = wave & 1, rh = wave >> 1;
  const int b = blockIdx.z;
  const int Fo = (a.F + a.stride - 1) / a.stride;
  const int rg = blockIdx.y / Fo;  // group of 8 row blocks
  const int fo = blockIdx.y - rg * Fo;
  const int t0 = blockIdx.x * W;
  const int Cin = a.Cin, Cout = a.Cout, F = a.F, T = a.T, st = a.stride;
  const int To = (T + st - 1) / st;
  const int G = (Cin + 15) >> 4, MB = (Cout + 31) >> 5;
  const int XR = (W - 1) * st + KS;  // staged columns of one input row
  const int nch = (G + CG - 1) / CG;

  unsigned char* xbuf = conv2d_smem;  // [CG][KS][XR][ROWB]

  const unsigned xbytes = (unsigned)Cin * (unsigned)F * (unsigned)T * 4u;
  const rsrc_t rx = make_rsrc(a.x + (size_t)b * Cin * F * T, xbytes);
  const rsrc_t ra = make_rsrc(a.a, a.a_bytes);
  const unsigned avoff = (unsigned)lane * 16u;

  // channels [32 c, 32 c + 32), input rows s fo - P + kf, columns s t0 - P + r -> xbuf[gl][kf][r], split
  auto stage = [&](int c) {
    const int per_q = KS * XR;
    const int units = CG * 4 * per_q;
    for (int u = tid; u < units; u += 256) {
      const int q = u / per_q, rem = u - q * per_q;
      const int kf = rem / XR, r = rem - kf * XR;
      const int fi = fo * st + kf - P, ti = t0 * st + r - P;
      const bool ok = fi >= 0 && fi < F && ti >= 0 && ti < T;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ch = 32 * c + 4 * q + j;
        v[j] = bload(rx, (ok && ch < Cin) ? (((unsigned)ch * (unsigned)F + (unsigned)fi) * (unsigned)T + (unsigned)ti) * 4u
                                          : OOB_OFF, 0u);
      }
      split_store4<S>(xbuf + (((q >> 2) * KS + kf) * XR + r) * ROWB + (q & 3) * 8, v[0], v[1], v[2], v[3]);
    }
  };

  int mb[NI];
  bool mbv[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    mb[i] = 8 * rg + rh + 2 * i;
    mbv[i] = mb[i] < MB;
  }
  f32x16 acc[NI];
  f32x4 af[2][NI][NP];  // A fragments: this step's and the next's
  const int S1 = KK * G;
  // A fragments of step s; past the packed array the range check gives 0
  auto load_a = [&](f32x4 (&dst)[NI][NP], int s) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int p = 0; p < NP; ++p)
        dst[i][p] = bload4(ra, (mbv[i] && s < S1) ? avoff : OOB_OFF, (unsigned)((mb[i] * S1 + s) * NP + p) * 1024u);
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
  // staged row of step j of a chunk: (group gl, taps kf, kt) = (j / KK, (j % KK) / KS, j % KS)
  auto brow_of = [&](int j) {
    const int gl = j / KK, k = j - KK * gl;
    const int kf = k / KS, kt = k - KS * kf;
    return xbuf + ((gl * KS + kf) * XR + col * st + kt) * ROWB + 16 * half;
  };

#pragma unroll
  for (int i = 0; i < NI; ++i) acc[i] = f32x16{};
  for (int c = 0; c < nch; ++c) {
    if (c > 0) __syncthreads();  // every wave is done with the previous chunk
    stage(c);
    __syncthreads();
    const int ng = min(CG, G - CG * c);
    const int ns = KK * ng;
    const int s0 = KK * CG * c;
    load_a(af[0], s0);
    for (int j = 0; j < ns; j += 2) {
      // two steps per iteration: the fragment ring returns to its start (no moves)
      load_a(af[1], s0 + j + 1);
      mma(af[0], brow_of(j));
      if (j + 1 < ns) {
        load_a(af[0], s0 + j + 2);
        mma(af[1], brow_of(j + 1));
      }
    }
  }

  // ---- y = scale act(acc + bias) + shift ----
  const rsrc_t ry = make_rsrc(a.y + (size_t)b * Cout * Fo * To, (unsigned)Cout * (unsigned)Fo * (unsigned)To * 4u);
  const int t = t0 + col;
  const bool relu = a.relu != 0;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    if (mbv[i]) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mb[i] * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        float v = acc[i][r] + a.bias[row];
        v = relu ? fmaxf(v, 0.f) : v;
        v = fmaf(v, a.scale[row], a.shift[row]);
        bstore(ry, v, (row < Cout && t < To) ? (((unsigned)row * (unsigned)Fo + (unsigned)fo) * (unsigned)To + (unsigned)t) * 4u
                                             : OOB_OFF, 0u);
        if (a.pool) {  // wave-uniform
          float p = t < To ? v : 0.f;
#pragma unroll
          for (int m = 1; m < 32; m <<= 1) p += __shfl_xor(p, m);  // within the 32 lanes of a half
          const int ncb = 2 * (int)gridDim.x;
          if (l32 == 0 && row < Cout)
            a.pool[(((size_t)b * Cout + row) * Fo + fo) * ncb + 2 * blockIdx.x + cb] = p;
        }
      }
    }
  }
}

size_t conv2d_lds(int mode, int KS, int stride) {
  const int rowb = mode == MATH_BF16 ? SchemeB1::ROWB : SchemeX6::ROWB;
  return (size_t)CG * KS * ((W - 1) * stride + KS) * rowb;
}

void conv2d_check(const Conv2dArgs& a, int B) {
  TTS_REQUIRE(a.x && a.y, 1, "conv2d: NULL argument");
  TTS_REQUIRE(a.KS == 3 || a.KS == 1, 3, "conv2d: the kernel must be 3x3 (pad 1) or 1x1 (pad 0)");
  TTS_REQUIRE(a.stride == 1 || a.stride == 2, 3, "conv2d: the stride must be 1 or 2");
  TTS_REQUIRE(a.Cin >= 1 && a.F >= 1 && a.T >= 1, 1, "conv2d: bad input shape");
  TTS_REQUIRE(a.Cout >= 1 && a.Cout <= kConv2dMaxCout, 3, "conv2d: output channels must lie in [1, 4096]");
  TTS_REQUIRE((int64_t)a.Cin * a.F * a.T * 4 < (int64_t)1 << 31, 3, "conv2d: a batch item's input plane exceeds 2 GiB");
  const int64_t Fo = conv2d_out(a.F, a.stride), To = conv2d_out(a.T, a.stride);
  TTS_REQUIRE((int64_t)a.Cout * Fo * To * 4 < (int64_t)1 << 31, 3, "conv2d: a batch item's output plane exceeds 2 GiB");
  TTS_REQUIRE(Fo * conv2d_rowgroups(a.Cout) <= 65535, 3,
              "conv2d: output rows x 256-channel groups exceed 65535");
  TTS_REQUIRE(B >= 1 && B <= 65535, 3, "conv2d: batch size must lie in [1, 65535]");
  TTS_REQUIRE((const void*)a.x != (const void*)a.y, 1, "conv2d: the output must not alias the input");
}

namespace {
template <class S, int KS>
void launch_s(const Conv2dArgs& a, const dim3& grid, size_t lds, hipStream_t s) {
  auto go = [&](auto kernel) {
    TTS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      kConv2dLdsLimit));
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, a);
  };
  switch ((std::min(conv2d_mblocks(a.Cout), 8) + 1) / 2) {
    case 1: go(conv2d_kernel<S, 1, KS>); break;
    case 2: go(conv2d_kernel<S, 2, KS>); break;
    case 3: go(conv2d_kernel<S, 3, KS>); break;
    default: go(conv2d_kernel<S, 4, KS>); break;
  }
}
}  // namespace

void launch_conv2d(int mode, const Conv2dArgs& a, int B, hipStream_t s) {
  TTS_REQUIRE(mode == MATH_FP32_X6 || mode == MATH_BF16, 3, "conv2d: math mode must be fp32x6 or bf16");
  conv2d_check(a, B);
  TTS_REQUIRE(a.a && a.bias && a.scale && a.shift, 1, "conv2d: NULL argument");
  const size_t lds = conv2d_lds(mode, a.KS, a.stride);
  TTS_REQUIRE(lds <= (size_t)kConv2dLdsLimit, 3, "conv2d: the tile does not fit the LDS");
  const dim3 grid(ceil_div(conv2d_out(a.T, a.stride), W), conv2d_out(a.F, a.stride) * conv2d_rowgroups(a.Cout), B);
  if (mode == MATH_BF16) {
    if (a.KS == 3) launch_s<SchemeB1, 3>(a, grid, lds, s);
    else launch_s<SchemeB1, 1>(a, grid, lds, s);
  } else {
    if (a.KS == 3) launch_s<SchemeX6, 3>(a, grid, lds, s);
    else launch_s<SchemeX6, 1>(a, grid, lds, s);
  }
  TTS_HIP_CHECK(hipGetLastError());
}

}  // namespace tts
