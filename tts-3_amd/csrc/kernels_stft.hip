// Linear spectrogram spec[b][k][t] = sqrt(|X[k][t]|^2 + 1e-6) (wav_to_spec, TTS/tts/models/vits.py,
// center=False) as one GEMM on the matrix cores (gfx950): rows = the windowed DFT matrix (packed on
// the host, stft.hpp: per 32-bin block a "re" row set and an "im" row set), columns = frames,
// depth = the n_fft samples of a frame.
//
// The frames are never materialised: frame t is samples [t hop, t hop + n_fft) of the reflect-padded
// wav, so the frames of one tile are a Hankel view of one contiguous window of (bn - 1) hop + n_fft
// samples.  A workgroup of 8 waves stages that window in LDS once (reflect padding resolved, the
// f16x3 input scale applied, split into the scheme's 16-bit pieces, one LDS plane per piece) and
// never writes it again, so there is no barrier after the staging.  The B fragment of k-step s for
// the lane of column c, half h is the 8 samples from c hop + 16 s + 8 h: one ds_read_b128 per piece.
//
// LDS image: frame starts are hop samples apart (512 B at hop 256), which would put the 16 lanes
// of a ds_read_b128 group on one 16-byte bank slot.  The window is therefore stored per hop block
// (hop samples) at a pitch of hop / 8 16-byte slots, plus one slot when that count is even: an odd
// slot pitch sends the 16 lanes of every group (columns of 16 distinct residues mod 16) to 16
// distinct slots, all 64 banks.  An 8-sample chunk never straddles a hop block (hop % 8 == 0).
//
// Wave w of a pass takes bin block 8 pass + w and keeps two accumulators per 32 columns over the same
// B fragments: re (cos rows) and im (-sin rows).  A lane then owns re and im of the same (bin,
// frame; flushed into a running sum every 8 k-steps in the fp32-faithful modes, see SUM), so the magnitude and
// the 1e-6 happen in the epilogue with no exchange, and only spec is
// written (consecutive lanes on consecutive t).  The DC bin's im row carries the Nyquist bin
// (stft.hpp), which the lane of bin 0 stores as a second output.  A (the matrix) streams from L2 as
// fragments, prefetched PD k-steps ahead.  Per output the k-steps and products run in one fixed order
// whatever the tile geometry, so results do not depend on the batch size or the launch shape.
#include <algorithm>

#include "split_device.hpp"
#include "stft.hpp"

namespace tts {

template <class S, int TN>
__global__ __launch_bounds__(512) void stft_kernel(StftArgs a) {
  constexpr int NP = S::NP;
  constexpr bool H3 = S::SCALED;
  constexpr int PD = 3;  // A prefetch distance in k-steps
  // The fp32-faithful modes move the MFMA accumulators into a running sum every FLUSH k-steps
  // (v_add_f32) and restart them from zero.  A bin that a tone fills sums n_fft coherent terms; in one
  // accumulator every MFMA (6 per k-step in fp32x6) rounds at the size of that partial sum: measured
  // max|d| 1.5e-4 at |X| = 204 (n_fft 1024), 1.0e-4 with the leading products in an accumulator of their
  // own.  With the flush the MFMAs round at 1/8 of the final magnitude at most and only the n_fft / 128
  // adds round at full size.
  constexpr bool SUM = S::NPROD > 1;
  constexpr int FLUSH = 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char stft_smem[];
  unsigned char* smem = stft_smem;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int l32 = lane & 31;
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * a.bn;  // first frame of the tile
  const int hop = a.hop;
  const int ex = H3 ? amax_exp(a.amax, b) : 0;
  const float xscale = H3 ? ldexpf(1.f, -ex) : 1.f;

  // ---- stage the window: hop block hb, sample w holds ypad[t0 hop + hb hop + w] ----
  {
    const int N = a.N;
    const rsrc_t rx = make_rsrc(a.wav + (size_t)b * a.wav_bstride, (unsigned)N * 4u);
    const int i0 = t0 * hop - a.pad;  // wav index of the window's first sample
    const int q4 = hop >> 2;          // 4-sample units per hop block
    const int units = a.nhb * q4;
    for (int u = tid; u < units; u += 512) {
      const int hb = u / q4, w4 = u - hb * q4;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int i = i0 + hb * hop + 4 * w4 + j;
        i = i < 0 ? -i : i;                  // left reflection (|i| <= pad < N)
        i = i >= N ? 2 * (N - 1) - i : i;    // right reflection
        // i < 0 now: past the padded wav (frames >= T of the last tile, never stored): zero
        v[j] = bload(rx, i >= 0 ? (unsigned)i * 4u : OOB_OFF, 0u);
        if (H3) v[j] *= xscale;
      }
      unsigned w0[NP], w1[NP];
      S::split2(v[0], v[1], w0);
      S::split2(v[2], v[3], w1);
      unsigned char* dst = smem + hb * a.pitch + w4 * 8;
#pragma unroll
      for (int pc = 0; pc < NP; ++pc) *reinterpret_cast<u32x2*>(dst + pc * a.plane) = u32x2{w0[pc], w1[pc]};
    }
  }
  __syncthreads();

  // ---- the lane's B address at k-step 0 (sample 8 half of its column) and the per-step advance ----
  int boff0[TN];
  const int q0 = (8 * half) / hop, ws0 = 8 * half - q0 * hop;
#pragma unroll
  for (int n = 0; n < TN; ++n) {
    // columns past the tile's frames (a window that had to be narrower than 32 TN) read the last
    // frame's samples: staged data, results never stored
    const int c = min(n * 32 + l32, a.bn - 1);
    boff0[n] = (c + q0) * a.pitch + ws0 * 2;
  }
  const int dq = 16 / hop, dw = 16 - dq * hop;  // a k-step = dq hop blocks + dw samples
  const int dstep = dq * a.pitch + dw * 2;
  const int dwrap = a.pitch - hop * 2;

  const int NS = a.nsteps;
  const int npt = (a.nblk + 7) >> 3;  // passes over the window
  const int RS = gridDim.z, rs = blockIdx.z;
  const int pass0 = rs * npt / RS, pass1 = (rs + 1) * npt / RS;
  const rsrc_t ra = make_rsrc(a.a, a.a_bytes);  // loads past the matrix (the last prefetches) return 0
  const unsigned avoff = (unsigned)lane * 16u;
  const float sc = H3 ? ldexpf(1.f, ex + a.w_exp) : 1.f;
  const int T = a.T;
  const bool pw = a.power != 0;  // |X|^2 instead of the magnitude
  const int nh = a.n_fft >> 1;
  const rsrc_t ry = make_rsrc(a.spec + (size_t)b * ((size_t)(nh + 1) * T), (unsigned)(nh + 1) * (unsigned)T * 4u);

  for (int pass = pass0; pass < pass1; ++pass) {
    const int blk = pass * 8 + wave;
    if (blk >= a.nblk) break;  // wave-uniform; no barrier follows
    const unsigned abase = (unsigned)blk * (unsigned)NS * (unsigned)(2 * NP * 1024);
    f32x4 ar[PD + 1][2][NP];
#pragma unroll
    for (int s = 0; s < PD; ++s)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int q = 0; q < NP; ++q) ar[s][c][q] = bload4(ra, avoff, abase + (unsigned)((s * 2 + c) * NP + q) * 1024u);
    f32x16 re[TN], im[TN], re_sum[TN], im_sum[TN];
    int boff[TN];
#pragma unroll
    for (int n = 0; n < TN; ++n) {
      re[n] = f32x16{};
      im[n] = f32x16{};
      re_sum[n] = f32x16{};
      im_sum[n] = f32x16{};
      boff[n] = boff0[n];
    }
    int ws = ws0;
    auto kstep = [&](int s) {
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int q = 0; q < NP; ++q)
          ar[PD][c][q] = bload4(ra, avoff, abase + (unsigned)(((s + PD) * 2 + c) * NP + q) * 1024u);
      f32x4 bf[TN][NP];
#pragma unroll
      for (int n = 0; n < TN; ++n)
#pragma unroll
        for (int q = 0; q < NP; ++q) bf[n][q] = *reinterpret_cast<const f32x4*>(smem + boff[n] + q * a.plane);
#pragma unroll
      for (int e = 0; e < S::NPROD; ++e)
#pragma unroll
        for (int n = 0; n < TN; ++n) {
          re[n] = S::mfma(ar[0][0][S::PA[e]], bf[n][S::PB[e]], re[n]);
          im[n] = S::mfma(ar[0][1][S::PA[e]], bf[n][S::PB[e]], im[n]);
        }
#pragma unroll
      for (int pp = 0; pp < PD; ++pp)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int q = 0; q < NP; ++q) ar[pp][c][q] = ar[pp + 1][c][q];
      ws += dw;
      int adv = dstep;
      if (ws >= hop) {
        ws -= hop;
        adv += dwrap;
      }
#pragma unroll
      for (int n = 0; n < TN; ++n) boff[n] += adv;
    };
    // PD + 1 steps per iteration: the ring of A fragments returns to its start, so the rotation
    // costs no moves; n_fft % 64 == 32 leaves two steps over
    int s = 0;
    for (; s + PD + 1 <= NS; s += PD + 1) {
#pragma unroll
      for (int u = 0; u <= PD; ++u) kstep(s + u);
      if (SUM && ((s + PD + 1) & (FLUSH - 1)) == 0) {
#pragma unroll
        for (int n = 0; n < TN; ++n) {
          re_sum[n] += re[n];
          im_sum[n] += im[n];
          re[n] = f32x16{};
          im[n] = f32x16{};
        }
      }
    }
    for (; s < NS; ++s) kstep(s);

    // ---- epilogue: magnitude, rows past n_fft/2 and columns past the tile / T suppressed ----
#pragma unroll
    for (int n = 0; n < TN; ++n) {
      const int c = n * 32 + l32;
      const int t = t0 + c;
      const bool okc = c < a.bn && t < T;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int bin = blk * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        float x = re[n][r], y = im[n][r];
        if (SUM) {
          x += re_sum[n][r];
          y += im_sum[n][r];
        }
        if (H3) {
          x *= sc;
          y *= sc;
        }
        float m2 = x * x + y * y;
        if (r == 0 && bin == 0) {  // DC: X[0] in re, the Nyquist bin's X[n_fft/2] in the im slot
          bstore(ry, pw ? y * y : sqrtf(y * y + 1e-6f), okc ? ((unsigned)nh * (unsigned)T + (unsigned)t) * 4u : OOB_OFF, 0u);
          m2 = x * x;
        }
        bstore(ry, pw ? m2 : sqrtf(m2 + 1e-6f), okc && bin < nh ? ((unsigned)bin * (unsigned)T + (unsigned)t) * 4u : OOB_OFF, 0u);
      }
    }
  }
}

namespace {
template <class S>
void launch_s(int TN, const StftArgs& a, const dim3& grid, size_t lds, hipStream_t s) {
  auto go = [&](auto kernel) {
    // above the default dynamic LDS limit: opt in (per function; cheap and idempotent)
    TTS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      kStftLdsLimit));
    hipLaunchKernelGGL(kernel, grid, dim3(512), lds, s, a);
  };
  if (TN == 2) go(stft_kernel<S, 2>);
  else go(stft_kernel<S, 1>);
}
}  // namespace

void launch_stft(int mode, int TN, const StftArgs& a, int B, int tiles, int RS, hipStream_t s) {
  const size_t lds = (size_t)a.plane * stft_pieces(mode);
  TTS_REQUIRE(lds <= (size_t)kStftLdsLimit && a.bn >= 1 && a.bn <= 32 * TN && (TN == 1 || TN == 2), 1,
              "stft: bad launch geometry");
  const dim3 grid(tiles, B, RS);
  if (mode == MATH_FP32_F16X3) launch_s<SchemeH3>(TN, a, grid, lds, s);
  else if (mode == MATH_BF16) launch_s<SchemeB1>(TN, a, grid, lds, s);
  else launch_s<SchemeX6>(TN, a, grid, lds, s);
  TTS_HIP_CHECK(hipGetLastError());
}

}  // namespace tts
