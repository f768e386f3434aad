// XTTS conditioning executor (tts_xtts_cond_*) and the resampler (tts_resample_*).
//   mel:       centred STFT, |X|^2 (stft.hpp) | filterbank, clamp, log, / mel_norms
//   style_emb: init conv (spec_dim -> E)
//              | per AttentionBlock: GroupNorm | qkv conv | flash attention | proj_out conv + the normalised input
//              | the learned latents copied to every batch item
//              | per perceiver layer: to_q | to_kv on the latents | to_kv on the context | cross-attention over
//                (latents, context) | to_out + residual | FF product with GEGLU | FF product + residual
//              | RMSNorm
// The latents live as planes [B][E][L] (L = num_latents columns), the layout get_style_emb returns.  The
// encoder's products and to_kv over the context's T columns are 1x1 convs of the conv path.  The
// perceiver's products over the L latent columns are launch_cond_product (kernels_xtts_cond.hip): 32
// columns fill a quarter of a conv tile's columns and leave 8 workgroups for a 1024-row matrix, and the
// GPT's skinny product takes at most 32 columns in all (B x 32 exceeds that from B = 2) and needs K % 64 == 0.
#include "xtts_cond.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <string>

namespace tts {

namespace {
constexpr float kGnEps = 1e-5f;
size_t al(size_t n) { return HostArena::align(n); }
TtsStftCfg stft_cfg(const TtsXttsCondCfg& c) {
  TtsStftCfg s{};
  s.n_fft = c.n_fft;
  s.hop_length = c.hop_length;
  s.win_length = c.win_length;
  s.math_mode = MATH_FP32_X6;  // the front end is fp32-faithful in every mode
  return s;
}
int conv_mode_of(int math_mode) { return math_mode == MATH_BF16 ? MATH_BF16 : MATH_FP32_X6; }

// torch Conv1d(K = 1) / Linear weight w [Cout][Cin] with its bias (nullptr: none)
void put_conv1(HostArena& arena, int mode, PackedConv& cv, const float* w, const float* b, int Cin, int Cout, bool res) {
  cv.Cin = Cin; cv.Cout = Cout; cv.K = 1;
  cv.tile = conv_tile_for(mode, Cout, 1, Cin, 1, res);
  std::vector<float> zero;
  if (!b) {
    zero.assign((size_t)Cout, 0.f);
    b = zero.data();
  }
  TTS_REQUIRE(arena.put_conv(cv, mode, conv_tile(mode, cv.tile), w, b) == 0, 3,
              "XTTS conditioning: scaled packing unsupported");
}

void run_conv1(int mode, const PackedConv& cv, const float* in, float* out, const float* res, int B, int T,
               hipStream_t s) {
  Conv1dArgs a{};
  a.x = in; a.w = cv.w; a.bias = cv.b; a.y = out; a.res = res;
  a.Cin = cv.Cin; a.Cout = cv.Cout; a.Tin = T; a.Tout = T;
  a.dil = 1; a.pad = 0; a.n_chunks = cv.n_chunks;
  a.in_slope = 1.f; a.out_slope = 1.f; a.zmode = 0; a.zdiv = 1.f;
  launch_conv(mode, a, B, 1, cv.tile, s);
}
}  // namespace

void xtts_cond_validate(const TtsXttsCondCfg& c) {
  TTS_REQUIRE(c.math_mode >= MATH_FP32 && c.math_mode <= MATH_LAST, 1, "XTTS conditioning: unknown math_mode");
  TTS_REQUIRE(c.spec_dim >= 1 && c.model_dim >= 1 && c.heads >= 1 && c.model_dim % c.heads == 0, 1,
              "bad XTTS conditioning configuration: spec_dim, model_dim, heads");
  TTS_REQUIRE(c.attn_blocks >= 0 && c.perceiver_depth >= 1 && c.num_latents >= 1 && c.perceiver_dim_head >= 1 &&
                  c.perceiver_heads >= 1 && c.ff_mult >= 1,
              1, "bad XTTS conditioning configuration: attn_blocks, perceiver_depth, num_latents, perceiver heads, ff_mult");
  TTS_REQUIRE(c.n_fft >= 1 && c.hop_length >= 1 && c.win_length >= 1, 1,
              "XTTS conditioning: n_fft, win_length and hop_length must be positive");
  const int dk = c.model_dim / c.heads;
  TTS_REQUIRE(c.model_dim <= kMhaCausalMaxE && (dk == 32 || dk == 64 || dk == 128), 3,
              "XTTS conditioning: head size must be one of 32, 64, 128 with at most 2048 channels");
  TTS_REQUIRE(c.num_latents <= kCondMaxLatents, 3,
              "XTTS conditioning: at most " + std::to_string(kCondMaxLatents) + " latents");
  TTS_REQUIRE(c.perceiver_dim_head <= 256 && (int64_t)c.perceiver_heads * c.perceiver_dim_head <= 4096, 3,
              "XTTS conditioning: perceiver_dim_head <= 256 and perceiver_heads * perceiver_dim_head <= 4096");
  TTS_REQUIRE(c.attn_blocks <= 64 && c.perceiver_depth <= 64 && c.spec_dim <= 1024 && c.ff_mult <= 16, 3,
              "XTTS conditioning: at most 64 attention blocks and perceiver layers, spec_dim <= 1024, ff_mult <= 16");
  TTS_REQUIRE(cond_ff_inner(c) >= 1, 1, "XTTS conditioning: the feed-forward's inner width is 0");
  stft_validate(stft_cfg(c));
}

std::vector<int64_t> xtts_cond_weight_shapes(const TtsXttsCondCfg& c) {
  const int64_t E = c.model_dim, inner = (int64_t)c.perceiver_heads * c.perceiver_dim_head, I = cond_ff_inner(c);
  std::vector<int64_t> n = {E * c.spec_dim, E};
  for (int i = 0; i < c.attn_blocks; ++i)
    for (int64_t v : {E, E, 3 * E * E, 3 * E, E * E, E}) n.push_back(v);
  n.push_back((int64_t)c.num_latents * E);
  for (int i = 0; i < c.perceiver_depth; ++i)
    for (int64_t v : {inner * E, 2 * inner * E, E * inner, 2 * I * E, 2 * I, E * I, E}) n.push_back(v);
  n.push_back(E);
  n.push_back(c.win_length);
  n.push_back((int64_t)(c.n_fft / 2 + 1) * c.spec_dim);
  return n;
}

XttsCond::XttsCond(const TtsXttsCondCfg& cfg, const float* const* hw, int device) : cfg_(cfg), device_(device) {
  xtts_cond_validate(cfg_);
  const auto shapes = xtts_cond_weight_shapes(cfg_);
  for (size_t i = 0; i < shapes.size(); ++i)
    TTS_REQUIRE(hw[i] != nullptr, 1, "weight pointer " + std::to_string(i) + " is NULL");
  int dev_count = 0;
  TTS_HIP_CHECK(hipGetDeviceCount(&dev_count));
  TTS_REQUIRE(device >= 0 && device < dev_count, 1, "XTTS conditioning: bad device index");
  mode_ = conv_mode_of(cfg_.math_mode);
  bf16_ = mode_ == MATH_BF16;
  E_ = cfg_.model_dim; H_ = cfg_.heads; G_ = cond_groupnorm_groups(E_); L_ = cfg_.num_latents;
  inner_ = cfg_.perceiver_heads * cfg_.perceiver_dim_head;
  I_ = cond_ff_inner(cfg_);

  HostArena arena;
  size_t wi = 0;
  put_conv1(arena, mode_, init_, hw[wi], hw[wi + 1], cfg_.spec_dim, E_, false);
  wi += 2;
  // the arena keeps the addresses of the pointer members until upload() patches them: no reallocation
  blocks_.resize((size_t)cfg_.attn_blocks);
  std::vector<float> wq((size_t)3 * E_ * E_), bq((size_t)3 * E_);
  for (Block& b : blocks_) {
    arena.put(hw[wi], (size_t)E_, &b.gn_g);
    arena.put(hw[wi + 1], (size_t)E_, &b.gn_b);
    pack_cond_qkv(hw[wi + 2], hw[wi + 3], E_, H_, wq.data(), bq.data());
    put_conv1(arena, mode_, b.qkv, wq.data(), bq.data(), E_, 3 * E_, false);
    put_conv1(arena, mode_, b.proj, hw[wi + 4], hw[wi + 5], E_, E_, true);
    wi += 6;
  }
  {  // latents [L][E] as the plane [E][L]
    const size_t off = arena.alloc((size_t)E_ * L_, &lat0_);
    float* p = arena.at(off);
    for (int l = 0; l < L_; ++l)
      for (int c = 0; c < E_; ++c) p[(size_t)c * L_ + l] = hw[wi][(size_t)l * E_ + c];
    ++wi;
  }
  layers_.resize((size_t)cfg_.perceiver_depth);
  auto put_rows = [&](const float* w, int64_t n, float** dst) {
    const size_t off = arena.alloc((size_t)cond_rows_numel(n, bf16_), dst);
    pack_cond_rows(w, n, bf16_, arena.at(off));
  };
  for (Layer& l : layers_) {
    put_rows(hw[wi], (int64_t)inner_ * E_, &l.w_q);
    put_rows(hw[wi + 1], (int64_t)2 * inner_ * E_, &l.w_kv);
    put_conv1(arena, mode_, l.to_kv, hw[wi + 1], nullptr, E_, 2 * inner_, false);
    put_rows(hw[wi + 2], (int64_t)E_ * inner_, &l.w_out);
    put_rows(hw[wi + 3], (int64_t)2 * I_ * E_, &l.w_ff0);
    arena.put(hw[wi + 4], (size_t)2 * I_, &l.b_ff0);
    put_rows(hw[wi + 5], (int64_t)E_ * I_, &l.w_ff2);
    arena.put(hw[wi + 6], (size_t)E_, &l.b_ff2);
    wi += 7;
  }
  arena.put(hw[wi++], (size_t)E_, &gamma_);
  stft_.reset(new Stft(stft_cfg(cfg_), hw[wi++], device, /*center=*/true, /*power=*/true));
  {  // the filterbank and, per column, the bins [lo, hi) that hold its nonzero entries
    const int K = cfg_.n_fft / 2 + 1, M = cfg_.spec_dim;
    const float* fb = hw[wi++];
    arena.put(fb, (size_t)K * M, &fb_);
    std::vector<int> range((size_t)2 * M);
    for (int m = 0; m < M; ++m) {
      int lo = K, hi = 0;
      for (int k = 0; k < K; ++k)
        if (fb[(size_t)k * M + m] != 0.f) {
          lo = std::min(lo, k);
          hi = k + 1;
        }
      range[2 * m] = std::min(lo, hi);
      range[2 * m + 1] = hi;
    }
    static_assert(sizeof(int) == sizeof(float), "the arena holds 4-byte words");
    std::memcpy(arena.at(arena.alloc(range.size(), &fb_range_)), range.data(), range.size() * sizeof(int));
  }
  TTS_REQUIRE(wi == shapes.size(), 1, "internal: XTTS conditioning weight inventory mismatch");
  arena.upload(device_, arena_);
}

int XttsCond::num_frames(int64_t N) const {
  TTS_REQUIRE(N >= 1, 1, "XTTS conditioning: the clip must not be empty");
  TTS_REQUIRE(N >= cfg_.n_fft / 2 + 1, 3,
              "XTTS conditioning: the clip must have at least n_fft / 2 + 1 = " + std::to_string(cfg_.n_fft / 2 + 1) +
                  " samples (the centred STFT's reflect padding)");
  TTS_REQUIRE(N * 4 < (int64_t)1 << 31, 3, "XTTS conditioning: a clip must stay below 2 GiB");
  const int64_t T = 1 + N / cfg_.hop_length;
  TTS_REQUIRE(L_ + T <= kCondMaxKeys, 3,
              "XTTS conditioning: num_latents + frames must not exceed " + std::to_string(kCondMaxKeys));
  return (int)T;
}

void XttsCond::mel(const float* wav, int B, int64_t N, const float* mel_norms, float* out, hipStream_t s,
                   Profiler* prof) {
  TTS_REQUIRE(wav && mel_norms && out, 1, "XTTS conditioning: NULL argument");
  TTS_REQUIRE(B >= 1, 1, "XTTS conditioning: the batch must not be empty");
  TTS_REQUIRE(B <= kCondMaxBatch, 3, "XTTS conditioning: at most " + std::to_string(kCondMaxBatch) + " rows");
  const int T = num_frames(N);
  TTS_REQUIRE(stft_->num_frames(N) == T, 1, "internal: XTTS conditioning frame count mismatch");
  const int K = cfg_.n_fft / 2 + 1, M = cfg_.spec_dim;
  DeviceGuard g(device_);
  ws_.grow(device_, (size_t)B * K * T * sizeof(float), "XTTS conditioning workspace");
  float* power = ws_.as<>();
  stft_->forward(wav, B, N, 0, power, s, prof);
  run(prof, s, "mel_log_norm", 2.0 * B * K * M * T, 4.0 * B * T * (K + M),
      [&] { launch_cond_logmel(power, B, K, M, T, fb_, reinterpret_cast<const int*>(fb_range_), mel_norms, out, s); });
}

void XttsCond::conv(const char* name, const PackedConv& cv, const float* in, float* out, const float* res, int B, int T,
                    hipStream_t s, Profiler* prof) const {
  const double P = (double)B * T;
  run(prof, s, name, 2.0 * P * cv.Cout * cv.Cin,
      4.0 * (P * (cv.Cin + cv.Cout + (res ? cv.Cout : 0)) + (double)cv.Cin * cv.Cout),
      [&] { run_conv1(mode_, cv, in, out, res, B, T, s); });
}

void XttsCond::style_emb(const float* mel, int B, int T, float* out, hipStream_t s, Profiler* prof) {
  TTS_REQUIRE(mel && out, 1, "XTTS conditioning: NULL argument");
  TTS_REQUIRE(B >= 1 && T >= 1, 1, "XTTS conditioning: the batch and the frame count must be >= 1");
  TTS_REQUIRE(B <= kCondMaxBatch, 3, "XTTS conditioning: at most " + std::to_string(kCondMaxBatch) + " rows");
  TTS_REQUIRE(L_ + (int64_t)T <= kCondMaxKeys, 3,
              "XTTS conditioning: num_latents + frames must not exceed " + std::to_string(kCondMaxKeys));
  DeviceGuard g(device_);
  const int E = E_, L = L_, dh = cfg_.perceiver_dim_head, PH = cfg_.perceiver_heads;
  // workspace: encoder planes X, XN, A [B][E][T] and QKV [B][3E][T]; the context's K | V [B][2 inner][T];
  // latent planes LA, LB [B][E][L], Q, ATT [B][inner][L], KVL [B][2 inner][L], GG [B][I][L]
  const size_t pe = al((size_t)B * E * T), pkv = al((size_t)B * 2 * inner_ * T), pl = al((size_t)B * E * L);
  const size_t pq = al((size_t)B * inner_ * L);
  const size_t total = 3 * pe + 3 * pe + pkv + 2 * pl + 2 * pq + 2 * pq + al((size_t)B * I_ * L);
  ws_.grow(device_, total * sizeof(float), "XTTS conditioning workspace");
  float* p = ws_.as<>();
  float* X = p; p += pe;
  float* XN = p; p += pe;
  float* A = p; p += pe;
  float* QKV = p; p += 3 * pe;
  float* KVC = p; p += pkv;
  float* LA = p; p += pl;
  float* LB = p; p += pl;
  float* Q = p; p += pq;
  float* ATT = p; p += pq;
  float* KVL = p; p += 2 * pq;
  float* GG = p;

  const double PT = (double)B * T;
  conv("init", init_, mel, X, nullptr, B, T, s, prof);
  for (const Block& b : blocks_) {
    run(prof, s, "group_norm", 8.0 * PT * E, 12.0 * PT * E,
        [&] { launch_cond_groupnorm(X, b.gn_g, b.gn_b, B, E, T, G_, kGnEps, XN, s); });
    conv("qkv", b.qkv, XN, QKV, nullptr, B, T, s, prof);
    run(prof, s, "attention", 4.0 * PT * T * E, 16.0 * PT * E,
        [&] { launch_mha_wide(mode_, QKV, nullptr, A, B, E, H_, T, s); });
    conv("proj_out", b.proj, A, X, XN, B, T, s, prof);  // xn + proj_out(a): the block's output replaces its input
  }
  float *lat = LA, *other = LB;
  const double PL = (double)B * L;
  run(prof, s, "latents", 0.0, 4.0 * (PL + L) * E, [&] { launch_cond_broadcast(lat0_, B, (int64_t)E * L, LA, s); });
  for (const Layer& l : layers_) {
    const double wb = bf16_ ? 2.0 : 4.0;
    auto product = [&](const char* name, const float* w, const float* bias, const float* in, const float* res, int R,
                       int K, int geglu, float* o) {
      run(prof, s, name, 2.0 * PL * R * K, wb * R * K + 4.0 * PL * (K + R), [&] {
        launch_cond_product(w, bf16_, bias, in, res, B, R, K, L, geglu, o, s);
      });
    };
    product("to_q", l.w_q, nullptr, lat, nullptr, inner_, E, 0, Q);
    product("to_kv_latents", l.w_kv, nullptr, lat, nullptr, 2 * inner_, E, 0, KVL);
    conv("to_kv_context", l.to_kv, X, KVC, nullptr, B, T, s, prof);
    run(prof, s, "cross_attention", 4.0 * PL * (L + T) * inner_, 8.0 * B * inner_ * (L + T) * (double)L,
        [&] { launch_cond_cross_attn(Q, KVL, KVC, B, PH, dh, L, T, ATT, s); });
    product("to_out", l.w_out, nullptr, ATT, lat, E, inner_, 0, other);
    std::swap(lat, other);
    product("ff_in_geglu", l.w_ff0, l.b_ff0, lat, nullptr, 2 * I_, E, 1, GG);
    product("ff_out", l.w_ff2, l.b_ff2, GG, lat, E, I_, 0, other);
    std::swap(lat, other);
  }
  run(prof, s, "rms_norm", 4.0 * PL * E, 8.0 * PL * E, [&] { launch_cond_rmsnorm(lat, gamma_, B, E, L, out, s); });
}

// ------------------------------------------------------------------------------------ kernel-test op
void op_cond_ff(const float* d_x, int B, int E, int I, int L, const float* w0, const float* b0, const float* w2,
                const float* b2, int math_mode, float* d_out, hipStream_t s) {
  TTS_REQUIRE(d_x && w0 && b0 && w2 && b2 && d_out, 1, "NULL argument");
  TTS_REQUIRE(B >= 1 && E >= 1 && I >= 1 && L >= 1, 1, "bad feed-forward shape");
  TTS_REQUIRE(math_mode >= MATH_FP32 && math_mode <= MATH_LAST, 1, "unknown math_mode");
  TTS_REQUIRE(B <= kCondMaxBatch && E <= 4096 && I <= 16384 && L <= kCondMaxLatents, 3,
              "feed-forward: shape outside the limits");
  TTS_REQUIRE(d_x != d_out, 1, "feed-forward: the output must not alias the input");
  const bool bf16 = math_mode == MATH_BF16;
  int dev = 0;
  TTS_HIP_CHECK(hipGetDevice(&dev));
  HostArena arena;
  float *dw0 = nullptr, *db0 = nullptr, *dw2 = nullptr, *db2 = nullptr;
  pack_cond_rows(w0, (int64_t)2 * I * E, bf16, arena.at(arena.alloc((size_t)cond_rows_numel((int64_t)2 * I * E, bf16), &dw0)));
  arena.put(b0, (size_t)2 * I, &db0);
  pack_cond_rows(w2, (int64_t)E * I, bf16, arena.at(arena.alloc((size_t)cond_rows_numel((int64_t)E * I, bf16), &dw2)));
  arena.put(b2, (size_t)E, &db2);
  DeviceBuffer wbuf, ws;
  arena.upload(dev, wbuf);
  ws.grow(dev, al((size_t)B * I * L) * sizeof(float), "operand");
  float* GG = ws.as<>();
  launch_cond_product(dw0, bf16, db0, d_x, nullptr, B, 2 * I, E, L, 1, GG, s);
  launch_cond_product(dw2, bf16, db2, GG, d_x, B, E, I, L, 0, d_out, s);
  TTS_HIP_CHECK(hipStreamSynchronize(s));  // the operand buffers are freed on return
}

// ------------------------------------------------------------------------------------------ resampler
Resampler::Resampler(int orig_freq, int new_freq, int device) : device_(device) {
  TTS_REQUIRE(orig_freq >= 1 && new_freq >= 1, 1, "resample: the sample rates must be positive");
  const int g = std::gcd(orig_freq, new_freq);
  o_ = orig_freq / g;
  n_ = new_freq / g;
  TTS_REQUIRE(o_ <= kResampleMaxFactor && n_ <= kResampleMaxFactor, 3,
              "resample: orig_freq / gcd and new_freq / gcd must not exceed " + std::to_string(kResampleMaxFactor));
  int dev_count = 0;
  TTS_HIP_CHECK(hipGetDeviceCount(&dev_count));
  TTS_REQUIRE(device >= 0 && device < dev_count, 1, "resample: bad device index");
  w_ = resample_width(o_, n_);
  std::vector<float> table((size_t)(2 * w_ + o_) * n_);
  build_resample_table(o_, n_, table.data());
  table_.grow(device_, table.size() * sizeof(float), "resample table");
  DeviceGuard dg(device_);
  TTS_HIP_CHECK(hipMemcpy(table_.as<>(), table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
}

int64_t Resampler::num_samples(int64_t N) const {
  TTS_REQUIRE(N >= 1, 1, "resample: the input must not be empty");
  TTS_REQUIRE(N < (int64_t)1 << 31 && (N * n_ + o_ - 1) / o_ < (int64_t)1 << 31, 3,
              "resample: rows of fewer than 2^31 samples");
  return (N * n_ + o_ - 1) / o_;
}

void Resampler::forward(const float* x, int B, int64_t N, float* y, hipStream_t s) {
  TTS_REQUIRE(x && y, 1, "resample: NULL argument");
  TTS_REQUIRE(B >= 1, 1, "resample: the batch must not be empty");
  const int64_t Nout = num_samples(N);
  DeviceGuard dg(device_);
  launch_resample(x, B, N, table_.as<>(), o_, n_, w_, Nout, y, s);
}

}  // namespace tts
