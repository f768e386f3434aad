// ResNetSpeakerEncoder executor (tts_speaker_encoder_*): validation, weight inventory, BatchNorm
// folding into the convs' epilogues, packing and the launch sequence.
//   front end (use_torch_spec): pre-emphasis -> centred STFT, |X|^2 (stft.hpp) -> mel filterbank
//   log (log_input) + instance norm                                         -> x0 [B][1][input_dim][T]
//   stem: conv1 + bias -> ReLU -> bn1 (one Conv2d launch)
//   per SEBasicBlock: conv1 -> ReLU -> bn1 | conv2 -> bn2, leaving the SE partial sums | downsample
//     conv + BatchNorm where the block has one | SE gate | relu(h gate + residual): 4 or 5 launches
//   head: attention.0 + ReLU + BatchNorm1d | attention.3 (both 1x1: the Conv2d kernel on [D][1][T']) |
//     softmax over T' + SAP / ASP | fc | L2 norm
// The downsample conv is a launch of its own, not extra k-steps of conv2: the SE gate multiplies
// conv2's part only and is known only after all of conv2's plane has been pooled, so the sum
// conv2 gate + downsample cannot be formed inside conv2's launch either way.
#include "speaker_encoder.hpp"

#include <algorithm>
#include <cmath>

#include "arena.hpp"

namespace tts {

namespace {
constexpr int kAttC = 128;  // attention bottleneck (fixed in the reference)
constexpr double kBnEps = 1e-5;

struct Dims {
  int F, T;
};
int block_stride(int layer, int i) { return (layer > 0 && i == 0) ? 2 : 1; }
bool block_has_down(const TtsSpeakerEncoderCfg& c, int layer, int i) {
  const int cin = i == 0 ? (layer == 0 ? c.num_filters[0] : c.num_filters[layer - 1]) : c.num_filters[layer];
  return block_stride(layer, i) != 1 || cin != c.num_filters[layer];
}
int n_freqs(const TtsSpeakerEncoderCfg& c) { return c.fft_size / 2 + 1; }
TtsStftCfg stft_cfg(const TtsSpeakerEncoderCfg& c) {
  TtsStftCfg s{};
  s.n_fft = c.fft_size;
  s.hop_length = c.hop_length;
  s.win_length = c.win_length;
  s.math_mode = MATH_FP32_X6;  // the front end is fp32-faithful in every mode
  return s;
}
}  // namespace

void speaker_encoder_validate(const TtsSpeakerEncoderCfg& c) {
  TTS_REQUIRE(c.math_mode >= MATH_FP32 && c.math_mode <= MATH_LAST, 1, "speaker encoder: unknown math_mode");
  TTS_REQUIRE(c.encoder_type == TTS_SPK_SAP || c.encoder_type == TTS_SPK_ASP, 1,
              "speaker encoder: encoder_type must be SAP or ASP");
  TTS_REQUIRE(c.input_dim >= 1 && c.proj_dim >= 1, 1, "speaker encoder: input_dim and proj_dim must be positive");
  int nblocks = 0;
  for (int l = 0; l < 4; ++l) {
    TTS_REQUIRE(c.layers[l] >= 1 && c.num_filters[l] >= 1, 1, "speaker encoder: layers and num_filters must be positive");
    nblocks += c.layers[l];
  }
  TTS_REQUIRE(c.input_dim % 8 == 0 && c.input_dim <= 512, 3,
              "speaker encoder: input_dim must be a multiple of 8 in [8, 512]");
  for (int l = 0; l < 4; ++l)
    TTS_REQUIRE(c.num_filters[l] % 8 == 0 && c.num_filters[l] <= TTS_SPK_MAX_FILTERS, 3,
                "speaker encoder: num_filters must be multiples of 8 in [8, 256]");
  TTS_REQUIRE(nblocks <= 64, 3, "speaker encoder: at most 64 residual blocks");
  TTS_REQUIRE(c.proj_dim <= 4096, 3, "speaker encoder: proj_dim must lie in [1, 4096]");
  TTS_REQUIRE((int64_t)c.num_filters[3] * (c.input_dim / 8) <= kConv2dMaxCout, 3,
              "speaker encoder: num_filters[3] * input_dim / 8 must not exceed 4096");
  if (c.use_torch_spec) {
    TTS_REQUIRE(c.fft_size >= 1 && c.hop_length >= 1 && c.win_length >= 1, 1,
                "speaker encoder: fft_size, win_length and hop_length must be positive");
    stft_validate(stft_cfg(c));
  }
}

std::vector<int64_t> speaker_encoder_weight_shapes(const TtsSpeakerEncoderCfg& c) {
  speaker_encoder_validate(c);
  std::vector<int64_t> s;
  auto bn = [&](int64_t n) {
    for (int i = 0; i < 4; ++i) s.push_back(n);
  };
  if (c.use_torch_spec) {
    s.push_back(2);
    s.push_back(c.win_length);
    s.push_back((int64_t)n_freqs(c) * c.input_dim);
  }
  const int64_t F0 = c.num_filters[0];
  s.push_back(F0 * 9);
  s.push_back(F0);
  bn(F0);
  int64_t cin = F0;
  for (int l = 0; l < 4; ++l) {
    const int64_t C = c.num_filters[l];
    for (int i = 0; i < c.layers[l]; ++i) {
      s.push_back(C * cin * 9);
      bn(C);
      s.push_back(C * C * 9);
      bn(C);
      s.push_back((C / 8) * C);
      s.push_back(C / 8);
      s.push_back(C * (C / 8));
      s.push_back(C);
      if (block_has_down(c, l, i)) {
        s.push_back(C * cin);
        bn(C);
      }
      cin = C;
    }
  }
  const int64_t D = (int64_t)c.num_filters[3] * (c.input_dim / 8);
  s.push_back(kAttC * D);
  s.push_back(kAttC);
  bn(kAttC);
  s.push_back(D * kAttC);
  s.push_back(D);
  s.push_back((int64_t)c.proj_dim * (c.encoder_type == TTS_SPK_ASP ? 2 * D : D));
  s.push_back(c.proj_dim);
  return s;
}

SpeakerEncoder::SpeakerEncoder(const TtsSpeakerEncoderCfg& cfg, const float* const* hw, int device)
    : cfg_(cfg), device_(device) {
  speaker_encoder_validate(cfg);
  mode_ = conv2d_mode(cfg.math_mode);
  const auto shapes = speaker_encoder_weight_shapes(cfg);
  for (size_t i = 0; i < shapes.size(); ++i)
    TTS_REQUIRE(hw[i] != nullptr, 1, "weight pointer " + std::to_string(i) + " is NULL");
  int dev_count = 0;
  TTS_HIP_CHECK(hipGetDeviceCount(&dev_count));
  TTS_REQUIRE(device >= 0 && device < dev_count, 1, "speaker encoder: bad device index");
  D_ = cfg.num_filters[3] * (cfg.input_dim / 8);

  HostArena arena;
  size_t wi = 0;
  // conv weights w, optional bias, optional BatchNorm (weight, bias, running_mean, running_var) folded
  // into the epilogue's scale / shift in fp64
  auto put_conv = [&](Conv& cv, const float* w, const float* bias, const float* const* bnp) {
    cv.numel16 = packed_conv2d_numel16(mode_, cv.Cout, cv.Cin, cv.KS);
    const size_t oa = arena.alloc((size_t)cv.numel16 / 2, &cv.a);
    pack_conv2d(mode_, w, cv.Cout, cv.Cin, cv.KS, reinterpret_cast<uint16_t*>(arena.at(oa)));
    std::vector<float> sc(cv.Cout, 1.f), sh(cv.Cout, 0.f);
    if (bnp) {
      for (int c = 0; c < cv.Cout; ++c) {
        const double k = (double)bnp[0][c] / std::sqrt((double)bnp[3][c] + kBnEps);
        sc[c] = (float)k;
        sh[c] = (float)((double)bnp[1][c] - (double)bnp[2][c] * k);
      }
    }
    const size_t nb = (size_t)32 * conv2d_mblocks(cv.Cout);
    const size_t ob = arena.alloc(nb, &cv.bias), os = arena.alloc(nb, &cv.scale), ot = arena.alloc(nb, &cv.shift);
    // at() pointers are valid until the next alloc: fetch them after the last one
    pack_conv2d_epilogue(bias, sc.data(), sh.data(), cv.Cout, arena.at(ob), arena.at(os), arena.at(ot));
  };

  if (cfg.use_torch_spec) {
    arena.put(hw[wi], 2, &filt_);
    stft_.reset(new Stft(stft_cfg(cfg), hw[wi + 1], device, /*center=*/true, /*power=*/true));
    arena.put(hw[wi + 2], (size_t)n_freqs(cfg) * cfg.input_dim, &fb_);
    wi += 3;
  }
  stem_.Cin = 1; stem_.Cout = cfg.num_filters[0]; stem_.KS = 3; stem_.stride = 1; stem_.relu = 1;
  stem_.name = "stem_c" + std::to_string(stem_.Cout);
  put_conv(stem_, hw[wi], hw[wi + 1], hw + wi + 2);
  wi += 6;
  int cin = cfg.num_filters[0];
  // the arena keeps the addresses of the blocks' pointer members until upload() patches them: the
  // vector must not reallocate while it is filled
  blocks_.reserve((size_t)cfg.layers[0] + cfg.layers[1] + cfg.layers[2] + cfg.layers[3]);
  for (int l = 0; l < 4; ++l) {
    const int C = cfg.num_filters[l];
    for (int i = 0; i < cfg.layers[l]; ++i) {
      Block bl;
      bl.C = C;
      const int st = block_stride(l, i);
      const std::string tag = "_c" + std::to_string(C) + (st == 2 ? "_s2" : "");
      bl.c1.Cin = cin; bl.c1.Cout = C; bl.c1.KS = 3; bl.c1.stride = st; bl.c1.relu = 1;
      bl.c1.name = "conv1" + tag;
      bl.c2.Cin = C; bl.c2.Cout = C; bl.c2.KS = 3; bl.c2.stride = 1; bl.c2.relu = 0;
      bl.c2.name = "conv2_c" + std::to_string(C);
      blocks_.push_back(bl);
      Block& b = blocks_.back();
      put_conv(b.c1, hw[wi], nullptr, hw + wi + 1);
      put_conv(b.c2, hw[wi + 5], nullptr, hw + wi + 6);
      arena.put(hw[wi + 10], (size_t)(C / 8) * C, &b.w0);
      arena.put(hw[wi + 11], (size_t)(C / 8), &b.b0);
      arena.put(hw[wi + 12], (size_t)C * (C / 8), &b.w2);
      arena.put(hw[wi + 13], (size_t)C, &b.b2);
      wi += 14;
      b.has_down = block_has_down(cfg, l, i);
      if (b.has_down) {
        b.down.Cin = cin; b.down.Cout = C; b.down.KS = 1; b.down.stride = st; b.down.relu = 0;
        b.down.name = "downsample" + tag;
        put_conv(b.down, hw[wi], nullptr, hw + wi + 1);
        wi += 5;
      }
      cin = C;
    }
  }
  att1_.Cin = D_; att1_.Cout = kAttC; att1_.KS = 1; att1_.stride = 1; att1_.relu = 1;
  att1_.name = "attention0_c" + std::to_string(D_);
  put_conv(att1_, hw[wi], hw[wi + 1], hw + wi + 2);
  wi += 6;
  att2_.Cin = kAttC; att2_.Cout = D_; att2_.KS = 1; att2_.stride = 1; att2_.relu = 0;
  att2_.name = "attention3_c" + std::to_string(D_);
  put_conv(att2_, hw[wi], hw[wi + 1], nullptr);
  wi += 2;
  const int DP = cfg.encoder_type == TTS_SPK_ASP ? 2 * D_ : D_;
  arena.put(hw[wi], (size_t)cfg.proj_dim * DP, &fc_w_);
  arena.put(hw[wi + 1], (size_t)cfg.proj_dim, &fc_b_);
  wi += 2;
  TTS_REQUIRE(wi == shapes.size(), 1, "internal: speaker encoder weight inventory mismatch");
  arena.upload(device_, arena_);
}

int SpeakerEncoder::num_frames(int64_t n) const {
  TTS_REQUIRE(n >= 1, 1, "speaker encoder: the input must not be empty");
  int64_t T = n;
  if (cfg_.use_torch_spec) {
    TTS_REQUIRE(n >= cfg_.fft_size / 2 + 1, 3,
                "speaker encoder: the wav must have at least fft_size / 2 + 1 = " + std::to_string(cfg_.fft_size / 2 + 1) +
                    " samples (the centred STFT's reflect padding)");
    TTS_REQUIRE(n * 4 < (int64_t)1 << 31, 3, "speaker encoder: a wav row must stay below 2 GiB");
    T = 1 + n / cfg_.hop_length;
  }
  TTS_REQUIRE(T <= TTS_SPK_MAX_FRAMES, 3,
              "speaker encoder: at most " + std::to_string(TTS_SPK_MAX_FRAMES) + " frames per forward");
  return (int)T;
}

void SpeakerEncoder::check_shape(int B, int T) const {
  TTS_REQUIRE(B >= 1, 1, "speaker encoder: the batch must not be empty");
  TTS_REQUIRE(B <= TTS_SPK_MAX_BATCH, 3,
              "speaker encoder: at most " + std::to_string(TTS_SPK_MAX_BATCH) + " rows per forward");
  // every conv's own limits (planes below 2 GiB, grid ranges), before anything is launched
  float dummy = 0.f;
  auto chk = [&](const Conv& c, int F, int Tc) {
    Conv2dArgs a{};
    a.x = &dummy; a.y = &dummy + 1;
    a.Cin = c.Cin; a.Cout = c.Cout; a.F = F; a.T = Tc; a.KS = c.KS; a.stride = c.stride;
    conv2d_check(a, B);
  };
  int F = cfg_.input_dim, Tc = T;
  chk(stem_, F, Tc);
  for (const Block& b : blocks_) {
    chk(b.c1, F, Tc);
    if (b.has_down) chk(b.down, F, Tc);
    F = conv2d_out(F, b.c1.stride);
    Tc = conv2d_out(Tc, b.c1.stride);
    chk(b.c2, F, Tc);
  }
  chk(att1_, 1, Tc);
  chk(att2_, 1, Tc);
}

void SpeakerEncoder::run_conv(const Conv& c, const float* x, int B, int F, int T, float* y, float* pool, hipStream_t s,
                              Profiler* prof) const {
  Conv2dArgs a{};
  a.x = x; a.y = y; a.a = c.a; a.bias = c.bias; a.scale = c.scale; a.shift = c.shift; a.pool = pool;
  a.a_bytes = (unsigned)(c.numel16 * 2);
  a.Cin = c.Cin; a.Cout = c.Cout; a.F = F; a.T = T; a.KS = c.KS; a.stride = c.stride; a.relu = c.relu;
  const double Fo = conv2d_out(F, c.stride), To = conv2d_out(T, c.stride);
  const double outs = (double)B * c.Cout * Fo * To;
  run(prof, s, c.name.c_str(), 2.0 * outs * c.Cin * c.KS * c.KS,
      ((double)B * c.Cin * F * T + outs) * 4 + (double)c.numel16 * 2, [&] { launch_conv2d(mode_, a, B, s); });
}

void SpeakerEncoder::features(const float* x, int B, int64_t n, float* feat, hipStream_t s, Profiler* prof) {
  TTS_REQUIRE(x && feat, 1, "speaker encoder: NULL argument");
  const int T = num_frames(n);
  check_shape(B, T);
  const int M = cfg_.input_dim;
  DeviceGuard g(device_);
  const float* src = x;
  if (cfg_.use_torch_spec) {
    const int K = n_freqs(cfg_);
    TTS_REQUIRE(stft_->num_frames(n) == T, 1, "internal: speaker encoder frame count mismatch");
    const size_t need = ((size_t)B * n + (size_t)B * K * T + (size_t)B * M * T) * sizeof(float);
    // the front end's scratch lives at the start of the workspace; forward() sizes it for the trunk too
    ws_.grow(device_, need, "speaker encoder workspace");
    float* wavp = ws_.as<>();
    float* power = wavp + (size_t)B * n;
    float* mel = power + (size_t)B * K * T;
    run(prof, s, "preemphasis", 2.0 * B * n, 8.0 * B * n, [&] { launch_spk_preemph(x, B, n, filt_, wavp, s); });
    stft_->forward(wavp, B, n, 0, power, s, prof);
    run(prof, s, "mel_filterbank", 2.0 * B * K * M * T, 4.0 * B * T * (K + M),
        [&] { launch_spk_mel(power, B, K, M, T, fb_, mel, s); });
    src = mel;
  }
  run(prof, s, "log_instance_norm", 8.0 * B * M * T, 8.0 * B * M * T,
      [&] { launch_spk_instnorm(src, B, M, T, cfg_.log_input, feat, s); });
}

void SpeakerEncoder::forward(const float* x, int B, int64_t n, int l2_norm, float* out, hipStream_t s, Profiler* prof) {
  TTS_REQUIRE(x && out, 1, "speaker encoder: NULL argument");
  const int T = num_frames(n);
  check_shape(B, T);
  const int M = cfg_.input_dim;
  DeviceGuard g(device_);

  // workspace: [front end scratch | x0 | 5 trunk planes | SE partial sums | gates | head]
  size_t front = 0;
  if (cfg_.use_torch_spec) front = (size_t)B * n + (size_t)B * n_freqs(cfg_) * T + (size_t)B * M * T;
  size_t plane = (size_t)stem_.Cout * M * T, pool_n = 0;
  {
    int F = M, Tc = T;
    for (const Block& b : blocks_) {
      F = conv2d_out(F, b.c1.stride);
      Tc = conv2d_out(Tc, b.c1.stride);
      plane = std::max(plane, (size_t)b.C * F * Tc);
      pool_n = std::max(pool_n, (size_t)b.C * F * conv2d_pool_slots(Tc));
    }
  }
  int Tp = T;
  for (const Block& b : blocks_) Tp = conv2d_out(Tp, b.c1.stride);
  const int DP = cfg_.encoder_type == TTS_SPK_ASP ? 2 * D_ : D_;
  const size_t feat_n = HostArena::align((size_t)B * M * T);
  plane = HostArena::align((size_t)B * plane);
  pool_n = HostArena::align((size_t)B * pool_n);
  const size_t gate_n = HostArena::align((size_t)B * TTS_SPK_MAX_FILTERS);
  const size_t att1_n = HostArena::align((size_t)B * kAttC * Tp), att2_n = HostArena::align((size_t)B * D_ * Tp);
  const size_t pooled_n = HostArena::align((size_t)B * DP);
  front = HostArena::align(front);
  const size_t total = front + feat_n + 5 * plane + pool_n + gate_n + att1_n + att2_n + pooled_n;
  ws_.grow(device_, total * sizeof(float), "speaker encoder workspace");

  float* p = ws_.as<>() + front;
  float* feat = p; p += feat_n;
  float* buf[5];
  for (auto& q : buf) { q = p; p += plane; }
  float* pool = p; p += pool_n;
  float* gate = p; p += gate_n;
  float* att1 = p; p += att1_n;
  float* att2 = p; p += att2_n;
  float* pooled = p;

  features(x, B, n, feat, s, prof);  // its scratch is the first `front` floats: already large enough

  int F = M, Tc = T;
  float* cur = buf[0];
  run_conv(stem_, feat, B, F, Tc, cur, nullptr, s, prof);
  for (const Block& b : blocks_) {
    // the four planes that are not the block's input
    float* fr[4];
    int k = 0;
    for (float* q : buf)
      if (q != cur) fr[k++] = q;
    float *h1 = fr[0], *h2 = fr[1], *res = fr[2], *nxt = fr[3];
    const int Fo = conv2d_out(F, b.c1.stride), To = conv2d_out(Tc, b.c1.stride);
    run_conv(b.c1, cur, B, F, Tc, h1, nullptr, s, prof);
    run_conv(b.c2, h1, B, Fo, To, h2, pool, s, prof);
    const float* r = cur;
    if (b.has_down) {
      run_conv(b.down, cur, B, F, Tc, res, nullptr, s, prof);
      r = res;
    }
    const int nparts = Fo * conv2d_pool_slots(To);
    run(prof, s, "se_gate", 2.0 * B * (nparts * b.C + 2.0 * b.C * (b.C / 8)), 4.0 * B * b.C * nparts, [&] {
      launch_spk_se_gate(pool, B, b.C, nparts, (float)Fo * (float)To, b.w0, b.b0, b.w2, b.b2, gate, s);
    });
    const int64_t P = (int64_t)Fo * To;
    run(prof, s, "se_scale_add_relu", 3.0 * B * b.C * P, 12.0 * B * b.C * P,
        [&] { launch_spk_se_apply(h2, r, gate, B, b.C, P, nxt, s); });
    cur = nxt;
    F = Fo;
    Tc = To;
  }
  // head: cur is [B][C3][F'][T'] = [B][D][T']
  TTS_REQUIRE(blocks_.back().C * F == D_ && Tc == Tp, 1, "internal: speaker encoder head shape mismatch");
  run_conv(att1_, cur, B, 1, Tc, att1, nullptr, s, prof);
  run_conv(att2_, att1, B, 1, Tc, att2, nullptr, s, prof);
  const int asp = cfg_.encoder_type == TTS_SPK_ASP;
  run(prof, s, "softmax_pool", 10.0 * B * D_ * Tc, 8.0 * B * D_ * Tc,
      [&] { launch_spk_pool(cur, att2, B, D_, Tc, asp, pooled, s); });
  run(prof, s, "fc", 2.0 * B * DP * cfg_.proj_dim, 4.0 * ((double)DP * cfg_.proj_dim + B * (DP + cfg_.proj_dim)),
      [&] { launch_spk_fc(pooled, B, DP, cfg_.proj_dim, fc_w_, fc_b_, out, s); });
  if (l2_norm)
    run(prof, s, "l2_norm", 3.0 * B * cfg_.proj_dim, 8.0 * B * cfg_.proj_dim,
        [&] { launch_spk_l2norm(out, B, cfg_.proj_dim, s); });
}

}  // namespace tts
