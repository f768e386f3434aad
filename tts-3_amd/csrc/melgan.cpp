// MelGAN-family generator executor (tts_melgan_*): validation, weight inventory, packing and the
// launch sequence.  Kernels: kernels_melgan.hip (residual block, tail + PQMF, input gather); the
// first conv and the upsamplers run on the split conv kernels (kernels_conv_split.hip).
#include "melgan.hpp"

#include <algorithm>

namespace tts {

namespace {
int run_mode(int math_mode) { return math_mode == MATH_BF16 ? MATH_BF16 : MATH_FP32_X6; }
int ipow(int b, int e) {
  int r = 1;
  for (int i = 0; i < e; ++i) r *= b;
  return r;
}
}  // namespace

void melgan_validate(const TtsMelganCfg& c) {
  TTS_REQUIRE(c.math_mode >= MATH_FP32 && c.math_mode <= MATH_LAST, 1, "melgan: unknown math_mode");
  TTS_REQUIRE(c.in_channels >= 1 && c.out_channels >= 1 && c.base_channels >= 1, 1, "melgan: channel counts must be positive");
  TTS_REQUIRE(c.proj_kernel >= 1 && c.proj_kernel % 2 == 1, 1, "melgan: proj_kernel must be odd ((proj_kernel - 1) % 2 == 0)");
  TTS_REQUIRE(c.res_kernel >= 1 && c.res_kernel % 2 == 1, 1, "melgan: res_kernel must be odd");
  TTS_REQUIRE(c.num_ups >= 1 && c.num_ups <= TTS_MAX_UPSAMPLES, 1, "melgan: num_ups must lie in [1, 8]");
  TTS_REQUIRE(c.num_res_blocks >= 1, 1, "melgan: num_res_blocks must be positive");
  TTS_REQUIRE((c.base_channels >> c.num_ups) >= 1, 1, "melgan: base_channels >> num_ups must be at least 1");
  TTS_REQUIRE(c.pqmf_bands >= 0, 1, "melgan: pqmf_bands must not be negative");
  for (int i = 0; i < c.num_ups; ++i) {
    const int u = c.upsample_factors[i];
    TTS_REQUIRE(u >= 1, 1, "melgan: upsample factors must be positive");
    TTS_REQUIRE(u == 2 || u == 4 || u == 8, 3, "melgan: upsample factors must be 2, 4 or 8");
  }
  TTS_REQUIRE(c.proj_kernel == 3 || c.proj_kernel == 5 || c.proj_kernel == 7 || c.proj_kernel == 11, 3,
              "melgan: proj_kernel must be 3, 5, 7 or 11");
  TTS_REQUIRE(c.res_kernel == 3, 3, "melgan: res_kernel must be 3");
  TTS_REQUIRE(c.num_res_blocks <= 4, 3, "melgan: at most 4 residual blocks per stack (dilation 27)");
  TTS_REQUIRE(c.base_channels <= 2 * kMelganMaxC, 3, "melgan: base_channels must not exceed 512");
  TTS_REQUIRE(c.out_channels <= kMelganTailMaxCo, 3, "melgan: out_channels must not exceed 4");
  if (c.pqmf_bands > 0) {
    TTS_REQUIRE(c.pqmf_bands == c.out_channels && c.pqmf_bands >= 2, 1, "melgan: pqmf_bands must equal out_channels (>= 2)");
    TTS_REQUIRE(c.pqmf_taps >= 2 && c.pqmf_taps % 2 == 0 && c.pqmf_taps <= 126, 3,
                "melgan: pqmf_taps must be even and lie in [2, 126]");
  }
}

std::vector<int64_t> melgan_weight_shapes(const TtsMelganCfg& c) {
  melgan_validate(c);
  std::vector<int64_t> s;
  s.push_back((int64_t)c.base_channels * c.in_channels * c.proj_kernel);
  s.push_back(c.base_channels);
  for (int i = 0; i < c.num_ups; ++i) {
    const int64_t Ci = c.base_channels >> i, Co = c.base_channels >> (i + 1);
    s.push_back(Ci * Co * 2 * c.upsample_factors[i]);
    s.push_back(Co);
    for (int j = 0; j < c.num_res_blocks; ++j) {
      s.push_back(Co * Co * c.res_kernel);
      s.push_back(Co);
      s.push_back(Co * Co);
      s.push_back(Co);
    }
    for (int j = 0; j < c.num_res_blocks; ++j) {
      s.push_back(Co * Co);
      s.push_back(Co);
    }
  }
  s.push_back((int64_t)c.out_channels * (c.base_channels >> c.num_ups) * c.proj_kernel);
  s.push_back(c.out_channels);
  if (c.pqmf_bands > 0) s.push_back((int64_t)c.pqmf_bands * (c.pqmf_taps + 1));
  return s;
}

void melgan_check_length(const TtsMelganCfg& c, int64_t T, int pad) {
  TTS_REQUIRE(T >= 1 && pad >= 0, 1, "melgan: T must be positive and pad non-negative");
  const int P = (c.proj_kernel - 1) / 2;
  int64_t len = T + 2 * (int64_t)pad;
  TTS_REQUIRE(P < len, 1,
              "melgan: reflection pad " + std::to_string(P) + " of the first conv must be smaller than its input length " +
                  std::to_string(len));
  TTS_REQUIRE((int64_t)std::max(c.in_channels, c.base_channels) * (len + 2 * P) * 4 < (int64_t)1 << 31, 3,
              "melgan: a batch item's plane exceeds the 32-bit buffer range (2 GiB)");
  for (int i = 0; i < c.num_ups; ++i) {
    len *= c.upsample_factors[i];
    TTS_REQUIRE((int64_t)(c.base_channels >> i) * len * 4 < (int64_t)1 << 31, 3,
                "melgan: a batch item's plane exceeds the 32-bit buffer range (2 GiB)");
    for (int j = 0; j < c.num_res_blocks; ++j) {
      const int d = ((c.res_kernel - 1) / 2) * ipow(c.res_kernel, j);
      TTS_REQUIRE(d < len, 1,
                  "melgan: reflection pad " + std::to_string(d) + " of residual block " + std::to_string(j) + " in stack " +
                      std::to_string(i) + " must be smaller than its input length " + std::to_string(len));
    }
  }
  TTS_REQUIRE(P < len, 1, "melgan: reflection pad of the last conv must be smaller than its input length");
  TTS_REQUIRE((int64_t)std::max(1, c.pqmf_bands) * c.out_channels * len * 4 < (int64_t)1 << 31, 3,
              "melgan: the output exceeds the 32-bit buffer range (2 GiB) per item");
}

Melgan::Melgan(const TtsMelganCfg& cfg, const float* const* hw, int device) : cfg_(cfg), device_(device) {
  melgan_validate(cfg);
  mode_ = run_mode(cfg.math_mode);
  const auto shapes = melgan_weight_shapes(cfg);
  for (size_t i = 0; i < shapes.size(); ++i)
    TTS_REQUIRE(hw[i] != nullptr, 1, "weight pointer " + std::to_string(i) + " is NULL");
  int dev_count = 0;
  TTS_HIP_CHECK(hipGetDeviceCount(&dev_count));
  TTS_REQUIRE(device >= 0 && device < dev_count, 1, "melgan: bad device index");

  const int base = cfg.base_channels, n = cfg.num_ups, NB = cfg.num_res_blocks;
  // arena order: first conv, upsamplers, residual blocks, tail, PQMF filters
  HostArena arena;
  size_t wi = 0;
  // first conv (pad 0 on the gathered input)
  pre_.Cin = cfg.in_channels; pre_.Cout = base; pre_.K = cfg.proj_kernel;
  pre_.tile = conv_tile_for(mode_, base, pre_.K, pre_.Cin, 1, false);
  pre_.name = "conv_pre_k" + std::to_string(pre_.K) + "_c" + std::to_string(base);
  (void)arena.put_conv(pre_, mode_, conv_tile(mode_, pre_.tile), hw[wi], hw[wi + 1]);
  wi += 2;

  struct BlockSrc {
    const float *w1, *b1, *w2, *b2, *ws, *bs;
  };
  std::vector<BlockSrc> blk_src;
  ups_.resize(n);
  for (int i = 0; i < n; ++i) {
    Conv& u = ups_[i];
    u.Cin = base >> i; u.Cout = base >> (i + 1); u.U = cfg.upsample_factors[i]; u.K = 2;
    u.tile = conv_tile_for(mode_, u.U * u.Cout, 2, u.Cin, 1, false);
    const ConvTile t = conv_tile(mode_, u.tile);
    u.n_chunks = ceil_div(u.Cin, t.CK);
    u.name = "ups_u" + std::to_string(u.U) + "_c" + std::to_string(u.Cout);
    const size_t o = arena.alloc(packed_conv_numel(mode_, u.U * u.Cout, u.Cin, 2, t), &u.w);
    (void)pack_convT_split(mode_, hw[wi], u.Cin, u.Cout, u.U, t, arena.at(o));
    std::vector<float> bias((size_t)u.U * u.Cout);  // the conv's bias repeated per phase
    for (int co = 0; co < u.Cout; ++co)
      for (int ph = 0; ph < u.U; ++ph) bias[(size_t)co * u.U + ph] = hw[wi + 1][co];
    arena.put_bias(bias.data(), u.U * u.Cout, t, &u.b);
    wi += 2;
    std::vector<BlockSrc> bs(NB);
    for (int j = 0; j < NB; ++j) {
      bs[j].w1 = hw[wi]; bs[j].b1 = hw[wi + 1]; bs[j].w2 = hw[wi + 2]; bs[j].b2 = hw[wi + 3];
      wi += 4;
    }
    for (int j = 0; j < NB; ++j) {
      bs[j].ws = hw[wi]; bs[j].bs = hw[wi + 1];
      wi += 2;
    }
    for (int j = 0; j < NB; ++j) {
      Block bl;
      bl.C = u.Cout; bl.dil = ipow(cfg.res_kernel, j);
      bl.a1_numel16 = packed_melgan_a1_numel16(mode_, bl.C);
      bl.a2_numel16 = packed_melgan_a2_numel16(mode_, bl.C);
      bl.name = "res_block_d" + std::to_string(bl.dil) + "_c" + std::to_string(bl.C);
      blocks_.push_back(bl);
      blk_src.push_back(bs[j]);
    }
  }
  for (size_t i = 0; i < blocks_.size(); ++i) {
    Block& bl = blocks_[i];
    const BlockSrc& s = blk_src[i];
    const size_t o1 = arena.alloc(bl.a1_numel16 / 2, &bl.a1), o2 = arena.alloc(bl.a2_numel16 / 2, &bl.a2);
    const size_t ob1 = arena.alloc(32 * melgan_mblocks(bl.C), &bl.bias1);
    const size_t ob2 = arena.alloc(32 * melgan_mblocks(bl.C), &bl.bias2);
    pack_melgan_block(mode_, s.w1, s.b1, s.w2, s.b2, s.ws, s.bs, bl.C, reinterpret_cast<uint16_t*>(arena.at(o1)),
                      reinterpret_cast<uint16_t*>(arena.at(o2)), arena.at(ob1), arena.at(ob2));
  }
  arena.put(hw[wi], (size_t)cfg.out_channels * (base >> n) * cfg.proj_kernel, &tail_w_);
  arena.put(hw[wi + 1], cfg.out_channels, &tail_b_);
  wi += 2;
  if (cfg.pqmf_bands > 0) arena.put(hw[wi++], (size_t)cfg.pqmf_bands * (cfg.pqmf_taps + 1), &g_);
  arena.upload(device_, arena_);
  hop_ = 1;
  for (int i = 0; i < n; ++i) hop_ *= cfg.upsample_factors[i];
}

int64_t Melgan::out_len(int T, int pad, int synth) const {
  melgan_check_length(cfg_, T, pad);
  TTS_REQUIRE(synth == 0 || synth == 1, 1, "melgan: synth must be 0 or 1");
  TTS_REQUIRE(!synth || cfg_.pqmf_bands > 0, 1, "melgan: synth = 1 needs a generator with PQMF bands");
  return (int64_t)hop_ * (T + 2 * (int64_t)pad) * (synth ? cfg_.pqmf_bands : 1);
}

// one activation plane: the largest [B][C_i][len_i] of the forward
int64_t Melgan::plane_floats(int B, int T, int pad) const {
  int64_t len = T + 2 * (int64_t)pad;
  int64_t m = (int64_t)cfg_.base_channels * len;
  for (int i = 0; i < cfg_.num_ups; ++i) {
    len *= cfg_.upsample_factors[i];
    m = std::max(m, (int64_t)(cfg_.base_channels >> (i + 1)) * len);
  }
  return ((m * B + 63) / 64) * 64;
}

int64_t Melgan::workspace_bytes(int B, int T, int pad) const {
  melgan_check_length(cfg_, T, pad);
  TTS_REQUIRE(B >= 1, 1, "melgan: batch size must be positive");
  const int64_t gather = (((int64_t)B * cfg_.in_channels * (T + 2 * (int64_t)pad + cfg_.proj_kernel - 1) + 63) / 64) * 64;
  return (2 * plane_floats(B, T, pad) + gather) * (int64_t)sizeof(float);
}

void Melgan::forward(const float* mel, int B, int C, int T, int pad, int synth, float* out, hipStream_t s,
                     Profiler* prof) {
  TTS_REQUIRE(mel && out, 1, "melgan: NULL argument");
  TTS_REQUIRE(B >= 1 && B <= 65535, 1, "melgan: batch size must lie in [1, 65535]");
  TTS_REQUIRE(C == cfg_.in_channels, 1,
              "melgan: the mel has " + std::to_string(C) + " channels, the generator takes " + std::to_string(cfg_.in_channels));
  (void)out_len(T, pad, synth);  // every length check, on the host, before any launch
  DeviceGuard g(device_);
  const size_t need = (size_t)workspace_bytes(B, T, pad);
  if (need > ws_.bytes()) {
    TTS_HIP_CHECK(hipStreamSynchronize(s));
    ws_.grow(device_, need, "workspace");
  }
  const int64_t plane = plane_floats(B, T, pad);
  float* buf[2] = {ws_.as<>(), ws_.as<>() + plane};
  float* gat = ws_.as<>() + 2 * plane;
  const int P = (cfg_.proj_kernel - 1) / 2;
  const int L0 = T + 2 * pad;

  run(prof, s, "mel_gather", 0.0, 4.0 * B * C * ((double)T + L0 + 2 * P),
      [&] { launch_melgan_gather(mel, B, C, T, pad, P, gat, s); });
  {
    Conv1dArgs a{};
    a.x = gat; a.w = pre_.w; a.bias = pre_.b; a.y = buf[0];
    a.Cin = pre_.Cin; a.Cout = pre_.Cout; a.Tin = L0 + 2 * P; a.Tout = L0;
    a.dil = 1; a.pad = 0; a.rep_pad = 0; a.n_chunks = pre_.n_chunks;
    a.in_slope = 1.f; a.out_slope = 1.f; a.zdiv = 1.f;
    run(prof, s, pre_.name.c_str(), 2.0 * B * pre_.Cout * (double)pre_.Cin * pre_.K * L0,
        4.0 * (B * ((double)pre_.Cin * a.Tin + (double)pre_.Cout * L0) + (double)pre_.Cout * pre_.Cin * pre_.K),
        [&] { launch_conv(mode_, a, B, pre_.K, pre_.tile, s); });
  }
  int cur = 0;
  int len = L0;
  const int NB = cfg_.num_res_blocks;
  for (int i = 0; i < cfg_.num_ups; ++i) {
    const Conv& u = ups_[i];
    const int lout = len * u.U;
    Conv1dArgs a{};
    a.x = buf[cur]; a.w = u.w; a.bias = u.b; a.y = buf[cur ^ 1];
    a.Cin = u.Cin; a.Cout = u.U * u.Cout; a.Tin = len; a.Tout = len + 1;
    a.dil = 1; a.pad = 1; a.n_chunks = u.n_chunks;
    a.in_slope = 0.2f; a.out_slope = 1.f; a.zdiv = 1.f; a.ups = u.U;
    run(prof, s, u.name.c_str(), 2.0 * B * u.Cout * (double)u.Cin * 2 * lout,
        4.0 * (B * ((double)u.Cin * len + (double)u.Cout * lout) + (double)u.Cin * u.Cout * 2 * u.U),
        [&] { launch_conv(mode_, a, B, 2, u.tile, s); });
    cur ^= 1;
    len = lout;
    for (int j = 0; j < NB; ++j) {
      const Block& bl = blocks_[i * NB + j];
      MelganBlockArgs ba{};
      ba.x = buf[cur]; ba.y = buf[cur ^ 1];
      ba.a1 = bl.a1; ba.a2 = bl.a2; ba.bias1 = bl.bias1; ba.bias2 = bl.bias2;
      ba.a1_bytes = (unsigned)(bl.a1_numel16 * 2); ba.a2_bytes = (unsigned)(bl.a2_numel16 * 2);
      ba.C = bl.C; ba.L = len; ba.dil = bl.dil;
      const double cc = (double)bl.C * bl.C;
      run(prof, s, bl.name.c_str(), 2.0 * B * cc * 5 * len, 4.0 * (2.0 * B * bl.C * len + 5 * cc),
          [&] { launch_melgan_block(mode_, ba, B, s); });
      cur ^= 1;
    }
  }
  MelganTailArgs ta{};
  ta.x = buf[cur]; ta.w = tail_w_; ta.b = tail_b_; ta.g = synth ? g_ : nullptr; ta.y = out;
  ta.Cin = cfg_.base_channels >> cfg_.num_ups; ta.Co = cfg_.out_channels; ta.K = cfg_.proj_kernel; ta.L = len;
  ta.taps = cfg_.pqmf_taps;
  const double tflops = 2.0 * B * ta.Co * (double)ta.Cin * ta.K * len + (synth ? 2.0 * B * (ta.taps + 1) * ta.Co * (double)len : 0.0);
  run(prof, s, synth ? "tail_pqmf" : "tail", tflops, 4.0 * B * ((double)ta.Cin + ta.Co) * len,
      [&] { launch_melgan_tail(ta, B, s); });
}

}  // namespace tts
