// ForwardTTS (FastPitch) inference executor (TTS/tts/models/forward_tts.py, inference):
//   encode: emb -> Encoder (FFTransformerBlock, keys under the token mask) * x_mask + emb_g
//           -> duration predictor -> format_durations -> pitch predictor -> + pitch_emb
//   decode: expansion by the durations -> positional encoding -> Decoder (FFTransformerBlock,
//           called without a mask by the reference) * y_mask -> postnet * y_mask
// around the caller's host read of y_lengths, as GlowTTS.inference runs.
//
// One FFTransformer layer (transformer.py) on [B][C][T] planes:
//   qkv = in_proj (1x1 conv, 3C rows); a = attention (launch_mha: the dk^-0.5 query scale is applied
//   there, the packed in_proj is the checkpoint's); y = x + 2 out_proj(a) (the factor 2 of the
//   reference's LN(src + 2 src2) is folded into the packed out_proj: exact, a power of two, and
//   x is the conv's residual); norm1 in place; h = relu(conv1(y)) (k3, the ReLU in the conv's
//   epilogue); z = y + conv2(h); norm2 in place.  Nothing is masked but the keys: padded columns carry
//   values and the k3 convs read them, as in the reference.
// The text side (encoder, both predictors) always runs fp32x6, so the durations do not depend on the
// math mode; the mode selects the decoder's arithmetic (fp32x6 or bf16).
#include "forward_tts.hpp"

#include <cmath>
#include <string>

#include "fft_attn.hpp"

namespace tts {

namespace {
constexpr float kEpsLn = 1e-5f;  // nn.LayerNorm

TtsVitsDpCfg predictor_cfg(int in, int hidden, int k) {
  TtsVitsDpCfg d{};
  d.in_channels = in;
  d.hidden_channels = hidden;
  d.kernel_size = k;
  d.cond_channels = 0;
  d.language_emb_dim = 0;
  d.math_mode = MATH_FP32_X6;
  return d;
}
}  // namespace

void forward_tts_validate(const TtsForwardTtsCfg& c) {
  TTS_REQUIRE(c.num_chars >= 1 && c.out_channels >= 1 && c.hidden_channels >= 1, 1, "bad ForwardTTS configuration");
  TTS_REQUIRE(c.encoder_num_layers >= 1 && c.decoder_num_layers >= 1 && c.encoder_ffn_channels >= 1 &&
                  c.decoder_ffn_channels >= 1 && c.encoder_num_heads >= 1 && c.decoder_num_heads >= 1,
              1, "bad ForwardTTS encoder / decoder parameters");
  TTS_REQUIRE(c.num_speakers >= 0, 1, "num_speakers must be >= 0");
  TTS_REQUIRE(c.math_mode >= MATH_FP32 && c.math_mode <= MATH_LAST, 1, "unknown math_mode");
  const int H = c.hidden_channels;
  TTS_REQUIRE(H % c.encoder_num_heads == 0 && H % c.decoder_num_heads == 0, 1,
              "hidden_channels must divide into the heads");
  TTS_REQUIRE(H <= kMhaMaxE && mha_head_size_ok(H / c.encoder_num_heads) && mha_head_size_ok(H / c.decoder_num_heads), 3,
              "ForwardTTS: head size must be one of 32, 64, 128, 192, 256, 384 with at most 512 channels");
  vits_dp_validate(predictor_cfg(H, c.duration_predictor_hidden_channels, c.duration_predictor_kernel_size));
  if (c.use_pitch) {
    vits_dp_validate(predictor_cfg(H, c.pitch_predictor_hidden_channels, c.pitch_predictor_kernel_size));
    TTS_REQUIRE(c.pitch_embedding_kernel_size >= 1 && c.pitch_embedding_kernel_size % 2 == 1 &&
                    c.pitch_embedding_kernel_size <= 31,
                3, "ForwardTTS: odd pitch_embedding_kernel_size <= 31");
  }
}

std::vector<int64_t> forward_tts_weight_shapes(const TtsForwardTtsCfg& c) {
  const int64_t H = c.hidden_channels, K = kFftKernel;
  std::vector<int64_t> n = {(int64_t)c.num_chars * H};
  auto block = [&](int layers, int64_t F) {
    for (int i = 0; i < layers; ++i)
      for (int64_t v : {3 * H * H, 3 * H, H * H, H, F * H * K, F, H * F * K, H, H, H, H, H}) n.push_back(v);
  };
  block(c.encoder_num_layers, c.encoder_ffn_channels);
  if (c.positional_encoding) n.push_back(H * TTS_FORWARD_TTS_MAX_FRAMES);
  block(c.decoder_num_layers, c.decoder_ffn_channels);
  n.push_back((int64_t)c.out_channels * H);
  n.push_back(c.out_channels);
  for (int64_t v : vits_dp_weight_shapes(
           predictor_cfg(c.hidden_channels, c.duration_predictor_hidden_channels, c.duration_predictor_kernel_size)))
    n.push_back(v);
  if (c.use_pitch) {
    for (int64_t v : vits_dp_weight_shapes(
             predictor_cfg(c.hidden_channels, c.pitch_predictor_hidden_channels, c.pitch_predictor_kernel_size)))
      n.push_back(v);
    n.push_back(H * c.pitch_embedding_kernel_size);
    n.push_back(H);
  }
  if (c.num_speakers > 0) n.push_back((int64_t)c.num_speakers * H);
  return n;
}

ForwardTts::ForwardTts(const TtsForwardTtsCfg& cfg, const float* const* hw, int device) : cfg_(cfg), device_(device) {
  forward_tts_validate(cfg_);
  DeviceGuard g(device_);
  dec_mode_ = cfg_.math_mode == MATH_BF16 ? MATH_BF16 : MATH_FP32_X6;
  const auto shapes = forward_tts_weight_shapes(cfg_);
  for (size_t i = 0; i < shapes.size(); ++i)
    TTS_REQUIRE(hw[i] != nullptr, 1, "weight pointer " + std::to_string(i) + " is NULL");
  const int H = cfg_.hidden_channels;
  HostArena arena;
  // text: the short-batch tile of the Glow encoder; frames: the tile table's choice for the shape
  auto put_conv = [&](Conv& cv, const float* w, const float* b, int Cout, int Cin, int K, int mode, bool frames,
                      float wscale) {
    cv.Cin = Cin; cv.Cout = Cout; cv.K = K;
    cv.tile = frames ? conv_tile_for(mode, Cout, K, Cin, 1, false) : 16;
    std::vector<float> ws, bs;
    if (wscale != 1.f) {
      ws.assign(w, w + (size_t)Cout * Cin * K);
      bs.assign(b, b + Cout);
      for (float& v : ws) v *= wscale;
      for (float& v : bs) v *= wscale;
      w = ws.data();
      b = bs.data();
    }
    TTS_REQUIRE(arena.put_conv(cv, mode, conv_tile(mode, cv.tile), w, b) == 0, 3,
                "ForwardTTS: scaled packing unsupported");
  };
  size_t wi = 0;
  arena.put(hw[wi++], (size_t)cfg_.num_chars * H, &emb_);
  auto put_block = [&](std::vector<Layer>& layers, int n, int F, int mode, bool frames) {
    layers.resize(n);
    for (Layer& L : layers) {
      put_conv(L.qkv, hw[wi], hw[wi + 1], 3 * H, H, 1, mode, frames, 1.f);
      put_conv(L.o, hw[wi + 2], hw[wi + 3], H, H, 1, mode, frames, 2.f);
      put_conv(L.ffn1, hw[wi + 4], hw[wi + 5], F, H, kFftKernel, mode, frames, 1.f);
      put_conv(L.ffn2, hw[wi + 6], hw[wi + 7], H, F, kFftKernel, mode, frames, 1.f);
      arena.put(hw[wi + 8], H, &L.g1); arena.put(hw[wi + 9], H, &L.b1);
      arena.put(hw[wi + 10], H, &L.g2); arena.put(hw[wi + 11], H, &L.b2);
      wi += 12;
    }
  };
  put_block(enc_, cfg_.encoder_num_layers, cfg_.encoder_ffn_channels, MATH_FP32_X6, false);
  if (cfg_.positional_encoding) arena.put(hw[wi++], (size_t)H * TTS_FORWARD_TTS_MAX_FRAMES, &pe_);
  put_block(dec_, cfg_.decoder_num_layers, cfg_.decoder_ffn_channels, dec_mode_, true);
  put_conv(postnet_, hw[wi], hw[wi + 1], cfg_.out_channels, H, 1, dec_mode_, true, 1.f);
  wi += 2;
  const TtsVitsDpCfg dc = predictor_cfg(H, cfg_.duration_predictor_hidden_channels, cfg_.duration_predictor_kernel_size);
  dp_ = std::make_unique<VitsDp>(dc, hw + wi, device_);
  wi += vits_dp_weight_shapes(dc).size();
  if (cfg_.use_pitch) {
    const TtsVitsDpCfg pc = predictor_cfg(H, cfg_.pitch_predictor_hidden_channels, cfg_.pitch_predictor_kernel_size);
    pp_ = std::make_unique<VitsDp>(pc, hw + wi, device_);
    wi += vits_dp_weight_shapes(pc).size();
    arena.put(hw[wi], (size_t)H * cfg_.pitch_embedding_kernel_size, &pitch_w_);
    arena.put(hw[wi + 1], H, &pitch_b_);
    wi += 2;
  }
  if (cfg_.num_speakers > 0) arena.put(hw[wi++], (size_t)cfg_.num_speakers * H, &emb_g_);
  TTS_REQUIRE(wi == shapes.size(), 2, "internal: ForwardTTS weight count mismatch");
  arena.upload(device_, arena_);
}

// X0, X1 (layer state), A (attention output) [H]; Wd [max(3H, ffn)] (qkv / FFN hidden)
void ForwardTts::reserve(int B, int T) {
  const size_t H = cfg_.hidden_channels;
  const size_t big = std::max({3 * H, (size_t)cfg_.encoder_ffn_channels, (size_t)cfg_.decoder_ffn_channels});
  const size_t need = ((size_t)B * T * (3 * H + big) + 4 * 64) * sizeof(float);
  ws_.grow(device_, need, "workspace");
}

float* ForwardTts::run_layers(const std::vector<Layer>& layers, int mode, int heads, const int64_t* key_len, int B,
                              int T, hipStream_t s, Profiler* prof, const char* tag) {
  const int H = cfg_.hidden_channels;
  const size_t plane = (size_t)B * T;
  const double P = (double)plane;
  auto al = [](size_t n) { return (n + 63) & ~size_t(63); };
  float* X0 = ws_.as<>();
  float* X1 = X0 + al(plane * H);
  float* A = X1 + al(plane * H);
  float* Wd = A + al(plane * H);
  const std::string t(tag);
  auto conv = [&](const std::string& name, const Conv& cv, const float* in, float* out, const float* res,
                  float out_slope) {
    Conv1dArgs a{};
    a.x = in; a.w = cv.w; a.bias = cv.b; a.y = out; a.res = res; a.mask = nullptr;
    a.Cin = cv.Cin; a.Cout = cv.Cout; a.Tin = T; a.Tout = T;
    a.dil = 1; a.pad = (cv.K - 1) / 2; a.rep_pad = 0; a.n_chunks = cv.n_chunks;
    a.in_slope = 1.f; a.out_slope = out_slope; a.zmode = 0; a.zdiv = 1.f;
    run(prof, s, name.c_str(), 2.0 * P * cv.Cout * cv.Cin * cv.K, 4.0 * P * (cv.Cin + cv.Cout + (res ? cv.Cout : 0)),
        [&] { launch_conv(mode, a, B, cv.K, cv.tile, s); });
  };
  auto norm = [&](const float* gamma, const float* beta, float* y) {
    run(prof, s, (t + "_layernorm").c_str(), 0.0, 8.0 * P * H,
        [&] { launch_layernorm(y, nullptr, gamma, beta, nullptr, y, B, H, T, kEpsLn, false, s); });
  };
  float* x = X0;
  for (const Layer& L : layers) {
    float* other = (x == X0) ? X1 : X0;
    conv(t + "_in_proj", L.qkv, x, Wd, nullptr, 1.f);
    run(prof, s, (t + "_attention").c_str(), 4.0 * (double)B * T * T * H, 4.0 * P * 4 * H,
        [&] { launch_mha(mode, Wd, key_len, A, B, H, heads, T, s); });
    conv(t + "_out_proj", L.o, A, other, x, 1.f);  // x + 2 out_proj(a)
    norm(L.g1, L.b1, other);
    conv(t + "_ffn1", L.ffn1, other, Wd, nullptr, 0.f);  // relu(conv1(.))
    conv(t + "_ffn2", L.ffn2, Wd, x, other, 1.f);        // y + conv2(h)
    norm(L.g2, L.b2, x);
  }
  return x;
}

void ForwardTts::block(bool decoder, const float* x, const int64_t* key_len, int B, int T, float* y, hipStream_t s,
                       Profiler* prof) {
  TTS_REQUIRE(x && y, 1, "NULL input/output pointer");
  TTS_REQUIRE(B >= 1 && T >= 1, 1, "batch and column count must be >= 1");
  DeviceGuard dg(device_);
  reserve(B, T);
  const size_t n = (size_t)B * T * cfg_.hidden_channels * sizeof(float);
  TTS_HIP_CHECK(hipMemcpyAsync(ws_.as<>(), x, n, hipMemcpyDeviceToDevice, s));
  const float* r = decoder ? run_layers(dec_, dec_mode_, cfg_.decoder_num_heads, key_len, B, T, s, prof, "dec")
                           : run_layers(enc_, MATH_FP32_X6, cfg_.encoder_num_heads, key_len, B, T, s, prof, "enc");
  TTS_HIP_CHECK(hipMemcpyAsync(y, r, n, hipMemcpyDeviceToDevice, s));
}

void ForwardTts::encode(const int64_t* tok, const int64_t* x_len, const int64_t* spk, const float* given, int B, int T,
                        float length_scale, float* o_en, float* x_mask, float* dur_log, float* pitch, float* dur,
                        int64_t* y_len, hipStream_t s, Profiler* prof) {
  TTS_REQUIRE(tok && x_len && o_en && x_mask && dur_log && dur && y_len, 1, "NULL input/output pointer");
  TTS_REQUIRE(!cfg_.use_pitch || pitch, 1, "NULL pitch output (use_pitch)");
  TTS_REQUIRE(cfg_.num_speakers == 0 || spk, 1, "this model has a speaker embedding: pass speaker ids");
  TTS_REQUIRE(B >= 1 && T >= 1, 1, "batch and token count must be >= 1");
  TTS_REQUIRE(T <= EXPAND_MAX_TX, 3, "more than " + std::to_string(EXPAND_MAX_TX) + " tokens per utterance");
  DeviceGuard dg(device_);
  reserve(B, T);
  const int H = cfg_.hidden_channels;
  const double P = (double)B * T;
  run(prof, s, "enc_embed", 0.0, 4.0 * P * H + 16.0 * P,
      [&] { launch_ftts_embed(tok, x_len, emb_, ws_.as<>(), x_mask, B, H, T, cfg_.num_chars, s); });
  const float* x = run_layers(enc_, MATH_FP32_X6, cfg_.encoder_num_heads, x_len, B, T, s, prof, "enc");
  run(prof, s, "enc_mask_speaker", 0.0, 8.0 * P * H, [&] {
    launch_ftts_mask_add(x, x_mask, cfg_.num_speakers > 0 ? emb_g_ : nullptr, spk, o_en, B, H, T, cfg_.num_speakers, s);
  });
  dp_->forward(o_en, x_mask, nullptr, nullptr, B, T, dur_log, s, prof);
  run(prof, s, "durations", 0.0, 12.0 * P,
      [&] { launch_ftts_durations(dur_log, x_mask, given, dur, y_len, B, T, length_scale, s); });
  if (cfg_.use_pitch) {
    pp_->forward(o_en, x_mask, nullptr, nullptr, B, T, pitch, s, prof);
    const int k = cfg_.pitch_embedding_kernel_size;
    run(prof, s, "pitch_emb", 2.0 * P * H * k, 8.0 * P * H,
        [&] { launch_ftts_pitch_emb(pitch, pitch_w_, pitch_b_, o_en, B, H, T, k, s); });
  }
}

void ForwardTts::decode(const float* o_en, const float* dur, const float* x_mask, const int64_t* y_len, int B, int T,
                        int T_de, bool mask_keys, float* out, float* attn, float* y_mask, hipStream_t s,
                        Profiler* prof) {
  TTS_REQUIRE(o_en && dur && x_mask && y_len && out && y_mask, 1, "NULL input/output pointer");
  TTS_REQUIRE(B >= 1 && T >= 1 && T_de >= 1, 1, "batch, token and frame count must be >= 1");
  TTS_REQUIRE(!cfg_.positional_encoding || T_de <= TTS_FORWARD_TTS_MAX_FRAMES, 1,
              "more than " + std::to_string(TTS_FORWARD_TTS_MAX_FRAMES) + " frames (the positional encoding's length)");
  DeviceGuard dg(device_);
  reserve(B, T_de);
  const int H = cfg_.hidden_channels;
  const double P = (double)B * T_de;
  // o_en_ex = attn^T o_en: every token column repeated dur times, zero past y_len
  ExpandArgs e{};
  e.w_ceil = dur; e.x_mask = x_mask; e.y_len = y_len; e.o_mean = o_en;
  e.C = H; e.T_x = T; e.T_y = T_de; e.z = ws_.as<>(); e.y_mask = y_mask; e.attn = attn;
  run(prof, s, "expand", 0.0, 4.0 * P * (2 * H + (attn ? T : 0)), [&] { launch_expand(e, B, s); });
  if (cfg_.positional_encoding)
    run(prof, s, "pos_encoding", 0.0, 12.0 * P * H, [&] {
      launch_ftts_posenc(ws_.as<>(), pe_, y_mask, B, H, T_de, TTS_FORWARD_TTS_MAX_FRAMES, sqrtf((float)H), s);
    });
  const float* x = run_layers(dec_, dec_mode_, cfg_.decoder_num_heads, mask_keys ? y_len : nullptr, B, T_de, s, prof,
                              "dec");
  // postnet(o * y_mask) * y_mask: a 1x1 conv, so the inner mask changes nothing the outer one keeps
  Conv1dArgs a{};
  a.x = x; a.w = postnet_.w; a.bias = postnet_.b; a.y = out; a.mask = y_mask;
  a.Cin = H; a.Cout = cfg_.out_channels; a.Tin = T_de; a.Tout = T_de;
  a.dil = 1; a.pad = 0; a.n_chunks = postnet_.n_chunks;
  a.in_slope = 1.f; a.out_slope = 1.f; a.zmode = 0; a.zdiv = 1.f;
  run(prof, s, "dec_postnet", 2.0 * P * H * cfg_.out_channels, 4.0 * P * (H + cfg_.out_channels),
      [&] { launch_conv(dec_mode_, a, B, 1, postnet_.tile, s); });
}

}  // namespace tts
