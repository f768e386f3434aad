// XTTS GPT executor (TTS/tts/layers/xtts/gpt.py, gpt_inference.py):
//   prefill:  the prefix [cond latents | start_text, text, stop_text] as planes [B][E][T] in one pass on
//             the conv path: per layer LayerNorm | c_attn (1x1 conv) | K, V into the cache layout |
//             causal MFMA attention | c_proj + residual | LayerNorm | c_fc | gelu_new | mlp c_proj + residual
//   generate: per step  5 launches per layer (c_attn with ln_1 | attention | c_proj + residual |
//             c_fc with ln_2 + gelu_new | mlp c_proj + residual), then the head (ln_f, final_norm,
//             mel_head) and the logits -> token step with the bookkeeping and the next input;
//             enqueued in chunks with one host read of the all-done word per chunk
//   latents:  the same whole-sequence pass over [prefix | start_audio, codes, stop_audio], then the head
//             per mel position (the step's head kernel on the plane's column)
// The step's products are fp32 FMA on fp32 matrices (bf16 mode: bf16-stored matrices, fp32 accumulation);
// the whole-sequence convs and attention run fp32x6 (bf16 mode: on the same bf16-rounded matrices); the
// cache, the activations and the softmax are fp32 in every mode.
#include "xtts_gpt.hpp"

#include <algorithm>
#include <cstring>
#include <string>

namespace tts {

namespace {
size_t al(size_t n) { return (n + 63) & ~size_t(63); }
// round to nearest even to 8 significant bits, as the skinny packer stores a bf16 matrix
float bf16_round(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  u &= 0xffff0000u;
  std::memcpy(&f, &u, 4);
  return f;
}
constexpr int kCtlInts = 7 * 64;  // skip, done, plen, n (kGptMaxBatch each, padded), counters, klen (int64)
}  // namespace

void xtts_gpt_validate(const TtsXttsGptCfg& c) {
  TTS_REQUIRE(c.layers >= 1 && c.model_dim >= 1 && c.heads >= 1 && c.model_dim % c.heads == 0, 1,
              "bad XTTS GPT configuration: layers, model_dim, heads");
  TTS_REQUIRE(c.n_text_tokens >= 1 && c.n_audio_tokens >= 2, 1, "bad XTTS GPT token counts");
  TTS_REQUIRE(c.start_text_token >= 0 && c.start_text_token < c.n_text_tokens && c.stop_text_token >= 0 &&
                  c.stop_text_token < c.n_text_tokens,
              1, "XTTS GPT: start / stop text tokens outside the text table");
  TTS_REQUIRE(c.start_audio_token >= 0 && c.start_audio_token < c.n_audio_tokens && c.stop_audio_token >= 0 &&
                  c.stop_audio_token < c.n_audio_tokens,
              1, "XTTS GPT: start / stop audio tokens outside the audio table");
  TTS_REQUIRE(c.text_positions >= 3 && c.mel_positions >= 1 && c.prompt_positions >= 0, 1,
              "bad XTTS GPT position counts");
  TTS_REQUIRE(c.chunk >= 0, 1, "chunk must be >= 0");
  TTS_REQUIRE(c.math_mode >= MATH_FP32 && c.math_mode <= MATH_LAST, 1, "unknown math_mode");
  const int dk = c.model_dim / c.heads;
  TTS_REQUIRE(dk == 32 || dk == 64 || dk == 128, 3, "XTTS GPT: the head size must be 32, 64 or 128");
  TTS_REQUIRE(c.model_dim % kSkinnyKAlign == 0, 3,
              "XTTS GPT: model_dim must be a multiple of " + std::to_string(kSkinnyKAlign));
  TTS_REQUIRE(c.n_audio_tokens <= kGptMaxVocab, 3,
              "XTTS GPT: at most " + std::to_string(kGptMaxVocab) + " audio tokens");
}

std::vector<int64_t> xtts_gpt_weight_shapes(const TtsXttsGptCfg& c) {
  const int64_t E = c.model_dim;
  std::vector<int64_t> n = {c.n_text_tokens * E, c.n_audio_tokens * E, c.text_positions * E, c.mel_positions * E};
  for (int i = 0; i < c.layers; ++i)
    for (int64_t v : {E, E, E * 3 * E, 3 * E, E * E, E, E, E, E * 4 * E, 4 * E, 4 * E * E, E}) n.push_back(v);
  for (int64_t v : {E, E, E, E, c.n_audio_tokens * E, (int64_t)c.n_audio_tokens}) n.push_back(v);
  return n;
}

XttsGpt::XttsGpt(const TtsXttsGptCfg& cfg, const float* const* hw, int device) : cfg_(cfg), device_(device) {
  xtts_gpt_validate(cfg_);
  DeviceGuard g(device_);
  bf16_ = cfg_.math_mode == MATH_BF16;
  E_ = cfg_.model_dim; H_ = cfg_.heads; dk_ = E_ / H_; L_ = cfg_.layers; V_ = cfg_.n_audio_tokens;
  P_ = cfg_.prompt_positions;
  const auto shapes = xtts_gpt_weight_shapes(cfg_);
  for (size_t i = 0; i < shapes.size(); ++i)
    TTS_REQUIRE(hw[i] != nullptr, 1, "weight pointer " + std::to_string(i) + " is NULL");
  // The whole-sequence convs and attention run fp32x6 in every mode.  In the bf16 mode their matrices
  // are the bf16-rounded ones the steps stream, as exact fp32x6 operands with fp32 activations: the
  // cache the prefill writes is then the one the steps would have written.  (bf16 MFMA operands also
  // round every activation: measured 5.7e-2 on the latents, beyond the bf16 gate of 5e-2.)
  conv_mode_ = MATH_FP32_X6;
  HostArena arena;
  // the HF Conv1D matrix w [K][R] as the 1x1 conv [R][K][1] of the whole-sequence pass
  auto put_conv = [&](PackedConv& cv, const float* w, const float* b, int K, int R, bool res) {
    std::vector<float> wt((size_t)R * K);
    for (int k = 0; k < K; ++k)
      for (int r = 0; r < R; ++r) wt[(size_t)r * K + k] = bf16_ ? bf16_round(w[(size_t)k * R + r]) : w[(size_t)k * R + r];
    cv.Cin = K; cv.Cout = R; cv.K = 1;
    cv.tile = conv_tile_for(conv_mode_, R, 1, K, 1, res);
    TTS_REQUIRE(arena.put_conv(cv, conv_mode_, conv_tile(conv_mode_, cv.tile), wt.data(), b) == 0, 3,
                "XTTS GPT: scaled packing unsupported");
  };
  auto put_cols = [&](const float* w, int K, int R, float** dst) {  // HF Conv1D [K][R]
    const size_t off = arena.alloc((size_t)packed_skinny_numel(R, K, bf16_), dst);
    pack_skinny_cols(w, K, R, bf16_, arena.at(off));
  };
  size_t wi = 0;
  arena.put(hw[wi++], (size_t)cfg_.n_text_tokens * E_, &text_emb_);
  arena.put(hw[wi++], (size_t)V_ * E_, &mel_emb_);
  arena.put(hw[wi++], (size_t)cfg_.text_positions * E_, &text_pos_);
  arena.put(hw[wi++], (size_t)cfg_.mel_positions * E_, &mel_pos_);
  layer_.resize(L_);
  for (int i = 0; i < L_; ++i, wi += 12) {
    Layer& l = layer_[i];
    const float* const* p = hw + wi;
    arena.put(p[0], E_, &l.ln1_g);
    arena.put(p[1], E_, &l.ln1_b);
    put_cols(p[2], E_, 3 * E_, &l.w_qkv);
    arena.put(p[3], (size_t)3 * E_, &l.b_qkv);
    put_cols(p[4], E_, E_, &l.w_proj);
    arena.put(p[5], E_, &l.b_proj);
    arena.put(p[6], E_, &l.ln2_g);
    arena.put(p[7], E_, &l.ln2_b);
    put_cols(p[8], E_, 4 * E_, &l.w_fc);
    arena.put(p[9], (size_t)4 * E_, &l.b_fc);
    put_cols(p[10], 4 * E_, E_, &l.w_mp);
    arena.put(p[11], E_, &l.b_mp);
    put_conv(l.c_qkv, p[2], p[3], E_, 3 * E_, false);
    put_conv(l.c_proj, p[4], p[5], E_, E_, true);
    put_conv(l.c_fc, p[8], p[9], E_, 4 * E_, false);
    put_conv(l.c_mp, p[10], p[11], 4 * E_, E_, true);
  }
  arena.put(hw[wi++], E_, &lnf_g_);
  arena.put(hw[wi++], E_, &lnf_b_);
  arena.put(hw[wi++], E_, &fn_g_);
  arena.put(hw[wi++], E_, &fn_b_);
  {  // mel_head is an nn.Linear: [n_audio][E] rows
    const size_t off = arena.alloc((size_t)packed_skinny_numel(V_, E_, bf16_), &head_w_);
    pack_skinny_rows(hw[wi++], V_, E_, bf16_, arena.at(off));
  }
  arena.put(hw[wi++], V_, &head_b_);
  TTS_REQUIRE(wi == shapes.size(), 2, "internal: XTTS GPT weight count mismatch");
  arena.upload(device_, arena_);
}

size_t XttsGpt::ws_floats(int B, int cap) const {
  const int BT = skinny_batch_tile(B);
  return 2 * al((size_t)E_ * BT) + al((size_t)4 * E_ * BT) + al((size_t)BT * E_) + al((size_t)BT * V_) + kCtlInts +
         2 * (size_t)L_ * al((size_t)B * cap * E_) + 4 * al((size_t)B * cap * E_) + al((size_t)B * cap * 4 * E_);
}

XttsGpt::Ws XttsGpt::carve(int B, int cap) const {
  const int BT = skinny_batch_tile(B);
  Ws w{};
  float* p = ws_.as<>();
  w.x = p; p += al((size_t)E_ * BT);
  w.att = p; p += al((size_t)E_ * BT);
  w.h4 = p; p += al((size_t)4 * E_ * BT);
  w.q = p; p += al((size_t)BT * E_);
  w.logits = p; p += al((size_t)BT * V_);
  int* ctl = reinterpret_cast<int*>(p);
  w.skip = ctl; w.done = ctl + 64; w.plen = ctl + 128; w.n = ctl + 192; w.counters = ctl + 256;
  w.klen = reinterpret_cast<int64_t*>(ctl + 320);
  p += kCtlInts;
  const size_t plane = al((size_t)B * cap * E_);
  w.pre = p; w.X0 = p + plane; w.X1 = p + 2 * plane; w.A = p + 3 * plane; w.Wd = p + 4 * plane;
  p += 4 * plane + al((size_t)B * cap * 4 * E_);
  w.layer_stride = al((size_t)B * cap * E_);
  w.kc = p;
  w.vc = p + (size_t)L_ * w.layer_stride;
  return w;
}

float* XttsGpt::seq_layers(const Ws& w, int T, hipStream_t s, Profiler* prof) {
  const int B = B_, E = E_;
  const double P = (double)B * T;
  auto conv = [&](const char* name, const PackedConv& cv, const float* in, float* out, const float* res) {
    Conv1dArgs a{};
    a.x = in; a.w = cv.w; a.bias = cv.b; a.y = out; a.res = res;
    a.Cin = cv.Cin; a.Cout = cv.Cout; a.Tin = T; a.Tout = T;
    a.dil = 1; a.pad = 0; a.n_chunks = cv.n_chunks;
    a.in_slope = 1.f; a.out_slope = 1.f; a.zmode = 0; a.zdiv = 1.f;
    run(prof, s, name, 2.0 * P * cv.Cout * cv.Cin, 4.0 * P * (cv.Cin + cv.Cout + (res ? cv.Cout : 0)),
        [&] { launch_conv(conv_mode_, a, B, 1, cv.tile, s); });
  };
  float *x = w.X0, *other = w.X1;
  for (int i = 0; i < L_; ++i) {
    const Layer& l = layer_[i];
    run(prof, s, "seq_ln_1", 0.0, 8.0 * P * E, [&] { launch_gpt_seq_layernorm(x, l.ln1_g, l.ln1_b, w.A, B, E, T, s); });
    conv("seq_c_attn", l.c_qkv, w.A, w.Wd, nullptr);
    run(prof, s, "seq_kv_to_cache", 0.0, 16.0 * P * E, [&] {
      launch_gpt_seq_kv(w.Wd, w.klen, w.kc + (size_t)i * w.layer_stride, w.vc + (size_t)i * w.layer_stride, B, E, T,
                        cap_, s);
    });
    run(prof, s, "seq_attention", 2.0 * P * T * E, 16.0 * P * E,
        [&] { launch_mha_causal(conv_mode_, w.Wd, w.klen, w.A, B, E, H_, T, s); });
    conv("seq_attn_c_proj", l.c_proj, w.A, other, x);  // x + c_proj(a)
    std::swap(x, other);
    run(prof, s, "seq_ln_2", 0.0, 8.0 * P * E, [&] { launch_gpt_seq_layernorm(x, l.ln2_g, l.ln2_b, w.A, B, E, T, s); });
    conv("seq_mlp_c_fc", l.c_fc, w.A, w.Wd, nullptr);
    run(prof, s, "seq_gelu_new", 0.0, 32.0 * P * E, [&] { launch_gpt_seq_gelu(w.Wd, (int64_t)B * 4 * E * T, s); });
    conv("seq_mlp_c_proj", l.c_mp, w.Wd, other, x);  // x + mlp.c_proj(h)
    std::swap(x, other);
  }
  return x;
}

void XttsGpt::layers(const Ws& w, const int* base, int off, const int* skip, hipStream_t s, Profiler* prof) {
  const int B = B_, BT = BT_, E = E_;
  const double wb = bf16_ ? 2.0 : 4.0;
  GptSkinnyArgs g{};
  g.B = B; g.BT = BT; g.bf16 = bf16_; g.skip = skip; g.base = base; g.off = off; g.cap = cap_; g.E = E;
  GptAttnArgs at{};
  at.q = w.q; at.base = base; at.off = off; at.cap = cap_; at.E = E; at.heads = H_; at.dk = dk_; at.B = B; at.BT = BT;
  at.skip = skip; at.out = w.att;
  for (int i = 0; i < L_; ++i) {
    const Layer& l = layer_[i];
    float* kc = w.kc + (size_t)i * w.layer_stride;
    float* vc = w.vc + (size_t)i * w.layer_stride;
    GptSkinnyArgs a = g;  // c_attn(ln_1(x)): q to the step buffer, k and v to the cache row
    a.w = l.w_qkv; a.bias = l.b_qkv; a.x = w.x; a.nln = 1; a.ln_g[0] = l.ln1_g; a.ln_b[0] = l.ln1_b;
    a.K = E; a.Kp = skinny_kp(E); a.R = 3 * E; a.epi = kGptEpiQkv; a.q = w.q; a.kc = kc; a.vc = vc;
    run(prof, s, "c_attn", 2.0 * 3 * E * E * B, wb * 3 * E * E, [&] { launch_gpt_skinny(a, s); });
    at.kc = kc; at.vc = vc;
    run(prof, s, "attention", 4.0 * B * E * cap_, 8.0 * B * E * cap_, [&] { launch_gpt_decode_attn(at, s); });
    GptSkinnyArgs pj = g;  // x += c_proj(attention)
    pj.w = l.w_proj; pj.bias = l.b_proj; pj.x = w.att; pj.K = E; pj.Kp = skinny_kp(E); pj.R = E;
    pj.epi = kGptEpiResidual; pj.out = w.x;
    run(prof, s, "attn_c_proj", 2.0 * E * E * B, wb * E * E, [&] { launch_gpt_skinny(pj, s); });
    GptSkinnyArgs fc = g;  // gelu_new(c_fc(ln_2(x)))
    fc.w = l.w_fc; fc.bias = l.b_fc; fc.x = w.x; fc.nln = 1; fc.ln_g[0] = l.ln2_g; fc.ln_b[0] = l.ln2_b;
    fc.K = E; fc.Kp = skinny_kp(E); fc.R = 4 * E; fc.epi = kGptEpiGelu; fc.out = w.h4;
    run(prof, s, "mlp_c_fc", 2.0 * 4 * E * E * B, wb * 4 * E * E, [&] { launch_gpt_skinny(fc, s); });
    GptSkinnyArgs mp = g;  // x += mlp.c_proj(.)
    mp.w = l.w_mp; mp.bias = l.b_mp; mp.x = w.h4; mp.K = 4 * E; mp.Kp = skinny_kp(4 * E); mp.R = E;
    mp.epi = kGptEpiResidual; mp.out = w.x;
    run(prof, s, "mlp_c_proj", 2.0 * 4 * E * E * B, wb * 4 * E * E, [&] { launch_gpt_skinny(mp, s); });
  }
}

void XttsGpt::head(const Ws& w, const int* skip, float* logits2, int64_t ld2, float* lat, int64_t ld_lat,
                   const int* lat_n, int lat_step, bool lat_only, hipStream_t s, Profiler* prof) {
  GptSkinnyArgs a{};
  a.B = B_; a.BT = BT_; a.bf16 = bf16_; a.skip = skip; a.E = E_;
  a.w = head_w_; a.bias = head_b_; a.x = w.x; a.nln = 2;
  a.ln_g[0] = lnf_g_; a.ln_b[0] = lnf_b_; a.ln_g[1] = fn_g_; a.ln_b[1] = fn_b_;
  a.K = E_; a.Kp = skinny_kp(E_); a.R = V_; a.epi = kGptEpiLogits;
  a.logits = w.logits; a.ld_logits = V_; a.logits2 = logits2; a.ld_logits2 = ld2;
  a.lat = lat; a.ld_lat = ld_lat; a.lat_n = lat_n; a.lat_step = lat_step; a.lat_only = lat_only;
  if (lat_only) run(prof, s, "final_norms", 0.0, 8.0 * E_ * B_, [&] { launch_gpt_skinny(a, s); });
  else run(prof, s, "mel_head", 2.0 * V_ * E_ * B_, (bf16_ ? 2.0 : 4.0) * V_ * E_, [&] { launch_gpt_skinny(a, s); });
}

void XttsGpt::prefill(const float* cond, const int64_t* tok, const int64_t* text_len, int B, int T, int max_new,
                      hipStream_t s, Profiler* prof) {
  TTS_REQUIRE(B >= 1 && T >= 0 && max_new >= 1, 1, "batch and max_new_tokens must be >= 1, the token count >= 0");
  TTS_REQUIRE(B <= kGptMaxBatch, 3, "XTTS GPT: more than " + std::to_string(kGptMaxBatch) + " utterances");
  TTS_REQUIRE(T + 2 <= cfg_.text_positions, 1,
              "XTTS GPT: " + std::to_string(T) + " text tokens and their start / stop tokens exceed the " +
                  std::to_string(cfg_.text_positions) + " text positions");
  TTS_REQUIRE(max_new <= cfg_.mel_positions, 1,
              "XTTS GPT: max_new_tokens exceeds the " + std::to_string(cfg_.mel_positions) + " mel positions");
  TTS_REQUIRE((P_ == 0 || cond) && (T == 0 || tok), 1, "NULL input pointer");
  DeviceGuard dg(device_);
  const int rows = P_ + T + 2, cap = rows + max_new;
  B_ = 0;  // no prefix is held while the workspace may move
  ws_.grow(device_, ws_floats(B, cap) * sizeof(float), "workspace");
  B_ = B; BT_ = skinny_batch_tile(B); cap_ = cap; max_new_ = max_new;
  const Ws w = carve(B, cap);
  // the padded batch columns and the control words start at zero
  TTS_HIP_CHECK(hipMemsetAsync(w.x, 0, (size_t)(reinterpret_cast<float*>(w.skip) + kCtlInts - w.x) * sizeof(float), s));
  pre_rows_ = rows;
  GptSeqEmbedArgs e{};
  e.cond = cond; e.text = tok; e.text_len = text_len; e.text_emb = text_emb_; e.text_pos = text_pos_;
  e.P = P_; e.Ttext = T; e.n_text = cfg_.n_text_tokens; e.start_text = cfg_.start_text_token;
  e.stop_text = cfg_.stop_text_token; e.pre = w.pre; e.pre_rows = rows; e.plen = w.plen; e.klen = w.klen;
  e.x = w.X0; e.B = B; e.E = E_; e.T = rows;
  run(prof, s, "seq_rows", 0.0, 8.0 * B * E_ * rows, [&] { launch_gpt_seq_embed(e, s); });
  seq_layers(w, rows, s, prof);
}

int XttsGpt::generate(int S, float penalty, float temperature, int top_k, float top_p, const float* u, int* codes,
                      int* lengths, float* logits, float* latents, hipStream_t s, Profiler* prof) {
  TTS_REQUIRE(B_ >= 1, 1, "XTTS GPT: generate needs a prefill first");
  TTS_REQUIRE(S >= 1 && S <= max_new_, 1, "XTTS GPT: max_new_tokens must lie in [1, the prefill's max_new_tokens]");
  TTS_REQUIRE(codes && lengths, 1, "NULL output pointer");
  TTS_REQUIRE(penalty > 0.f && (!u || temperature > 0.f) && top_p >= 0.f, 1,
              "XTTS GPT: repetition_penalty and temperature must be > 0, top_p >= 0");
  DeviceGuard dg(device_);
  const int B = B_;
  const Ws w = carve(B, cap_);
  TTS_HIP_CHECK(hipMemsetAsync(w.done, 0, 64 * sizeof(int), s));
  TTS_HIP_CHECK(hipMemsetAsync(w.n, 0, 128 * sizeof(int), s));  // n and the counters
  TTS_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(codes), cfg_.stop_audio_token, (size_t)B * S, s));
  if (logits) TTS_HIP_CHECK(hipMemsetAsync(logits, 0, (size_t)B * S * V_ * sizeof(float), s));
  if (latents) TTS_HIP_CHECK(hipMemsetAsync(latents, 0, (size_t)B * S * E_ * sizeof(float), s));
  GptEmbedArgs e{};
  e.mel = 1; e.t = 0; e.mel_emb = mel_emb_; e.mel_pos = mel_pos_; e.n_audio = V_;
  e.start_audio = cfg_.start_audio_token; e.stop_audio = cfg_.stop_audio_token; e.x = w.x; e.B = B; e.BT = BT_; e.E = E_;
  run(prof, s, "start_row", 0.0, 8.0 * B * E_, [&] { launch_gpt_embed(e, s); });
  GptSampleArgs sp{};
  sp.logits = w.logits; sp.V = V_; sp.B = B; sp.BT = BT_; sp.E = E_;
  sp.penalty = penalty; sp.temperature = temperature; sp.top_p = top_p; sp.top_k = top_k;
  sp.u = u; sp.ldu = S; sp.codes = codes; sp.S = S; sp.max_steps = S;
  sp.start_audio = cfg_.start_audio_token; sp.stop_audio = cfg_.stop_audio_token;
  sp.done = w.done; sp.n = w.n; sp.counters = w.counters; sp.mel_emb = mel_emb_; sp.mel_pos = mel_pos_; sp.x = w.x;
  const int chunk = cfg_.chunk > 0 ? cfg_.chunk : 32;
  int step = 0, all_done = 0;
  while (step < S && !all_done) {
    const int end = std::min(S, step + chunk);
    for (; step < end; ++step) {
      layers(w, w.plen, step, w.done, s, prof);
      head(w, w.done, logits ? logits + (size_t)step * V_ : nullptr, (int64_t)S * V_,
           latents ? latents + (size_t)step * E_ : nullptr, (int64_t)S * E_, nullptr, step, false, s, prof);
      sp.step = step; sp.u_off = step;
      run(prof, s, "sample", 0.0, 4.0 * B * V_, [&] { launch_gpt_sample(sp, s); });
    }
    TTS_HIP_CHECK(hipMemcpyAsync(&all_done, w.counters + 1, sizeof(int), hipMemcpyDeviceToHost, s));
    TTS_HIP_CHECK(hipStreamSynchronize(s));
  }
  // the last step ends every utterance, so n[] is complete here
  TTS_HIP_CHECK(hipMemcpyAsync(lengths, w.n, (size_t)B * sizeof(int), hipMemcpyDeviceToDevice, s));
  return step;
}

void XttsGpt::latents(const int* codes, const int* lengths, int S, int rows, float* lat, float* logits, hipStream_t s,
                      Profiler* prof) {
  TTS_REQUIRE(B_ >= 1, 1, "XTTS GPT: latents needs a prefill first");
  TTS_REQUIRE(codes && lengths && (lat || logits), 1, "NULL argument");
  TTS_REQUIRE(S >= 1 && rows >= 1, 1, "XTTS GPT: the code and row counts must be >= 1");
  TTS_REQUIRE(rows <= max_new_ && rows <= cfg_.mel_positions, 1,
              "XTTS GPT: more mel positions than the prefill reserved or the position table holds");
  DeviceGuard dg(device_);
  const int B = B_;
  const Ws w = carve(B, cap_);
  if (lat) TTS_HIP_CHECK(hipMemsetAsync(lat, 0, (size_t)B * rows * E_ * sizeof(float), s));
  if (logits) TTS_HIP_CHECK(hipMemsetAsync(logits, 0, (size_t)B * rows * V_ * sizeof(float), s));
  // one pass over [prefix | mel rows] (the prefix from the rows the prefill saved); it rewrites the
  // cache rows of the prefix with the same values and leaves the mel rows' behind them
  const int T = pre_rows_ + rows;
  GptSeqEmbedArgs e{};
  e.from_pre = 1; e.pre = w.pre; e.pre_rows = pre_rows_; e.P = P_;
  e.codes = codes; e.n = lengths; e.S = S; e.rows = rows; e.mel_emb = mel_emb_; e.mel_pos = mel_pos_; e.n_audio = V_;
  e.start_audio = cfg_.start_audio_token; e.stop_audio = cfg_.stop_audio_token; e.plen = w.plen; e.klen = w.klen;
  e.x = w.X0; e.B = B; e.E = E_; e.T = T;
  run(prof, s, "seq_rows", 0.0, 8.0 * B * E_ * T, [&] { launch_gpt_seq_embed(e, s); });
  const float* h = seq_layers(w, T, s, prof);
  // ln_f, final_norm and mel_head per mel position through the step's head kernel
  for (int t = 0; t < rows; ++t) {
    run(prof, s, "seq_column", 0.0, 8.0 * B * E_,
        [&] { launch_gpt_seq_column(h, w.plen, lengths, S, t, B, E_, T, BT_, w.x, w.skip, s); });
    head(w, w.skip, logits ? logits + (size_t)t * V_ : nullptr, (int64_t)rows * V_,
         lat ? lat + (size_t)t * E_ : nullptr, (int64_t)rows * E_, lengths, t, logits == nullptr, s, prof);
  }
}

// ------------------------------------------------------------------------------------ kernel-test ops
void op_gpt_decode_attn(const float* d_q, const float* d_k, const float* d_v, const int* d_lens, int B, int E, int heads,
                        int cap, float* d_out, hipStream_t s) {
  TTS_REQUIRE(d_q && d_k && d_v && d_lens && d_out, 1, "NULL argument");
  TTS_REQUIRE(B >= 1 && E >= 1 && heads >= 1 && cap >= 1 && E % heads == 0, 1, "bad attention shape");
  TTS_REQUIRE(B <= kGptMaxBatch, 3, "XTTS GPT: more than " + std::to_string(kGptMaxBatch) + " utterances");
  const int dk = E / heads;
  TTS_REQUIRE(dk == 32 || dk == 64 || dk == 128, 3, "XTTS GPT: the head size must be 32, 64 or 128");
  int dev = 0;
  TTS_HIP_CHECK(hipGetDevice(&dev));
  const int BT = skinny_batch_tile(B);
  DeviceBuffer buf;
  buf.grow(dev, (size_t)E * BT * sizeof(float), "operand");
  GptAttnArgs a{};
  a.q = d_q; a.kc = d_k; a.vc = d_v; a.base = d_lens; a.off = -1; a.cap = cap; a.E = E; a.heads = heads; a.dk = dk;
  a.B = B; a.BT = BT; a.out = buf.as<>();
  TTS_HIP_CHECK(hipMemsetAsync(buf.as<>(), 0, (size_t)E * BT * sizeof(float), s));
  launch_gpt_decode_attn(a, s);
  launch_t2_transpose(buf.as<>(), d_out, E, B, BT, E, s);
  TTS_HIP_CHECK(hipStreamSynchronize(s));  // the operand buffer is freed on return
}

void op_gpt_sample(const float* d_logits, int B, int V, int* d_codes, int n_prev, int start_audio, float penalty,
                   float temperature, int top_k, float top_p, const float* d_u, hipStream_t s) {
  TTS_REQUIRE(d_logits && d_codes, 1, "NULL argument");
  TTS_REQUIRE(B >= 1 && n_prev >= 0 && penalty > 0.f && (!d_u || temperature > 0.f) && top_p >= 0.f, 1,
              "bad sampling arguments");
  TTS_REQUIRE(B <= kGptMaxBatch, 3, "XTTS GPT: more than " + std::to_string(kGptMaxBatch) + " utterances");
  GptSampleArgs a{};
  a.logits = d_logits; a.V = V; a.B = B; a.BT = skinny_batch_tile(B);
  a.penalty = penalty; a.temperature = temperature; a.top_p = top_p; a.top_k = top_k;
  a.u = d_u; a.ldu = 1; a.u_off = 0; a.codes = d_codes; a.S = n_prev + 1; a.step = n_prev; a.max_steps = n_prev + 1;
  a.start_audio = start_audio; a.stop_audio = -1;
  launch_gpt_sample(a, s);
  TTS_HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace tts
