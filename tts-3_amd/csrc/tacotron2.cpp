// Tacotron2 inference executor (TTS/tts/models/tacotron2.py, inference):
//   encode:  embedding -> 3 x (conv k5 + folded BatchNorm, ReLU in the conv epilogue) -> W_ih x for every
//            token and both directions as one 1x1 conv -> T_en LSTM steps (both directions per launch)
//            -> speaker columns -> inputs_layer
//   decode:  per step  attention RNN | attention | decoder RNN | projection | stop, bookkeeping, next prenet
//            (5 launches), enqueued in chunks with one host read of the all-done word per chunk
//   postnet: planes -> 5 x (conv k5 + folded BatchNorm, masked; tanh after the first four) -> + residual
// The convs run on the shared conv path (fp32x6, or bf16 in the bf16 mode); the recurrent products are
// fp32 FMA (bf16 mode: bf16-stored attention / decoder RNN matrices, fp32 accumulation).
#include "tacotron2.hpp"

#include <algorithm>
#include <cmath>
#include <string>

namespace tts {

namespace {
constexpr int kPostnetDim = 512;  // hard-coded by the reference's Postnet
constexpr int kConvK = 5;
constexpr double kEpsBn = 1e-5;

size_t al(size_t n) { return (n + 63) & ~size_t(63); }
}  // namespace

void tacotron2_validate(const TtsTacotron2Cfg& c) {
  TTS_REQUIRE(c.num_chars >= 1 && c.out_channels >= 1 && c.r >= 1, 1, "bad Tacotron2 configuration");
  TTS_REQUIRE(c.encoder_dim >= 2 && c.encoder_dim % 2 == 0 && c.query_dim >= 1 && c.prenet_dim >= 1 &&
                  c.attention_dim >= 1 && c.location_filters >= 1 && c.location_kernel_size >= 1,
              1, "bad Tacotron2 widths");
  TTS_REQUIRE(c.attention_norm == 0 || c.attention_norm == 1, 1, "attention_norm must be 0 (sigmoid) or 1 (softmax)");
  TTS_REQUIRE(c.embed_dim >= 0 && c.num_speakers >= 0 && (c.num_speakers == 0 || c.embed_dim > 0), 1,
              "bad speaker embedding configuration");
  TTS_REQUIRE(c.chunk >= 0, 1, "chunk must be >= 0");
  TTS_REQUIRE(c.math_mode >= MATH_FP32 && c.math_mode <= MATH_LAST, 1, "unknown math_mode");
  TTS_REQUIRE((c.encoder_dim / 2) % kLstmUnitBlock == 0 && c.query_dim % kLstmUnitBlock == 0, 3,
              "Tacotron2: encoder_dim / 2 and query_dim must be multiples of " + std::to_string(kLstmUnitBlock));
  TTS_REQUIRE(c.attention_dim <= kT2MaxA && c.location_filters <= kT2MaxF && c.location_kernel_size <= kT2MaxLocK &&
                  c.location_kernel_size % 2 == 1,
              3, "Tacotron2: attention_dim <= 128, location_filters <= 32, odd location_kernel_size <= 31");
  TTS_REQUIRE(c.query_dim <= kT2MaxQ && c.prenet_dim <= kT2MaxP && (int64_t)c.out_channels * c.r <= kT2MaxOut, 3,
              "Tacotron2: query_dim <= 2048, prenet_dim <= 1024, out_channels * r <= 1024");
}

std::vector<int64_t> tacotron2_weight_shapes(const TtsTacotron2Cfg& c) {
  const int64_t E = c.encoder_dim, He = E / 2, Q = c.query_dim, P = c.prenet_dim, A = c.attention_dim,
                F = c.location_filters, Kl = c.location_kernel_size, C = c.out_channels, Cr = C * c.r,
                D = E + c.embed_dim;
  std::vector<int64_t> n = {(int64_t)c.num_chars * E};
  auto conv_bn = [&](int64_t co, int64_t ci) {
    for (int64_t v : {co * ci * kConvK, co, co, co, co, co}) n.push_back(v);
  };
  for (int i = 0; i < 3; ++i) conv_bn(E, E);
  for (int d = 0; d < 2; ++d)
    for (int64_t v : {4 * He * E, 4 * He * He, 4 * He, 4 * He}) n.push_back(v);
  n.push_back(P * C);
  n.push_back(P * P);
  for (int64_t v : {4 * Q * (P + D), 4 * Q * Q, 4 * Q, 4 * Q}) n.push_back(v);
  for (int64_t v : {A * Q, A * D, A, (int64_t)1, F * 2 * Kl, A * F}) n.push_back(v);
  for (int64_t v : {4 * Q * (Q + D), 4 * Q * Q, 4 * Q, 4 * Q}) n.push_back(v);
  n.push_back(Cr * (Q + D));
  n.push_back(Cr);
  n.push_back(Q + Cr);
  n.push_back(1);
  for (int i = 0; i < 5; ++i) conv_bn(i == 4 ? C : kPostnetDim, i == 0 ? C : kPostnetDim);
  if (c.num_speakers > 0) n.push_back((int64_t)c.num_speakers * c.embed_dim);
  return n;
}

Tacotron2::Tacotron2(const TtsTacotron2Cfg& cfg, const float* const* hw, int device) : cfg_(cfg), device_(device) {
  tacotron2_validate(cfg_);
  DeviceGuard g(device_);
  conv_mode_ = cfg_.math_mode == MATH_BF16 ? MATH_BF16 : MATH_FP32_X6;
  const bool bf16 = cfg_.math_mode == MATH_BF16;
  E_ = cfg_.encoder_dim; He_ = E_ / 2; Q_ = cfg_.query_dim; P_ = cfg_.prenet_dim; A_ = cfg_.attention_dim;
  F_ = cfg_.location_filters; Kl_ = cfg_.location_kernel_size; C_ = cfg_.out_channels; Cr_ = C_ * cfg_.r;
  D_ = E_ + cfg_.embed_dim;
  const auto shapes = tacotron2_weight_shapes(cfg_);
  for (size_t i = 0; i < shapes.size(); ++i)
    TTS_REQUIRE(hw[i] != nullptr, 1, "weight pointer " + std::to_string(i) + " is NULL");
  HostArena arena;
  auto put_conv = [&](PackedConv& cv, const float* w, const float* b, int Cout, int Cin, int K) {
    cv.Cin = Cin; cv.Cout = Cout; cv.K = K;
    cv.tile = conv_tile_for(conv_mode_, Cout, K, Cin, 1, false);
    TTS_REQUIRE(arena.put_conv(cv, conv_mode_, conv_tile(conv_mode_, cv.tile), w, b) == 0, 3,
                "Tacotron2: scaled packing unsupported");
  };
  // conv + BatchNorm1d (running statistics) folded in fp64: w' = w s, b' = (b - mean) s + beta, s = gamma / sqrt(var + eps)
  auto put_conv_bn = [&](PackedConv& cv, const float* const* p, int Cout, int Cin) {
    std::vector<float> w((size_t)Cout * Cin * kConvK), b(Cout);
    for (int co = 0; co < Cout; ++co) {
      const double s = (double)p[2][co] / std::sqrt((double)p[5][co] + kEpsBn);
      for (int i = 0; i < Cin * kConvK; ++i)
        w[(size_t)co * Cin * kConvK + i] = (float)((double)p[0][(size_t)co * Cin * kConvK + i] * s);
      b[co] = (float)(((double)p[1][co] - (double)p[4][co]) * s + (double)p[3][co]);
    }
    put_conv(cv, w.data(), b.data(), Cout, Cin, kConvK);
  };
  auto put_lstm = [&](Lstm& L, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int H, int I,
                      bool b16) {
    L.H = H; L.I = I; L.bf16 = b16;
    const size_t off = arena.alloc((size_t)packed_lstm_numel(H, I + H, b16), &L.w);
    pack_lstm(w_ih, w_hh, H, I, b16, arena.at(off));
    if (b_ih || b_hh) {
      const size_t ob = arena.alloc((size_t)4 * H, &L.b);
      pack_lstm_bias(b_ih, b_hh, H, arena.at(ob));
    }
  };
  auto put_t = [&](const float* w, int rows, int cols, float** dst) {  // w [rows][cols] -> [cols][rows]
    const size_t off = arena.alloc((size_t)rows * cols, dst);
    float* o = arena.at(off);
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) o[(size_t)c * rows + r] = w[(size_t)r * cols + c];
  };
  size_t wi = 0;
  arena.put(hw[wi++], (size_t)cfg_.num_chars * E_, &emb_);
  for (int i = 0; i < 3; ++i, wi += 6) put_conv_bn(enc_conv_[i], hw + wi, E_, E_);
  {  // W_ih x + b_ih + b_hh of both directions: one 1x1 conv of 8 He rows; the steps add W_hh h
    std::vector<float> w((size_t)8 * He_ * E_), b((size_t)8 * He_);
    for (int d = 0; d < 2; ++d) {
      const float* const* p = hw + wi + 4 * d;
      std::copy(p[0], p[0] + (size_t)4 * He_ * E_, w.begin() + (size_t)d * 4 * He_ * E_);
      for (int i = 0; i < 4 * He_; ++i) b[(size_t)d * 4 * He_ + i] = p[2][i] + p[3][i];
      put_lstm(enc_lstm_[d], nullptr, p[1], nullptr, nullptr, He_, 0, false);
    }
    put_conv(enc_pre_, w.data(), b.data(), 8 * He_, E_, 1);
    wi += 8;
  }
  put_t(hw[wi], P_, C_, &prenet0t_);
  put_t(hw[wi + 1], P_, P_, &prenet1t_);
  wi += 2;
  put_lstm(att_rnn_, hw[wi], hw[wi + 1], hw[wi + 2], hw[wi + 3], Q_, P_ + D_, bf16);
  wi += 4;
  arena.put(hw[wi], (size_t)A_ * Q_, &wq_);
  put_t(hw[wi + 1], A_, D_, &win_t_);
  arena.put(hw[wi + 2], A_, &v_);
  arena.put(hw[wi + 3], 1, &vb_);
  arena.put(hw[wi + 4], (size_t)F_ * 2 * Kl_, &loc_w_);
  arena.put(hw[wi + 5], (size_t)A_ * F_, &loc_d_);
  wi += 6;
  put_lstm(dec_rnn_, hw[wi], hw[wi + 1], hw[wi + 2], hw[wi + 3], Q_, Q_ + D_, bf16);
  wi += 4;
  {
    const size_t off = arena.alloc((size_t)packed_skinny_numel(Cr_, Q_ + D_, false), &proj_w_);
    pack_skinny_rows(hw[wi], Cr_, Q_ + D_, false, arena.at(off));
    arena.put(hw[wi + 1], Cr_, &proj_b_);
    arena.put(hw[wi + 2], (size_t)Q_ + Cr_, &stop_w_);
    arena.put(hw[wi + 3], 1, &stop_b_);
    wi += 4;
  }
  for (int i = 0; i < 5; ++i, wi += 6)
    put_conv_bn(post_conv_[i], hw + wi, i == 4 ? C_ : kPostnetDim, i == 0 ? C_ : kPostnetDim);
  if (cfg_.num_speakers > 0) arena.put(hw[wi++], (size_t)cfg_.num_speakers * cfg_.embed_dim, &spk_);
  TTS_REQUIRE(wi == shapes.size(), 2, "internal: Tacotron2 weight count mismatch");
  arena.upload(device_, arena_);
}

void Tacotron2::conv(const PackedConv& cv, const float* x, float* y, const float* mask, float out_slope, int B, int T,
                     hipStream_t s, Profiler* prof, const char* name) {
  Conv1dArgs a{};
  a.x = x; a.w = cv.w; a.bias = cv.b; a.y = y; a.mask = mask;
  a.Cin = cv.Cin; a.Cout = cv.Cout; a.Tin = T; a.Tout = T;
  a.dil = 1; a.pad = (cv.K - 1) / 2; a.n_chunks = cv.n_chunks;
  a.in_slope = 1.f; a.out_slope = out_slope; a.zmode = 0; a.zdiv = 1.f;
  const double P = (double)B * T;
  run(prof, s, name, 2.0 * P * cv.Cout * cv.Cin * cv.K, 4.0 * P * (cv.Cin + cv.Cout),
      [&] { launch_conv(conv_mode_, a, B, cv.K, cv.tile, s); });
}

void Tacotron2::encode(const int64_t* tok, const int64_t* x_len, const int64_t* spk, const float* dvec, int B, int T,
                       float* inputs, float* pinp, hipStream_t s, Profiler* prof) {
  TTS_REQUIRE(tok && inputs && pinp, 1, "NULL input/output pointer");
  TTS_REQUIRE(B >= 1 && T >= 1, 1, "batch and token count must be >= 1");
  TTS_REQUIRE(B <= kSkinnyMaxBatch, 3, "Tacotron2: more than " + std::to_string(kSkinnyMaxBatch) + " utterances");
  TTS_REQUIRE(T <= TTS_TACOTRON2_MAX_TOKENS, 3,
              "Tacotron2: more than " + std::to_string(TTS_TACOTRON2_MAX_TOKENS) + " tokens per utterance");
  const int W = cfg_.embed_dim;
  TTS_REQUIRE(cfg_.num_speakers == 0 || spk, 1, "this model has a speaker embedding: pass speaker ids");
  TTS_REQUIRE(cfg_.num_speakers > 0 || W == 0 || dvec, 1, "this model takes d-vectors: pass them");
  DeviceGuard dg(device_);
  const int BT = skinny_batch_tile(B);
  const size_t plane = al((size_t)B * E_ * T), st = al((size_t)He_ * BT);
  ws_.grow(device_, (2 * plane + al((size_t)B * 8 * He_ * T) + 6 * st) * sizeof(float), "workspace");
  float* X0 = ws_.as<>();
  float* X1 = X0 + plane;
  float* PRE = X1 + plane;
  float* state = PRE + al((size_t)B * 8 * He_ * T);  // h[2 buffers][2 directions], c[2 directions]
  run(prof, s, "enc_embed", 0.0, 4.0 * B * T * E_,
      [&] { launch_t2_embed(tok, emb_, X0, B, E_, T, cfg_.num_chars, s); });
  conv(enc_conv_[0], X0, X1, nullptr, 0.f, B, T, s, prof, "enc_conv0");
  conv(enc_conv_[1], X1, X0, nullptr, 0.f, B, T, s, prof, "enc_conv1");
  conv(enc_conv_[2], X0, X1, nullptr, 0.f, B, T, s, prof, "enc_conv2");
  conv(enc_pre_, X1, PRE, nullptr, 1.f, B, T, s, prof, "enc_lstm_input");
  TTS_HIP_CHECK(hipMemsetAsync(state, 0, 6 * st * sizeof(float), s));
  TTS_HIP_CHECK(hipMemsetAsync(inputs, 0, (size_t)B * T * D_ * sizeof(float), s));
  SkinnyArgs a{};
  a.K = He_; a.Kp = skinny_kp(He_); a.B = B; a.BT = BT; a.bf16 = 0; a.ndir = 2; a.lstm = 1; a.H = He_;
  a.n[2] = He_;
  a.pre = PRE; a.y = inputs; a.T = T; a.ldy = D_; a.len = x_len;
  for (int d = 0; d < 2; ++d) {
    a.w[d] = enc_lstm_[d].w;
    a.c[d] = state + (4 + d) * st;
  }
  run(prof, s, "enc_lstm_steps", 2.0 * T * 2 * 4 * He_ * He_ * B, 4.0 * T * 2 * 4 * He_ * He_, [&] {
    for (int t = 0; t < T; ++t) {
      for (int d = 0; d < 2; ++d) {
        a.x[d][2] = state + ((t & 1) * 2 + d) * st;
        a.h_out[d] = state + (((t + 1) & 1) * 2 + d) * st;
      }
      a.step = t;
      launch_skinny(a, s);
    }
  });
  if (W > 0)
    run(prof, s, "enc_speaker", 0.0, 4.0 * B * T * W,
        [&] { launch_t2_speaker(cfg_.num_speakers > 0 ? spk : nullptr, spk_, cfg_.num_speakers, dvec, inputs, B, T, E_, W, s); });
  run(prof, s, "inputs_layer", 2.0 * B * T * D_ * A_, 4.0 * B * T * (D_ + A_),
      [&] { launch_t2_processed_inputs(inputs, win_t_, pinp, B, T, D_, A_, s); });
}

int Tacotron2::decode(const float* inputs, const float* pinp, const int64_t* x_len, int B, int T, int S,
                      float stop_threshold, float* dec_out, float* align, float* stop_tokens, int* steps, hipStream_t s,
                      Profiler* prof) {
  TTS_REQUIRE(B >= 1 && T >= 1, 1, "batch and token count must be >= 1");
  TTS_REQUIRE(B <= kSkinnyMaxBatch, 3, "Tacotron2: more than " + std::to_string(kSkinnyMaxBatch) + " utterances");
  TTS_REQUIRE(T <= TTS_TACOTRON2_MAX_TOKENS, 3,
              "Tacotron2: more than " + std::to_string(TTS_TACOTRON2_MAX_TOKENS) + " tokens per utterance");
  TTS_REQUIRE(S >= 1, 3, "Tacotron2: max_decoder_steps must be >= 1");
  TTS_REQUIRE(inputs && pinp && dec_out && align && stop_tokens && steps, 1, "NULL input/output pointer");
  DeviceGuard dg(device_);
  const int BT = skinny_batch_tile(B);
  const size_t nP = al((size_t)P_ * BT), nD = al((size_t)D_ * BT), nQ = al((size_t)Q_ * BT), nT = al((size_t)B * T);
  const size_t nstate = nP + nD + 6 * nQ + 4 * nT + 64;
  ws_.grow(device_, nstate * sizeof(float), "workspace");
  float* p = ws_.as<>();
  float* ctx = p + nP;
  float* q[2] = {ctx + nD, ctx + nD + nQ};
  float* hd[2] = {q[1] + nQ, q[1] + 2 * nQ};
  float* ca = hd[1] + nQ;
  float* cd = ca + nQ;
  float* aw[2] = {cd + nQ, cd + nQ + nT};
  float* awc[2] = {aw[1] + nT, aw[1] + 2 * nT};
  int* done = reinterpret_cast<int*>(awc[1] + nT);  // [32] done, [32..33] counters
  int* counters = done + kSkinnyMaxBatch;
  // the go frame, both RNN states, the context and the attention weights start at zero; so does the
  // prenet of the zero go frame (no bias)
  TTS_HIP_CHECK(hipMemsetAsync(p, 0, nstate * sizeof(float), s));
  TTS_HIP_CHECK(hipMemsetAsync(dec_out, 0, (size_t)B * S * Cr_ * sizeof(float), s));
  TTS_HIP_CHECK(hipMemsetAsync(align, 0, (size_t)B * S * T * sizeof(float), s));
  TTS_HIP_CHECK(hipMemsetAsync(stop_tokens, 0, (size_t)B * S * sizeof(float), s));
  TTS_HIP_CHECK(hipMemsetAsync(steps, 0, (size_t)B * sizeof(int), s));

  SkinnyArgs ra{};  // attention RNN: [prenet | context | query]
  ra.w[0] = att_rnn_.w; ra.bias[0] = att_rnn_.b; ra.n[0] = P_; ra.n[1] = D_; ra.n[2] = Q_;
  ra.K = P_ + D_ + Q_; ra.Kp = skinny_kp(ra.K); ra.B = B; ra.BT = BT; ra.bf16 = att_rnn_.bf16; ra.ndir = 1;
  ra.lstm = 1; ra.H = Q_; ra.c[0] = ca; ra.done = done; ra.x[0][0] = p; ra.x[0][1] = ctx;
  SkinnyArgs rd = ra;  // decoder RNN: [query | context | decoder hidden]
  rd.w[0] = dec_rnn_.w; rd.bias[0] = dec_rnn_.b; rd.n[0] = Q_; rd.K = 2 * Q_ + D_; rd.Kp = skinny_kp(rd.K);
  rd.bf16 = dec_rnn_.bf16; rd.c[0] = cd;
  SkinnyArgs pj{};  // projection: [decoder hidden | context]
  pj.w[0] = proj_w_; pj.bias[0] = proj_b_; pj.n[0] = Q_; pj.n[1] = D_; pj.K = Q_ + D_; pj.Kp = skinny_kp(pj.K);
  pj.B = B; pj.BT = BT; pj.ndir = 1; pj.lstm = 0; pj.R = Cr_; pj.ldo = (int64_t)S * Cr_; pj.done = done;
  pj.x[0][1] = ctx;
  T2AttnArgs at{};
  at.wq = wq_; at.loc_w = loc_w_; at.loc_d = loc_d_; at.pinp = pinp; at.v = v_; at.v_bias = vb_; at.inputs = inputs;
  at.len = x_len; at.done = done; at.ctx = ctx; at.align = align;
  at.B = B; at.BT = BT; at.T = T; at.D = D_; at.A = A_; at.F = F_; at.Kl = Kl_; at.Q = Q_; at.S = S;
  at.softmax = cfg_.attention_norm;
  T2StopArgs sp{};
  sp.dec_out = dec_out; sp.stop_w = stop_w_; sp.stop_b = stop_b_; sp.w0t = prenet0t_; sp.w1t = prenet1t_;
  sp.prenet = p; sp.stop_tokens = stop_tokens; sp.done = done; sp.steps = steps; sp.counters = counters;
  sp.B = B; sp.BT = BT; sp.Q = Q_; sp.C = C_; sp.r = cfg_.r; sp.P = P_; sp.S = S; sp.max_steps = S;
  sp.threshold = stop_threshold;

  const double wbytes = att_rnn_.bf16 ? 2.0 : 4.0;
  const int chunk = cfg_.chunk > 0 ? cfg_.chunk : 32;
  int step = 0, all_done = 0;
  while (step < S && !all_done) {
    const int end = std::min(S, step + chunk);
    for (; step < end; ++step) {
      const int cur = step & 1, nxt = cur ^ 1;
      ra.x[0][2] = q[cur]; ra.h_out[0] = q[nxt];
      run(prof, s, "attention_rnn", 2.0 * 4 * Q_ * ra.K * B, wbytes * 4 * Q_ * ra.K, [&] { launch_skinny(ra, s); });
      at.query = q[nxt]; at.aw_in = aw[cur]; at.awc_in = awc[cur]; at.aw_out = aw[nxt]; at.awc_out = awc[nxt];
      at.step = step;
      run(prof, s, "attention", 2.0 * B * ((double)A_ * Q_ + (double)T * (F_ * 2 * Kl_ + A_ * F_ + D_)),
          4.0 * B * ((double)A_ * Q_ + (double)T * (A_ + D_)), [&] { launch_t2_attention(at, s); });
      rd.x[0][0] = q[nxt]; rd.x[0][2] = hd[cur]; rd.h_out[0] = hd[nxt];
      run(prof, s, "decoder_rnn", 2.0 * 4 * Q_ * rd.K * B, wbytes * 4 * Q_ * rd.K, [&] { launch_skinny(rd, s); });
      pj.x[0][0] = hd[nxt]; pj.out = dec_out + (size_t)step * Cr_;
      run(prof, s, "projection", 2.0 * Cr_ * pj.K * B, 4.0 * Cr_ * pj.K, [&] { launch_skinny(pj, s); });
      sp.hd = hd[nxt]; sp.step = step;
      run(prof, s, "stop_prenet", 2.0 * B * (Q_ + Cr_ + (double)P_ * (C_ + P_)), 4.0 * P_ * (C_ + P_),
          [&] { launch_t2_stop_prenet(sp, s); });
    }
    TTS_HIP_CHECK(hipMemcpyAsync(&all_done, counters + 1, sizeof(int), hipMemcpyDeviceToHost, s));
    TTS_HIP_CHECK(hipStreamSynchronize(s));
  }
  // the last step ends every utterance, so steps[] is complete here
  int hs[kSkinnyMaxBatch];
  TTS_HIP_CHECK(hipMemcpyAsync(hs, steps, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
  TTS_HIP_CHECK(hipStreamSynchronize(s));
  return *std::max_element(hs, hs + B);
}

void Tacotron2::postnet(const float* dec_out, const int* steps, int B, int S, int row_stride, float* model_out,
                        hipStream_t s, Profiler* prof) {
  TTS_REQUIRE(dec_out && steps && model_out, 1, "NULL input/output pointer");
  TTS_REQUIRE(B >= 1 && S >= 1 && row_stride >= S, 1, "batch and step count must be >= 1, row_stride >= steps");
  DeviceGuard dg(device_);
  const int L = S * cfg_.r;
  const size_t plane = al((size_t)B * std::max(kPostnetDim, C_) * L);
  ws_.grow(device_, (2 * plane + al((size_t)B * L)) * sizeof(float), "workspace");
  float* X0 = ws_.as<>();
  float* X1 = X0 + plane;
  float* mask = X1 + plane;
  const int64_t bstride = (int64_t)row_stride * Cr_;
  run(prof, s, "postnet_planes", 0.0, 8.0 * B * L * C_,
      [&] { launch_t2_to_planes(dec_out, steps, cfg_.r, X0, mask, B, C_, L, bstride, s); });
  float *x = X0, *y = X1;
  for (int i = 0; i < 5; ++i) {
    // masked after every layer: an utterance sees zeros past its own end, as a batch of one does
    conv(post_conv_[i], x, y, mask, 1.f, B, L, s, prof, "postnet_conv");
    if (i < 4)
      run(prof, s, "postnet_tanh", 0.0, 8.0 * B * L * kPostnetDim,
          [&] { launch_t2_tanh(y, (int64_t)B * kPostnetDim * L, s); });
    std::swap(x, y);
  }
  run(prof, s, "postnet_residual", 0.0, 12.0 * B * L * C_,
      [&] { launch_t2_residual_out(dec_out, x, mask, model_out, B, C_, L, bstride, s); });
}

void op_lstm_cell(const float* d_x, const float* d_h, const float* d_c, int B, int I, int H, const float* w_ih,
                  const float* w_hh, const float* b_ih, const float* b_hh, int math_mode, float* d_h_out,
                  float* d_c_out, hipStream_t s) {
  TTS_REQUIRE(d_x && d_h && d_c && w_ih && w_hh && d_h_out && d_c_out, 1, "NULL argument");
  TTS_REQUIRE(B >= 1 && I >= 1 && H >= 1, 1, "batch and sizes must be >= 1");
  TTS_REQUIRE(math_mode >= MATH_FP32 && math_mode <= MATH_LAST, 1, "unknown math_mode");
  TTS_REQUIRE(B <= kSkinnyMaxBatch, 3, "LSTM: more than " + std::to_string(kSkinnyMaxBatch) + " batch columns");
  const bool bf16 = math_mode == MATH_BF16;
  HostArena arena;
  float *w = nullptr, *bias = nullptr;
  const size_t off = arena.alloc((size_t)packed_lstm_numel(H, I + H, bf16), &w);
  pack_lstm(w_ih, w_hh, H, I, bf16, arena.at(off));
  const size_t ob = arena.alloc((size_t)4 * H, &bias);
  pack_lstm_bias(b_ih, b_hh, H, arena.at(ob));
  int dev = 0;
  TTS_HIP_CHECK(hipGetDevice(&dev));
  DeviceBuffer wbuf, st;
  arena.upload(dev, wbuf);
  const int BT = skinny_batch_tile(B);
  const size_t nI = al((size_t)I * BT), nH = al((size_t)H * BT);
  st.grow(dev, (nI + 3 * nH) * sizeof(float), "operand");
  float* x = st.as<>();
  float* h = x + nI;
  float* c = h + nH;
  float* ho = c + nH;
  TTS_HIP_CHECK(hipMemsetAsync(x, 0, (nI + 3 * nH) * sizeof(float), s));
  launch_t2_transpose(d_x, x, B, I, I, BT, s);
  launch_t2_transpose(d_h, h, B, H, H, BT, s);
  launch_t2_transpose(d_c, c, B, H, H, BT, s);
  SkinnyArgs a{};
  a.w[0] = w; a.bias[0] = bias; a.x[0][0] = x; a.x[0][2] = h; a.n[0] = I; a.n[2] = H;
  a.K = I + H; a.Kp = skinny_kp(a.K); a.B = B; a.BT = BT; a.bf16 = bf16; a.ndir = 1; a.lstm = 1; a.H = H;
  a.c[0] = c; a.h_out[0] = ho;
  launch_skinny(a, s);
  launch_t2_transpose(ho, d_h_out, H, B, BT, H, s);
  launch_t2_transpose(c, d_c_out, H, B, BT, H, s);
  TTS_HIP_CHECK(hipStreamSynchronize(s));  // the operand buffers are freed on return
}

}  // namespace tts
