// XTTS GPT (the autoregressive GPT-2 trunk of XTTS): executor (xtts_gpt.cpp), its kernels
// (kernels_xtts_gpt.hip) and the host packer of the HF Conv1D matrices (pack.cpp).  Semantics:
// TTS/tts/layers/xtts/gpt.py, gpt_inference.py (Coqui TTS 0.22.0) as restated in DESIGN.md section 4.
#pragma once

#include <vector>

#include "common.hpp"
#include "hifigan.hpp"
#include "fft_attn.hpp"
#include "tacotron2.hpp"
#include "tts_mi355x.h"

namespace tts {

constexpr int kGptMaxBatch = TTS_XTTS_GPT_MAX_BATCH;
constexpr int kGptMaxVocab = TTS_XTTS_GPT_MAX_AUDIO_TOKENS;
constexpr int kGptAttnWaves = 8;   // waves of one (utterance, head) workgroup of the decode attention
constexpr int kGptAttnTile = 64;   // cached keys one wave takes per pass (one per lane)
constexpr float kGptLnEps = 1e-5f;

// HF Conv1D weight w [K][R] (y = x w + b) as the skinny image of its transpose: out[rb][k][j] =
// w[k][16 rb + j], rows padded with zeros to whole blocks of 16, k to skinny_kp(K)
void pack_skinny_cols(const float* w, int K, int R, bool bf16, float* out);

// ---- decode-step product [R x K] . [K x B] with a LayerNorm prologue and a fused epilogue ----
// The weights are a packed skinny image (tacotron2.hpp); x is batch-minor, x[k * BT + b].
enum GptEpilogue {
  kGptEpiQkv = 0,       // + bias; rows [0, E) -> q[b][row], [E, 2E) / [2E, 3E) -> row pos_b of the K / V cache
  kGptEpiResidual = 1,  // out[row][b] += v + bias
  kGptEpiGelu = 2,      // out[row][b] = gelu_new(v + bias)
  kGptEpiLogits = 3,    // logits[b][row] = v + bias (and logits2, if given)
};
struct GptSkinnyArgs {
  const void* w;
  const float* bias;     // [R]
  const float* x;        // [K][BT]
  const float* ln_g[2];  // nln LayerNorms applied to x in sequence before the product (0, 1 or 2)
  const float* ln_b[2];
  int nln;
  int K, Kp, R, B, BT, bf16, epi;
  const int* skip;       // [B]: utterances with skip[b] != 0 are left untouched
  // kGptEpiQkv: the cache row is pos_b = (base ? base[b] : 0) + off, of cap rows per utterance
  float* q;              // [B][E]
  float* kc;             // [B][cap][E]
  float* vc;
  const int* base;
  int off, cap, E;
  // kGptEpiResidual / kGptEpiGelu
  float* out;            // [R][BT], never x
  // kGptEpiLogits
  float* logits;         // [b * ld_logits + row]
  int64_t ld_logits;
  float* logits2;        // a second copy, or nullptr
  int64_t ld_logits2;
  // the normalised input itself, written by the first workgroup: lat[b * ld_lat + k] while
  // lat_step < (lat_n ? lat_n[b] - 2 : INT_MAX); nullptr: not written
  float* lat;
  int64_t ld_lat;
  const int* lat_n;
  int lat_step;
  int lat_only;  // 1: one workgroup writes lat and the product is not run (no logits wanted)
};
void launch_gpt_skinny(const GptSkinnyArgs& a, hipStream_t s);

// ---- single-query attention over the cache: out[(h dk + d) * BT + b] ----
struct GptAttnArgs {
  const float* q;   // [B][E]
  const float* kc;  // [B][cap][E]
  const float* vc;
  const int* base;  // utterance b attends to keys [0, (base ? base[b] : 0) + off]
  int off, cap, E, heads, dk, B, BT;
  const int* skip;
  float* out;       // [E][BT]
};
void launch_gpt_decode_attn(const GptAttnArgs& a, hipStream_t s);

// ---- logits -> token, bookkeeping, next input ----
struct GptSampleArgs {
  const float* logits;  // [B][V]
  int V, B, BT, E;
  float penalty, temperature, top_p;
  int top_k;
  const float* u;       // u[b * ldu + u_off]: a uniform in [0, 1) per utterance, or nullptr: greedy
  int64_t ldu;
  int u_off;
  int* codes;           // [B][S]: codes[b][0 .. step) are the utterance's earlier codes
  int S, step, max_steps;
  int start_audio, stop_audio;
  int* done;            // [B], or nullptr (the op)
  int* n;               // [B]
  int* counters;        // [0] utterances ended, [1] all ended
  const float* mel_emb; // [V][E], or nullptr: no next input (the op)
  const float* mel_pos; // [positions][E]
  float* x;             // [E][BT]
};
void launch_gpt_sample(const GptSampleArgs& a, hipStream_t s);

// ---- the input row of a step ----
struct GptEmbedArgs {
  int mel;                 // 0: prefix row t, 1: mel position t
  int t;
  // prefix: [cond (P rows) | start_text, text, stop_text]
  const float* cond;       // [B][P][E]
  const int64_t* text;     // [B][T]
  const int64_t* text_len; // [B] or nullptr (T)
  const float* text_emb;
  const float* text_pos;
  int P, T, n_text, start_text, stop_text;
  int* plen;               // [B]: receives P + L_b + 2
  // mel: [start_audio, c_0 .. c_{n-1}, stop_audio]; codes == nullptr: the start token alone (t = 0)
  const int* codes;        // [B][S]
  const int* n;            // [B]
  const float* mel_emb;
  const float* mel_pos;
  int S, n_audio, start_audio, stop_audio;
  int* skip;               // [B]: set when utterance b has no row t (prefix: t >= plen; mel: t >= n_b + 2)
  float* x;                // [E][BT]
  int B, BT, E;
};
void launch_gpt_embed(const GptEmbedArgs& a, hipStream_t s);

// ---- whole-sequence pass (prefill, latent pass) on the conv path: planes [B][C][T] ----
// Row t of utterance b's sequence [prefix (plen_b rows) | mel rows]: zeros at and past its length.
struct GptSeqEmbedArgs {
  // from_pre == 0: the prefix from its sources (the prefill; its rows are also saved to pre);
  // from_pre == 1: from the rows in pre, plen read (the latent pass)
  int from_pre;
  const float* cond;       // [B][P][E], NULL with P = 0
  const int64_t* text;     // [B][Ttext]
  const int64_t* text_len;
  const float* text_emb;
  const float* text_pos;
  int P, Ttext, n_text, start_text, stop_text;
  float* pre;              // [B][pre_rows][E]: the prefix's input rows
  int pre_rows;
  // the mel rows [start_audio, c_0 .. c_{n-1}, stop_audio], at most `rows` of them; codes == nullptr: none
  const int* codes;        // [B][S]
  const int* n;
  const float* mel_emb;
  const float* mel_pos;
  int S, rows, n_audio, start_audio, stop_audio;
  int* plen;               // [B]: written (from the sources) or read (from pre)
  int64_t* klen;           // [B]: receives the sequence length
  float* x;                // [B][E][T]
  int B, E, T;
};
void launch_gpt_seq_embed(const GptSeqEmbedArgs& a, hipStream_t s);
// y = LayerNorm over the channels (any C); y may be x
void launch_gpt_seq_layernorm(const float* x, const float* gamma, const float* beta, float* y, int B, int C, int T,
                              hipStream_t s);
void launch_gpt_seq_gelu(float* x, int64_t n, hipStream_t s);
// kc / vc [B][cap][E] rows t < klen[b] from qkv [B][3E][T]
void launch_gpt_seq_kv(const float* qkv, const int64_t* klen, float* kc, float* vc, int B, int E, int T, int cap,
                       hipStream_t s);
// x[k][b] = h[b][k][plen_b + s]; skip[b] = s >= n_b + 2
void launch_gpt_seq_column(const float* h, const int* plen, const int* n, int S, int s_, int B, int E, int T, int BT,
                           float* x, int* skip, hipStream_t s);

// kernel-test ops (pack / upload / run / synchronise)
void op_gpt_decode_attn(const float* d_q, const float* d_k, const float* d_v, const int* d_lens, int B, int E, int heads,
                        int cap, float* d_out, hipStream_t s);
// d_codes [B][n_prev + 1]: the earlier codes, then the slot that receives the token; d_u [B] or nullptr
void op_gpt_sample(const float* d_logits, int B, int V, int* d_codes, int n_prev, int start_audio, float penalty,
                   float temperature, int top_k, float top_p, const float* d_u, hipStream_t s);

void xtts_gpt_validate(const TtsXttsGptCfg& c);
std::vector<int64_t> xtts_gpt_weight_shapes(const TtsXttsGptCfg& c);

class XttsGpt {
 public:
  XttsGpt(const TtsXttsGptCfg& cfg, const float* const* host_weights, int device);
  // one whole-sequence pass over the prefix on the conv path; leaves its keys and values in the cache
  void prefill(const float* cond, const int64_t* tok, const int64_t* text_len, int B, int T, int max_new_tokens,
               hipStream_t s, Profiler* prof = nullptr);
  // returns the number of steps enqueued
  int generate(int S, float penalty, float temperature, int top_k, float top_p, const float* u, int* codes, int* lengths,
               float* logits, float* latents, hipStream_t s, Profiler* prof = nullptr);
  void latents(const int* codes, const int* lengths, int S, int rows, float* lat, float* logits, hipStream_t s,
               Profiler* prof = nullptr);
  int device() const { return device_; }

 private:
  struct Layer {
    float *ln1_g, *ln1_b, *w_qkv, *b_qkv, *w_proj, *b_proj, *ln2_g, *ln2_b, *w_fc, *b_fc, *w_mp, *b_mp;
    PackedConv c_qkv, c_proj, c_fc, c_mp;  // the same matrices as 1x1 convs of the whole-sequence pass
  };
  struct Ws {
    float *x, *att, *h4, *q, *logits, *kc, *vc;
    float *pre, *X0, *X1, *A, *Wd;  // the prefix's input rows; planes [B][E | 4E][cap]
    int64_t* klen;
    int *skip, *done, *plen, *n, *counters;
    size_t layer_stride;  // floats between two layers' caches
  };
  Ws carve(int B, int cap) const;
  size_t ws_floats(int B, int cap) const;
  // the layers over planes of T positions, K and V of every layer into the cache; returns the hidden plane
  float* seq_layers(const Ws& w, int T, hipStream_t s, Profiler* prof);
  void layers(const Ws& w, const int* base, int off, const int* skip, hipStream_t s, Profiler* prof);
  // lat_only: the latent row alone, mel_head is not run
  void head(const Ws& w, const int* skip, float* logits2, int64_t ld2, float* lat, int64_t ld_lat, const int* lat_n,
            int lat_step, bool lat_only, hipStream_t s, Profiler* prof);

  TtsXttsGptCfg cfg_;
  int device_;
  bool bf16_;
  int conv_mode_;  // MATH_FP32_X6 (bf16 mode: on bf16-rounded matrices)
  int E_, H_, dk_, L_, V_, P_;
  std::vector<Layer> layer_;
  float *text_emb_ = nullptr, *mel_emb_ = nullptr, *text_pos_ = nullptr, *mel_pos_ = nullptr;
  float *lnf_g_ = nullptr, *lnf_b_ = nullptr, *fn_g_ = nullptr, *fn_b_ = nullptr, *head_w_ = nullptr, *head_b_ = nullptr;
  DeviceBuffer arena_, ws_;
  // the prefix a prefill left in the cache
  int B_ = 0, BT_ = 0, cap_ = 0, max_new_ = 0, pre_rows_ = 0;
};

}  // namespace tts
