/*
 * tts_mi355x.h — C-ABI of the MI355X-native mel→waveform path.
 *
 * This library replaces, for inference on gfx950, the PyTorch-ATen compute under two
 * reference modules of Coqui TTS 0.22.0 (paths relative to the reference repo root):
 *
 *   HiFiGAN generator  TTS/vocoder/models/hifigan_generator.py
 *       HifiganGenerator.__init__        :163-234   -> tts_hifigan_create
 *       HifiganGenerator.forward         :236-265   -> tts_hifigan_forward (pad = 0)
 *       HifiganGenerator.inference       :267-282   -> tts_hifigan_forward (pad = inference_padding)
 *       HifiganGenerator.remove_weight_norm :284-291 (weights arrive already folded)
 *   Glow-TTS decoder   TTS/tts/layers/glow_tts/decoder.py
 *       Decoder.__init__                 :68-111    -> tts_glow_decoder_create
 *       Decoder.forward(reverse=True/False) :113-137 -> tts_glow_decoder_forward
 *       Decoder.store_inverse            :139-141   (W^-1 arrives precomputed)
 *   Glow-TTS encoder   TTS/tts/layers/glow_tts/encoder.py (rel_pos_transformer)
 *       Encoder.__init__                 :83-141    -> tts_glow_encoder_create
 *       Encoder.forward                  :143-179   -> tts_glow_encoder_forward
 *   TTS -> vocoder hand-off  TTS/utils/synthesizer.py:412-428 -> tts_mel_handoff
 *   save_wav int16 scaling   TTS/utils/audio/numpy_transforms.py:430-447 -> tts_wav_to_int16
 *   Glow-TTS inference glue  TTS/tts/models/glow_tts.py
 *       GlowTTS.inference durations      :349-351   -> tts_glow_durations
 *       generate_path + compute_outputs + z :352-361 -> tts_glow_expand
 *       GlowTTS.forward / inference_with_MAS logp :218-228 -> tts_glow_mas_logp
 *       maximum_path (TTS/tts/utils/helpers.py)   -> tts_maximum_path
 *
 * The reference has no native FFI for this path (it is pure Python over ATen); the Python
 * binding a maintainer adds is the ctypes stub in INTEGRATION.md.
 *
 * Conventions
 *   - All tensors are fp32, contiguous NCW ([batch][channel][time]) device pointers of the
 *     device the handle was created on.  Weights are passed as HOST pointers in the
 *     reference's PyTorch layouts (Conv1d [Cout][Cin][K], ConvTranspose1d [Cin][Cout][K]),
 *     already weight-norm-folded; the library packs them into kernel layouts once.
 *   - Every entry point returns TTS_OK (0) or a TTS_ERR_* code; no C++ exception crosses
 *     the ABI.  tts_last_error() returns the calling thread's last message.
 *   - forward calls are stream-ordered on the given hipStream_t (NULL = default stream),
 *     never synchronise (except *_profiled), never allocate after the first call for a given
 *     (B, T) or smaller (the per-handle workspace grows only).
 *   - A handle may be used from one host thread at a time; distinct handles are independent.
 */
#ifndef TTS_MI355X_H
#define TTS_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TTS_OK 0
#define TTS_ERR_INVALID 1     /* bad argument / shape (reference: ValueError / assert)      */
#define TTS_ERR_HIP 2         /* HIP runtime error                                           */
#define TTS_ERR_UNSUPPORTED 3 /* configuration outside the implemented path                 */
#define TTS_ERR_OOM 4         /* device allocation failed                                   */

/* Arithmetic of the conv contractions (both produce fp32 results from fp32 inputs):
 *   TTS_MATH_FP32     v_mfma_f32_32x32x2_f32, exact fp32 products, fp32 accumulation
 *   TTS_MATH_FP32_X6  each fp32 operand split exactly into 3 bf16 pieces, the 6 significant
 *                     cross products accumulated in fp32 on v_mfma_f32_32x32x16_bf16
 *                     (dropped terms < 2^-26 relative; 2.67x the fp32-MFMA ceiling)
 *   TTS_MATH_FP32_F16X3  each operand, scaled by an exact power of two so its max-abs lies in
 *                     [2^13, 2^14), split into hi = fp16(x) and lo = fp16(x - hi); hi*hi, hi*lo
 *                     and lo*hi accumulated in fp32 on v_mfma_f32_32x32x16_f16 (22 significant
 *                     bits per operand, dropped term ~2^-22 relative; 5.3x the fp32-MFMA
 *                     ceiling).  The
 *                     scales come from max-abs statistics each producing kernel records; the
 *                     HiFiGAN executor runs conv_pre (user input, no statistics) in FP32_X6.
 *                     HiFiGAN, the Glow decoder and the VITS flow; the Glow encoder rejects it
 *                     (TTS_ERR_UNSUPPORTED).
 *   TTS_MATH_BF16     bf16 operands on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (the bf16
 *                     arithmetic of configs 3 / 5; not fp32-faithful: ~2^-9 relative per product).
 *                     The HiFiGAN executor keeps its internal activation planes in HBM as bf16 (one
 *                     rounding per stored plane, as a bf16 PyTorch forward has; the environment
 *                     variable TTS_MI355X_BF16_PLANES=0 at create time keeps them fp32); every tensor
 *                     crossing this ABI stays fp32. */
#define TTS_MATH_FP32 0
#define TTS_MATH_FP32_X6 1
#define TTS_MATH_FP32_F16X3 2
#define TTS_MATH_BF16 3

#define TTS_MAX_UPSAMPLES 8
#define TTS_MAX_KERNELS 4
#define TTS_MAX_DILATIONS 4

/* ------------------------------------------------------------------------------------ */
/* Library                                                                               */
/* ------------------------------------------------------------------------------------ */

/* Last error message of the calling thread ("" if none). */
const char* tts_last_error(void);
/* ABI version (major*100 + minor). */
int tts_abi_version(void);
/* Target the device code was built for ("gfx950"). */
const char* tts_build_target(void);
/* Provenance: "target=gfx950 src=<16 hex>", the first 16 hex digits of the sha256 of the
 * library's sources (tts-3_amd/Makefile HASHED: sorted paths, contents concatenated) at build time. */
const char* tts_build_info(void);

/* ------------------------------------------------------------------------------------ */
/* HiFiGAN generator                                                                     */
/* ------------------------------------------------------------------------------------ */

/* Mirrors HifiganGenerator.__init__ arguments (hifigan_generator.py:163-178). */
typedef struct TtsHifiganCfg {
  int in_channels;                      /* num_mels (setup_generator, vocoder/models/__init__.py:41) */
  int out_channels;                     /* 1 */
  int resblock_type;                    /* 1 = ResBlock1 (:18-105), 2 = ResBlock2 (:108-159) */
  int num_kernels;                      /* len(resblock_kernel_sizes) */
  int resblock_kernel_sizes[TTS_MAX_KERNELS];
  int num_dilations;                    /* len(resblock_dilation_sizes[j]); 3 (type 1) or 2 (type 2) */
  int resblock_dilation_sizes[TTS_MAX_KERNELS][TTS_MAX_DILATIONS];
  int num_upsamples;                    /* len(upsample_factors) */
  int upsample_factors[TTS_MAX_UPSAMPLES];
  int upsample_kernel_sizes[TTS_MAX_UPSAMPLES];
  int upsample_initial_channel;
  int inference_padding;                /* default 5 (:173) */
  int cond_channels;                    /* 0 = no cond_layer (:227-228) */
  int conv_post_bias;                   /* default 1 (:177) */
  int math_mode;                        /* TTS_MATH_FP32 (default), _X6, _F16X3 or TTS_MATH_BF16 */
  int cond_in_each_up_layer;            /* XTTS generator (TTS/tts/layers/xtts/hifigan_decoder.py:199, :276-279):
                                           o = ups[i](o) + conds[i](g) after every upsampling; needs cond_channels */
} TtsHifiganCfg;

/* Number of host weight tensors create() expects, and the element count of tensor idx.
 * Order (state_dict order of the reference module after remove_weight_norm):
 *   conv_pre.weight [C0][in][7], conv_pre.bias [C0]
 *   for i < num_upsamples:  ups.i.weight [C_i][C_i/2][k_i], ups.i.bias [C_i/2]
 *   for r < num_upsamples*num_kernels (resblocks.r):
 *       type 1: convs1.m.weight/bias for m < 3, then convs2.m.weight/bias for m < 3
 *       type 2: convs.m.weight/bias for m < num_dilations
 *   conv_post.weight [out][C_last][7], conv_post.bias [out] (only if conv_post_bias)
 *   cond_layer.weight [C0][cond][1], cond_layer.bias [C0]  (only if cond_channels > 0)
 *   conds.i.weight [C_{i+1}][cond][1], conds.i.bias [C_{i+1}] for i < num_upsamples
 *                                                          (only if cond_in_each_up_layer)
 * with C0 = upsample_initial_channel, C_i = C0 >> i. */
int tts_hifigan_num_weights(const TtsHifiganCfg* cfg);
int64_t tts_hifigan_weight_numel(const TtsHifiganCfg* cfg, int idx);

/* Build a generator on HIP device `device`: validates cfg, packs + uploads weights. */
int tts_hifigan_create(const TtsHifiganCfg* cfg, const float* const* host_weights, int device,
                       void** handle);
int tts_hifigan_destroy(void* handle);

/* Output samples per batch item: prod(upsample_factors) * (T + 2*pad). */
int64_t tts_hifigan_output_length(const void* handle, int T, int pad);
/* Workspace the handle needs for (B, T, pad), and an explicit pre-allocation. */
int64_t tts_hifigan_workspace_bytes(const void* handle, int B, int T, int pad);
int tts_hifigan_reserve(void* handle, int B, int T, int pad);

/* wav[B][out][hop*(T+2*pad)] = G(replicate_pad(mel[B][C][T], pad)).  pad = 0 is
 * HifiganGenerator.forward, pad = inference_padding is .inference (hifigan_generator.py:281).
 * d_g ([B][cond_channels], may be NULL when cond_channels == 0) is the global conditioning
 * vector (the reference's g[B][cond][1], :250-251).
 * Streams: the call is ordered on hip_stream; internally it forks onto the handle's own lane /
 * branch streams and joins back before returning.  Those streams, their events and the handle's
 * workspace are per handle, so one handle must be driven from one caller stream at a time (a
 * second stream must wait for the first call's completion); use one handle per concurrent stream.
 * Non-finite mel values are outside the contract: the kernels build without NaN semantics, so a
 * NaN or inf input yields an unspecified waveform for that utterance (the other utterances of the
 * batch are unaffected: every statistic is per utterance). */
int tts_hifigan_forward(void* handle, const float* d_mel, int B, int C, int T, int pad,
                        const float* d_g, float* d_wav, void* hip_stream);

/* Same computation, with a hipEvent pair around every kernel launch.  Synchronises the
 * stream before returning.  records[i] describes launch i in issue order. */
typedef struct TtsLaunchRecord {
  char name[48];    /* kernel family, e.g. "mrf_conv_k11_c128" */
  double flops;     /* algorithmic FLOPs of this launch (2*MACs, no padding waste) */
  double bytes;     /* compulsory HBM bytes of this launch (inputs + weights + outputs) */
  float ms;         /* measured duration */
} TtsLaunchRecord;
int tts_hifigan_forward_profiled(void* handle, const float* d_mel, int B, int C, int T, int pad,
                                 const float* d_g, float* d_wav, void* hip_stream,
                                 TtsLaunchRecord* records, int max_records, int* n_records);

/* ------------------------------------------------------------------------------------ */
/* Glow-TTS decoder flow (reverse)                                                        */
/* ------------------------------------------------------------------------------------ */

/* Mirrors Decoder.__init__ (decoder.py:68-81). */
typedef struct TtsGlowDecoderCfg {
  int in_channels;         /* 80 (out_channels of GlowTTS) */
  int hidden_channels;     /* 192 (hidden_channels_dec) */
  int kernel_size;         /* 5 */
  int dilation_rate;       /* 1 */
  int num_flow_blocks;     /* 12 */
  int num_coupling_layers; /* 4 */
  int num_splits;          /* 4 */
  int num_squeeze;         /* 2 */
  int sigmoid_scale;       /* 0 */
  int c_in_channels;       /* 0 = unconditioned; > 0: speaker vector size, every WN gets a cond_layer
                              (wavenet.py:64-66, :98-107) */
  int math_mode;           /* TTS_MATH_FP32 (default), _X6, _F16X3 or TTS_MATH_BF16 */
} TtsGlowDecoderCfg;

/* Host weight order, per flow block b < num_flow_blocks (flows 3b, 3b+1, 3b+2):
 *   actnorm.logs [C2], actnorm.bias [C2]                          (C2 = in*num_squeeze)
 *   invconv.weight_inv [S][S]  (torch.inverse(weight), glow.py:139-141)
 *   invconv.weight [S][S]      (the forward direction, glow.py:126-130; since ABI 112)
 *   coupling.start.weight [H][C2/2] (weight-norm folded), coupling.start.bias [H]
 *   if c_in_channels: wn.cond_layer.weight [2*H*L][c_in] (weight-norm folded), bias [2*H*L]
 *   for l < L: wn.in_layers.l.weight [2H][H][k], wn.in_layers.l.bias [2H]
 *              wn.res_skip_layers.l.weight [l<L-1 ? 2H : H][H], bias
 *   coupling.end.weight [C2][H], coupling.end.bias [C2] */
int tts_glow_decoder_num_weights(const TtsGlowDecoderCfg* cfg);
int64_t tts_glow_decoder_weight_numel(const TtsGlowDecoderCfg* cfg, int idx);
int tts_glow_decoder_create(const TtsGlowDecoderCfg* cfg, const float* const* host_weights,
                            int device, void** handle);
int tts_glow_decoder_destroy(void* handle);
/* (y, logdet) = Decoder.forward(x, x_mask, g, reverse=reverse) (decoder.py:113-137): y[B][C][T'] with
 * T' = T rounded down to a multiple of num_squeeze (decoder.py:19); d_mask is [B][1][T] (0/1); d_g is
 * the speaker vector [B][c_in_channels] (the reference's g [B][c_in][1]), NULL when c_in_channels == 0.
 * reverse = 1: the inference direction (glow_tts.py:363), d_logdet unused (the reference returns None).
 * reverse = 0: the flows in order (GlowTTS.decoder_inference, glow_tts.py:333); d_logdet [B] fp32
 * receives logdet_tot (ActNorm + InvConvNear + coupling terms, summed per utterance in fp64 in a fixed
 * order), or is NULL to skip it.  Since ABI 112 (d_logdet added). */
int tts_glow_decoder_forward(void* handle, const float* d_x, const float* d_mask, const float* d_g, int B,
                             int C, int T, int reverse, float* d_y, float* d_logdet, void* hip_stream);
/* Same with a hipEvent pair around every launch (synchronises; see tts_hifigan_forward_profiled). */
int tts_glow_decoder_forward_profiled(void* handle, const float* d_x, const float* d_mask, const float* d_g,
                                      int B, int C, int T, int reverse, float* d_y, float* d_logdet,
                                      void* hip_stream, TtsLaunchRecord* records, int max_records,
                                      int* n_records);

/* ------------------------------------------------------------------------------------ */
/* Glow-TTS encoder (rel_pos_transformer) and the GlowTTS.inference glue                   */
/* ------------------------------------------------------------------------------------ */

/* Mirrors Encoder.__init__ (encoder.py:83-141) for encoder_type "rel_pos_transformer", with the
 * transformer's encoder_params flattened (transformer.py:345-357; GlowTTS passes
 * in = out = hidden = hidden_channels_enc). */
typedef struct TtsGlowEncoderCfg {
  int num_chars;            /* embedding rows */
  int out_channels;         /* 80 (mel channels) */
  int hidden_channels;      /* 192 (hidden_channels_enc) */
  int hidden_channels_dp;   /* 256 */
  int hidden_channels_ffn;  /* 768 (encoder_params) */
  int num_heads;            /* 2 */
  int num_layers;           /* 6 */
  int kernel_size;          /* 3: FFN conv kernel (encoder_params) */
  int rel_attn_window_size; /* 0 = None (Glow-TTS default); 4 in the VITS-style encoders */
  int mean_only;            /* 1 (GlowTTSConfig default): x_logs = zeros */
  int use_prenet;           /* 1: ResidualConv1dLayerNormBlock(k5, 3 layers) before the transformer */
  int c_in_channels;        /* 0 = unconditioned; > 0: speaker vector size, the duration predictor reads
                               cat(x, g.expand(T)) (encoder.py:166-168; GlowTTS c_in_channels) */
  int math_mode;            /* TTS_MATH_FP32 (default), TTS_MATH_FP32_X6 or TTS_MATH_BF16 */
  /* since ABI 113: the other encoder types of encoder.py:97-123 (0 = rel_pos_transformer) */
  int encoder_type;         /* TTS_ENC_REL_POS_TRANSFORMER / _GATED_CONV / _RESIDUAL_CONV_BN / _TIME_DEPTH_SEPARABLE */
  int num_conv_blocks;      /* residual_conv_bn: convs per residual block (2) */
  int num_res_blocks;       /* residual_conv_bn: residual blocks (13) = entries of dilations */
  int dilations[32];        /* residual_conv_bn: dilation of each residual block */
  int layer_norm_type;      /* rel_pos_transformer: 1 (LayerNorm, eps 1e-4; 0 = 1) or 2 (LayerNorm2, eps 1e-5) */
  int has_input_length;     /* rel_pos_transformer: 1 when input_length is set (transformer.py:148-150): */
  int input_length;         /*   scores with |i - j| > input_length are -1e4 (block-limited attention) */
} TtsGlowEncoderCfg;

#define TTS_ENC_REL_POS_TRANSFORMER 0
#define TTS_ENC_GATED_CONV 1          /* GatedConvBlock(H, kernel_size, dropout, num_layers), no prenet */
#define TTS_ENC_RESIDUAL_CONV_BN 2    /* ResidualConv1dBNBlock + postnet conv1x1 -> BatchNorm */
#define TTS_ENC_TIME_DEPTH_SEPARABLE 3 /* TimeDepthSeparableConvBlock (prenet as rel_pos) */

/* Host weight order (R = 2*rel_attn_window_size + 1, dk = hidden/num_heads, H = hidden, k =
 * kernel_size; a BatchNorm "BN(C)" is weight [C], bias [C], running_mean [C], running_var [C]):
 *   emb.weight [num_chars][H]
 *   if use_prenet (rel_pos_transformer, time_depth_separable):
 *                  for l < 3: prenet.conv_layers.l.weight [H][H][5], bias [H],
 *                             prenet.norm_layers.l.gamma [H], beta [H]
 *                  prenet.proj.weight [H][H][1], bias [H]
 *   gated_conv, for l < num_layers: encoder.conv_layers.l.weight [2H][H][k], bias [2H],
 *                                   encoder.norm_layers.l.gamma [2H], beta [2H]
 *   residual_conv_bn, for i < num_res_blocks, j < num_conv_blocks:
 *       encoder.res_blocks.i.conv_bn_blocks.j.conv1d.weight [H][H][k], bias [H], .norm BN(H)
 *     then postnet.0.weight [H][H][1], bias [H], postnet.1 BN(H)
 *   time_depth_separable, for l < num_layers: encoder.layers.l.time_conv.weight [2H][H][1], bias [2H],
 *       norm1 BN(2H), depth_conv.weight [H][1][k], bias [H], norm2 BN(H),
 *       time_conv2.weight [H][H][1], bias [H], norm3 BN(H)
 *   rel_pos_transformer, for l < num_layers (encoder.*):
 *       attn_layers.l.conv_q.weight [H][H][1], bias, conv_k.*, conv_v.*, conv_o.*
 *       if rel_attn_window_size: attn_layers.l.emb_rel_k [1][R][dk], emb_rel_v [1][R][dk]
 *       norm_layers_1.l.gamma [H], beta [H]
 *       ffn_layers.l.conv_1.weight [ffn][H][k], bias [ffn], conv_2.weight [H][ffn][k], bias [H]
 *       norm_layers_2.l.gamma [H], beta [H]
 *   proj_m.weight [out][H][1], bias [out];  if !mean_only: proj_s.weight, bias
 *   duration_predictor.conv_1.weight [dp][H + c_in_channels][3], bias, norm_1.gamma, beta,
 *                      conv_2.weight [dp][dp][3], bias, norm_2.gamma, beta,
 *                      proj.weight [1][dp][1], proj.bias [1] */
int tts_glow_encoder_num_weights(const TtsGlowEncoderCfg* cfg);
int64_t tts_glow_encoder_weight_numel(const TtsGlowEncoderCfg* cfg, int idx);
int tts_glow_encoder_create(const TtsGlowEncoderCfg* cfg, const float* const* host_weights, int device,
                            void** handle);
int tts_glow_encoder_destroy(void* handle);
/* (x_m, x_logs, logw, x_mask) = Encoder.forward(tokens, lengths, g): tokens [B][T] int64 (ids in
 * [0, num_chars); padded positions may hold any id), lengths [B] int64, d_g the speaker vector
 * [B][c_in_channels] (the reference's g [B][c_in][1]; NULL when c_in_channels == 0); outputs x_m,
 * x_logs [B][out][T], logw [B][1][T], x_mask [B][1][T].  x_logs may be NULL when mean_only.
 * T <= 3072. */
int tts_glow_encoder_forward(void* handle, const int64_t* d_tokens, const int64_t* d_lengths, const float* d_g,
                             int B, int T, float* d_x_m, float* d_x_logs, float* d_logw, float* d_x_mask,
                             void* hip_stream);
int tts_glow_encoder_forward_profiled(void* handle, const int64_t* d_tokens, const int64_t* d_lengths,
                                      const float* d_g, int B, int T, float* d_x_m, float* d_x_logs, float* d_logw,
                                      float* d_x_mask,
                                      void* hip_stream, TtsLaunchRecord* records, int max_records,
                                      int* n_records);

/* glow_tts.py:350-352 and :147: w_ceil[B][1][T_x] = max(ceil((exp(logw) - 1) * x_mask *
 * length_scale), 1); y_lengths[B] (int64) = max(sum(w_ceil), 1); o_attn_dur [B][1][T_x] =
 * log(1 + sum_j attn[i][j]) * x_mask (may be NULL).  The caller reads y_lengths back to size
 * T_y = max(y_lengths) (the reference's sequence_mask(y_lengths, None), glow_tts.py:353). */
int tts_glow_durations(const float* d_logw, const float* d_x_mask, int B, int T_x, float length_scale,
                       float* d_w_ceil, int64_t* d_y_lengths, float* d_o_attn_dur, void* hip_stream);
/* glow_tts.py:353-361: y_mask [B][1][T_y]; attn = generate_path(w_ceil, x_mask*y_mask)
 * (helpers.py:154-169); y_mean = attn^T o_mean, y_log_scale = attn^T o_log_scale (compute_outputs
 * :138-145); z = (y_mean + exp(y_log_scale) * noise * noise_scale) * y_mask.
 * o_log_scale NULL = zeros (mean_only); noise [B][C][T_y] (torch.randn_like drawn by the caller)
 * NULL = zeros.  y_mean, y_log_scale [B][C][T_y] and attn [B][T_x][T_y] may be NULL.
 * T_y must be >= max(y_lengths).  T_x <= 16384. */
int tts_glow_expand(const float* d_w_ceil, const float* d_x_mask, const int64_t* d_y_lengths,
                    const float* d_o_mean, const float* d_o_log_scale, const float* d_noise, float noise_scale,
                    int B, int C, int T_x, int T_y, float* d_z, float* d_y_mask, float* d_y_mean,
                    float* d_y_log_scale, float* d_attn, void* hip_stream);

/* The alignment log-likelihood of GlowTTS.forward / inference_with_MAS (glow_tts.py:218-228), with
 * s = exp(-2 o_log_scale):
 *   logp[b][x][y] = sum_c(-0.5 log(2 pi) - o_log_scale[c][x]) + sum_c s[c][x] (-0.5 z[c][y]^2)
 *                 + sum_c (o_mean[c][x] s[c][x]) z[c][y] + sum_c -0.5 o_mean[c][x]^2 s[c][x]
 * o_mean, o_log_scale [B][C][T_en] (o_log_scale NULL = zeros: mean_only), z [B][C][T_de], logp
 * [B][T_en][T_de].  One fp32 arithmetic (v_mfma_f32_32x32x2_f32, depth 2C); any C, T_en, T_de >= 1
 * whose per-item planes stay under 2 GiB. */
int tts_glow_mas_logp(const float* d_o_mean, const float* d_o_log_scale, const float* d_z, int B, int C, int T_en,
                      int T_de, float* d_logp, void* hip_stream);
/* Monotonic Alignment Search (maximum_path): per item the monotonic path through value [T_en][T_de]
 * (y fastest) from (0, 0) to (t_x - 1, t_y - 1) with the largest sum, found with the reference's
 * loops (each cell one fp32 max and one fp32 add; ties stay on the token), so the path equals a CPU
 * evaluation of them exactly.  d_mask (NULL = none) is multiplied into every value on load.  t_x,
 * t_y [B] int64 on the device.  Outputs, each may be NULL: path [B][T_en][T_de] (0 / 1), durations
 * [B][T_en] (row sums of the path), log_dur = logf(1 + durations).  Items with t_x < 1, t_y < t_x,
 * t_x > T_en or t_y > T_de (the reference reads out of bounds there) get an all-zero path and
 * durations.  d_workspace: tts_maximum_path_workspace_bytes(B, T_en, T_de) bytes of device memory
 * (never 0; -1 for a shape outside the limits).
 * Limits: T_en <= 1024, T_en * T_de * 4 bytes < 2 GiB, B <= 65535 (TTS_ERR_UNSUPPORTED beyond). */
int64_t tts_maximum_path_workspace_bytes(int B, int T_en, int T_de);
int tts_maximum_path(const float* d_value, const float* d_mask, const int64_t* d_t_x, const int64_t* d_t_y, int B,
                     int T_en, int T_de, void* d_workspace, float* d_path, float* d_durations, float* d_log_dur,
                     void* hip_stream);

/* ------------------------------------------------------------------------------------ */
/* TTS -> vocoder hand-off and the int16 wav writer                                       */
/* ------------------------------------------------------------------------------------ */

/* AudioProcessor normalisation fields (processor.py:259-336; BaseAudioConfig defaults
 * shared_configs.py:126-154), as the Python values (they are rounded to fp32 where numpy
 * would).  d_mel_mean / d_mel_scale: device fp64 [C] mel_scaler statistics (mean-var
 * normalisation, processor.py:275-277 / :316-318), or NULL for range normalisation. */
typedef struct TtsAudioNormCfg {
  int signal_norm;     /* 0: identity */
  int symmetric_norm;
  int clip_norm;
  double max_norm;
  double min_level_db;
  double ref_level_db;
  const double* d_mel_mean;
  const double* d_mel_scale;
} TtsAudioNormCfg;

/* Synthesizer hand-off (synthesizer.py:412-428), batched: out[B][C][T_out] =
 * interpolate(vocoder_ap.normalize(tts_ap.denormalize(in))).  in: model_outputs [B][T][C]
 * (time_major = 1) or [B][C][T].  T_out == T: no resampling; otherwise the time axis is resampled
 * like interpolate_vocoder_input (vocoder/utils/generic_utils.py:11-29: bilinear,
 * align_corners=False, recompute_scale_factor=True; pass T_out = floor(T * sr_voc / sr_tts) and
 * src_scale = 0, which maps with T / T_out).  src_scale > 0 maps output j to source
 * src_scale * (j + 0.5) - 0.5 instead: F.interpolate(mode="linear", scale_factor=s) without
 * recompute_scale_factor passes src_scale = 1/s (the XTTS latent upsampling,
 * xtts/hifigan_decoder.py:688-698).  denorm / norm may be NULL (identity). */
int tts_mel_handoff(const float* d_in, int B, int T, int C, int time_major, const TtsAudioNormCfg* denorm,
                    const TtsAudioNormCfg* norm, int T_out, float src_scale, float* d_out, void* hip_stream);
/* save_wav scaling (numpy_transforms.py:436-438): out = int16(wav * (32767 / max(0.01, max|wav|)))
 * per utterance.  wav [B][n] fp32; d_lengths [B] (int64, NULL = n) limits each utterance (samples
 * beyond it are written as 0); d_scratch: B x uint32 of device memory. */
int tts_wav_to_int16(const float* d_wav, int B, int64_t n, const int64_t* d_lengths, unsigned* d_scratch,
                     int16_t* d_out, void* hip_stream);

/* ------------------------------------------------------------------------------------ */
/* VITS flow: ResidualCouplingBlocks, reverse (TTS/tts/layers/vits/networks.py:169-232)     */
/* ------------------------------------------------------------------------------------ */

/* Mirrors ResidualCouplingBlocks.__init__ (networks.py:169-202; VITS builds it at
 * vits.py:675-682 with mean-only blocks). */
typedef struct TtsVitsFlowCfg {
  int channels;        /* 192 (hidden_channels) */
  int hidden_channels; /* 192 */
  int kernel_size;     /* 5 (kernel_size_flow) */
  int dilation_rate;   /* 1 (dilation_rate_flow) */
  int num_layers;      /* 4 (num_layers_flow) */
  int num_flows;       /* 4 */
  int cond_channels;   /* speaker embedding size, 0 = none (embedded_speaker_dim) */
  int math_mode;       /* TTS_MATH_FP32 (default), _X6, _F16X3 or TTS_MATH_BF16 */
} TtsVitsFlowCfg;

/* Host weight order, per flow f < num_flows (weight norm folded: w = g * v / ||v||):
 *   pre.weight [H][C/2], pre.bias [H]
 *   for l < L: enc.in_layers.l.weight [2H][H][k], enc.in_layers.l.bias [2H]
 *   for l < L: enc.res_skip_layers.l.weight [l<L-1 ? 2H : H][H], bias
 *   if cond_channels: enc.cond_layer.weight [2*H*L][cond_channels], enc.cond_layer.bias [2*H*L]
 *   post.weight [C/2][H], post.bias [C/2] */
int tts_vits_flow_num_weights(const TtsVitsFlowCfg* cfg);
int64_t tts_vits_flow_weight_numel(const TtsVitsFlowCfg* cfg, int index);
int tts_vits_flow_create(const TtsVitsFlowCfg* cfg, const float* const* host_weights, int device,
                         void** handle);
int tts_vits_flow_destroy(void* handle);
/* y[B][C][T] = ResidualCouplingBlocks(x, mask, g, reverse=reverse) (networks.py:217-232).  x, y:
 * [B][C][T] fp32 (y may equal x: in place), mask: [B][T], g: [B][cond_channels] (NULL when
 * cond_channels == 0).  reverse = 1: the inference direction (vits.py:1155); reverse = 0: the
 * posterior side of voice conversion, z_p = flow(z, y_mask, g) (vits.py:1226; since ABI 112). */
int tts_vits_flow_forward(void* handle, const float* d_x, const float* d_mask, const float* d_g, int B,
                          int C, int T, int reverse, float* d_y, void* hip_stream);
int tts_vits_flow_forward_profiled(void* handle, const float* d_x, const float* d_mask, const float* d_g,
                                   int B, int C, int T, int reverse, float* d_y, void* hip_stream,
                                   TtsLaunchRecord* records, int max_records, int* n_records);

/* ------------------------------------------------------------------------------------ */
/* VITS posterior encoder (TTS/tts/layers/vits/networks.py:235-288), since ABI 112        */
/* ------------------------------------------------------------------------------------ */

/* Mirrors PosteriorEncoder.__init__ (networks.py:236-273); VITS builds it from the linear
 * spectrogram (vits.py:594-602: in = fft_size/2 + 1 = 513, out = hidden = 192, k5, d1, 16 layers). */
typedef struct TtsVitsPosteriorCfg {
  int in_channels;     /* 513 */
  int out_channels;    /* 192 */
  int hidden_channels; /* 192 */
  int kernel_size;     /* 5 */
  int dilation_rate;   /* 1 */
  int num_layers;      /* 16 */
  int cond_channels;   /* speaker embedding size, 0 = none */
  int math_mode;       /* TTS_MATH_* (f16x3 / fp32x6 / fp32 / bf16) */
} TtsVitsPosteriorCfg;

/* Host weight order (weight norm folded):
 *   pre.weight [H][in], pre.bias [H]
 *   for l < L: enc.in_layers.l.weight [2H][H][k], bias [2H]
 *   for l < L: enc.res_skip_layers.l.weight [l<L-1 ? 2H : H][H], bias
 *   if cond_channels: enc.cond_layer.weight [2*H*L][cond_channels], bias [2*H*L]
 *   proj.weight [2*out][H], proj.bias [2*out] */
int tts_vits_posterior_num_weights(const TtsVitsPosteriorCfg* cfg);
int64_t tts_vits_posterior_weight_numel(const TtsVitsPosteriorCfg* cfg, int index);
int tts_vits_posterior_create(const TtsVitsPosteriorCfg* cfg, const float* const* host_weights, int device,
                              void** handle);
int tts_vits_posterior_destroy(void* handle);
/* (z, m, logs) = PosteriorEncoder.forward(x, x_lengths, g)[:3] (networks.py:275-288): x [B][in][T],
 * mask [B][T] (sequence_mask(x_lengths)), g [B][cond_channels] or NULL, eps [B][out][T] the standard
 * normal sample the reference draws with torch.randn_like (NULL: zero noise, z = m); z, m, logs
 * [B][out][T] fp32 (m or logs may be NULL when not wanted). */
int tts_vits_posterior_forward(void* handle, const float* d_x, const float* d_mask, const float* d_g,
                               const float* d_eps, int B, int C, int T, float* d_z, float* d_m, float* d_logs,
                               void* hip_stream);
int tts_vits_posterior_forward_profiled(void* handle, const float* d_x, const float* d_mask, const float* d_g,
                                        const float* d_eps, int B, int C, int T, float* d_z, float* d_m,
                                        float* d_logs, void* hip_stream, TtsLaunchRecord* records,
                                        int max_records, int* n_records);

/* ------------------------------------------------------------------------------------ */
/* Linear spectrogram of a waveform: wav_to_spec (TTS/tts/models/vits.py), the posterior   */
/* encoder's input in voice conversion                                                    */
/* ------------------------------------------------------------------------------------ */

/* spec = sqrt(|STFT(y)|^2 + 1e-6) as VITS computes it (center=False): with p = (n_fft - hop) / 2
 * the wav y[B][N] is reflect-padded by p samples on both sides (the edge sample is not repeated:
 * y[-i] = y[i], y[N-1+i] = y[N-1-i]; needs N > p), framed every hop_length samples
 * (T = 1 + (N + 2p - n_fft) / hop_length frames, trailing samples that do not fill a frame are
 * dropped), multiplied by the window (win_length values, zero-padded to n_fft, centred: left pad
 * (n_fft - win_length) / 2) and transformed: X[k][t] = sum_n window[n] ypad[t hop + n]
 * e^(-2 pi i k n / n_fft), k = 0 .. n_fft/2.
 *
 * One launch (two with the input's max-abs pass in TTS_MATH_FP32_F16X3): a GEMM of the windowed DFT
 * matrix (packed once per plan) with the frames, on the matrix cores, magnitude fused.
 * Supported: n_fft a multiple of 32 in [64, 2048]; 1 <= win_length <= n_fft; hop_length a multiple
 * of 8 in [8, n_fft]; math_mode TTS_MATH_FP32_X6, _F16X3 or TTS_MATH_BF16 (TTS_MATH_FP32 has no
 * kernel here: TTS_ERR_UNSUPPORTED); N > p and N + 2p >= n_fft; N * 4 and
 * (n_fft/2 + 1) * T * 4 below 2 GiB.  Outside: TTS_ERR_UNSUPPORTED / TTS_ERR_INVALID. */
typedef struct TtsStftCfg {
  int n_fft;      /* 1024 (VITS fft_size) */
  int hop_length; /* 256 */
  int win_length; /* 1024 */
  int math_mode;  /* TTS_MATH_FP32_X6, TTS_MATH_FP32_F16X3 or TTS_MATH_BF16 */
} TtsStftCfg;

/* h_window: win_length fp32 values on the host (torch.hann_window(win_length) for VITS); the packed
 * DFT matrix lives in the handle. */
int tts_stft_create(const TtsStftCfg* cfg, const float* h_window, int device, void** handle);
int tts_stft_destroy(void* handle);
/* Frames T of an N-sample wav (host only); -TTS_ERR_* on a bad configuration or N. */
int tts_stft_num_frames(const TtsStftCfg* cfg, int64_t N);
/* d_spec[B][n_fft/2 + 1][T] fp32 (T = tts_stft_num_frames(cfg, N)) from d_wav: B rows of N fp32
 * samples, wav_bstride floats apart (0 = N). */
int tts_stft_forward(void* handle, const float* d_wav, int B, int64_t N, int64_t wav_bstride, float* d_spec,
                     void* hip_stream);
int tts_stft_forward_profiled(void* handle, const float* d_wav, int B, int64_t N, int64_t wav_bstride,
                              float* d_spec, void* hip_stream, TtsLaunchRecord* records, int max_records,
                              int* n_records);

/* ------------------------------------------------------------------------------------ */
/* VITS text side of Vits.inference (TTS/tts/models/vits.py:1121-1155), since ABI 114       */
/* ------------------------------------------------------------------------------------ */

/* Mirrors TextEncoder.__init__ (TTS/tts/layers/vits/networks.py:29-81; VITS builds it at
 * vits.py:653-663 with out = hidden = hidden_channels).  The transformer is the Glow encoder's
 * RelativePositionTransformer with layer_norm_type "2" and rel_attn_window_size 4. */
typedef struct TtsVitsTextEncoderCfg {
  int n_vocab;             /* num_chars */
  int out_channels;        /* 192 */
  int hidden_channels;     /* 192 */
  int hidden_channels_ffn; /* 768 */
  int num_heads;           /* 2 */
  int num_layers;          /* 6 */
  int kernel_size;         /* 3 (FFN) */
  int language_emb_dim;    /* 0, or L > 0 (YourTTS): the transformer runs at H + L channels (since ABI 115) */
  int math_mode;           /* TTS_MATH_FP32, _X6 or TTS_MATH_BF16 */
} TtsVitsTextEncoderCfg;

/* Host weight order, with E = H + language_emb_dim (networks.py:63-64): emb.weight [n_vocab][H]; per
 * layer l: encoder.attn_layers.l.conv_q/k/v/o (weight [E][E][1], bias [E]), emb_rel_k [1][9][dk],
 * emb_rel_v [1][9][dk] (dk = E / num_heads), encoder.norm_layers_1.l gamma [E], beta [E],
 * encoder.ffn_layers.l.conv_1 (weight [ffn][E][k], bias), conv_2 (weight [E][ffn][k], bias),
 * encoder.norm_layers_2.l gamma, beta; proj.weight [2 out][E][1], proj.bias [2 out]. */
int tts_vits_text_encoder_num_weights(const TtsVitsTextEncoderCfg* cfg);
int64_t tts_vits_text_encoder_weight_numel(const TtsVitsTextEncoderCfg* cfg, int index);
int tts_vits_text_encoder_create(const TtsVitsTextEncoderCfg* cfg, const float* const* host_weights, int device,
                                 void** handle);
int tts_vits_text_encoder_destroy(void* handle);
/* (x, m, logs, x_mask) = TextEncoder.forward(tokens, lengths, lang_emb) (networks.py:83-100): tokens
 * [B][T] int64, lengths [B] int64, lang_emb [B][language_emb_dim] (NULL when language_emb_dim = 0;
 * the reference's [B][L][1]); x [B][E][T], m and logs [B][out][T], x_mask [B][1][T].  T <= 3072. */
int tts_vits_text_encoder_forward(void* handle, const int64_t* d_tokens, const int64_t* d_lengths,
                                  const float* d_lang_emb, int B, int T, float* d_x, float* d_m, float* d_logs,
                                  float* d_x_mask, void* hip_stream);
int tts_vits_text_encoder_forward_profiled(void* handle, const int64_t* d_tokens, const int64_t* d_lengths,
                                           const float* d_lang_emb, int B, int T, float* d_x, float* d_m,
                                           float* d_logs, float* d_x_mask, void* hip_stream,
                                           TtsLaunchRecord* records, int max_records, int* n_records);

/* Mirrors StochasticDurationPredictor.__init__ (TTS/tts/layers/vits/stochastic_duration_predictor.py:
 * 185-227; VITS: in = hidden_channels, hidden 192, kernel 3, 4 flows, cond = embedded_speaker_dim when
 * condition_dp_on_speaker, vits.py:684-692).  ConvFlows use 10 bins, tail bound 5 (:96-104). */
typedef struct TtsVitsSdpCfg {
  int in_channels;      /* 192 (+ language_emb_dim: the text encoder's x width, :191-192) */
  int hidden_channels;  /* 192 (<= 512) */
  int kernel_size;      /* 3 */
  int num_flows;        /* 4 */
  int cond_channels;    /* 0 = no cond layer */
  int language_emb_dim; /* 0 = no cond_lang layer (since ABI 115) */
  int math_mode;        /* TTS_MATH_FP32, _X6 or TTS_MATH_BF16 (its 1x1 convs) */
} TtsVitsSdpCfg;

/* Host weight order (the inference-side tensors in state_dict order; post_* are training-only):
 *   pre.weight [H][in][1], pre.bias [H]
 *   DDS(convs): convs_sep.i.weight [H][1][k], bias [H] (i < 3); convs_1x1.i.weight [H][H][1], bias [H];
 *               norms_1.i.gamma [H], beta [H]; norms_2.i.gamma [H], beta [H]
 *   proj.weight [H][H][1], proj.bias [H]
 *   flows.0.translation [2][1], flows.0.log_scale [2][1]
 *   for f = 1 .. num_flows: flows.f.pre.weight [H][1][1], bias [H]; DDS(flows.f.convs);
 *                           flows.f.proj.weight [29][H][1], bias [29]
 *   if cond_channels: cond.weight [H][cond][1], cond.bias [H]
 *   if language_emb_dim: cond_lang.weight [H][L][1], cond_lang.bias [H] */
int tts_vits_sdp_num_weights(const TtsVitsSdpCfg* cfg);
int64_t tts_vits_sdp_weight_numel(const TtsVitsSdpCfg* cfg, int index);
int tts_vits_sdp_create(const TtsVitsSdpCfg* cfg, const float* const* host_weights, int device, void** handle);
int tts_vits_sdp_destroy(void* handle);
/* logw [B][1][T] = StochasticDurationPredictor.forward(x, x_mask, g=g, lang_emb=lang, reverse=True,
 * noise_scale) (:242-282): x [B][in][T], x_mask [B][1][T], g [B][cond_channels] or NULL, lang
 * [B][language_emb_dim] or NULL (x = pre(x) + cond(g) + cond_lang(lang), :249-254), noise [B][2][T]
 * the standard normal draw of :277 (torch.randn(B, 2, T); NULL = zeros). */
int tts_vits_sdp_reverse(void* handle, const float* d_x, const float* d_x_mask, const float* d_g,
                         const float* d_lang_emb, const float* d_noise, float noise_scale, int B, int T,
                         float* d_logw, void* hip_stream);
int tts_vits_sdp_reverse_profiled(void* handle, const float* d_x, const float* d_x_mask, const float* d_g,
                                  const float* d_lang_emb, const float* d_noise, float noise_scale, int B, int T,
                                  float* d_logw, void* hip_stream, TtsLaunchRecord* records, int max_records,
                                  int* n_records);

/* Mirrors the deterministic DurationPredictor VITS builds with use_sdp=False (vits.py:694-702:
 * TTS/tts/layers/glow_tts/duration_predictor.py:6-44 with in = hidden_channels, filter 256, kernel 3,
 * cond = embedded_speaker_dim, language_emb_dim), since ABI 115. */
typedef struct TtsVitsDpCfg {
  int in_channels;      /* hidden_channels (192); the module adds language_emb_dim itself (:28-29) */
  int hidden_channels;  /* filter channels, 256 */
  int kernel_size;      /* 3 (odd, <= 11) */
  int cond_channels;    /* 0 = no cond layer */
  int language_emb_dim; /* 0 = no cond_lang layer */
  int math_mode;        /* TTS_MATH_FP32, _X6 or TTS_MATH_BF16 */
} TtsVitsDpCfg;

/* Host weight order (state_dict order), I = in_channels + language_emb_dim, F = hidden_channels:
 *   conv_1.weight [F][I][k], conv_1.bias [F]; norm_1.gamma [F], norm_1.beta [F];
 *   conv_2.weight [F][F][k], conv_2.bias [F]; norm_2.gamma [F], norm_2.beta [F];
 *   proj.weight [1][F][1], proj.bias [1];
 *   if cond_channels: cond.weight [I][cond][1], cond.bias [I];
 *   if language_emb_dim: cond_lang.weight [I][L][1], cond_lang.bias [I] */
int tts_vits_dp_num_weights(const TtsVitsDpCfg* cfg);
int64_t tts_vits_dp_weight_numel(const TtsVitsDpCfg* cfg, int index);
int tts_vits_dp_create(const TtsVitsDpCfg* cfg, const float* const* host_weights, int device, void** handle);
int tts_vits_dp_destroy(void* handle);
/* logw [B][1][T] = DurationPredictor.forward(x, x_mask, g, lang_emb) (duration_predictor.py:49-68):
 * x [B][I][T], x_mask [B][1][T], g [B][cond_channels] or NULL, lang [B][language_emb_dim] or NULL. */
int tts_vits_dp_forward(void* handle, const float* d_x, const float* d_x_mask, const float* d_g,
                        const float* d_lang_emb, int B, int T, float* d_logw, void* hip_stream);
int tts_vits_dp_forward_profiled(void* handle, const float* d_x, const float* d_x_mask, const float* d_g,
                                 const float* d_lang_emb, int B, int T, float* d_logw, void* hip_stream,
                                 TtsLaunchRecord* records, int max_records, int* n_records);

/* vits.py:1145-1148: w_ceil [B][1][T_x] = ceil(exp(logw) * x_mask * length_scale); y_lengths [B]
 * (int64) = max(sum(w_ceil), 1).  The caller reads y_lengths back for T_y = max(y_lengths). */
int tts_vits_durations(const float* d_logw, const float* d_x_mask, int B, int T_x, float length_scale,
                       float* d_w_ceil, int64_t* d_y_lengths, void* hip_stream);
/* vits.py:1147-1154: y_mask [B][1][T_y]; attn = generate_path(w_ceil, x_mask * y_mask) [B][T_x][T_y]
 * (may be NULL); m_p' = attn^T m_p, logs_p' = attn^T logs_p ([B][C][T_y], may be NULL);
 * z_p = m_p' + noise * exp(logs_p') * noise_scale (not masked; noise [B][C][T_y] NULL = zeros).
 * T_y >= max(y_lengths), T_x <= 16384. */
int tts_vits_expand(const float* d_w_ceil, const float* d_x_mask, const int64_t* d_y_lengths, const float* d_m_p,
                    const float* d_logs_p, const float* d_noise, float noise_scale, int B, int C, int T_x, int T_y,
                    float* d_z_p, float* d_y_mask, float* d_m_p_out, float* d_logs_p_out, float* d_attn,
                    void* hip_stream);

/* The rest of Vits.inference's glue on the device (since ABI 115).
 * Given durations (vits.py:1141-1146): w = durations.unsqueeze(0); w_ceil [B][1][T_x] = ceil(w) (no
 * mask, no length_scale), y_lengths [B] = max(sum(w_ceil), 1); durations [T_x] shared by every
 * utterance (dur_bstride 0) or [B][T_x] (dur_bstride T_x). */
int tts_vits_durations_given(const float* d_durations, int64_t dur_bstride, int B, int T_x, float* d_w_ceil,
                             int64_t* d_y_lengths, void* hip_stream);
/* (z * y_mask)[:, :, :T_out] (vits.py:1161): z [B][C][T] (batch stride C * T), y_mask [B][1][T],
 * out [B][C][T_out], 1 <= T_out <= T. */
int tts_vits_mask_slice(const float* d_z, const float* d_y_mask, int B, int C, int T, int T_out, float* d_out,
                        void* hip_stream);
/* upsampling_z (vits.py:944-959, encoder_sample_rate with interpolate_z): z2 [B][C][T2] =
 * F.interpolate(z [B][C][T], scale_factor=[factor], mode="linear"), T2 = floor(T * factor);
 * y_mask2 [B][1][T2] = sequence_mask(y_lengths * factor) (may be NULL).  The reference's product
 * z2 * y_mask2 needs ceil(max(y_lengths) * factor) == T2; the caller checks it. */
int tts_vits_upsample_z(const float* d_z, const int64_t* d_y_lengths, int B, int C, int T, double factor, int T2,
                        float* d_z2, float* d_y_mask2, void* hip_stream);
/* out [B][dim] = table[ids[b * id_stride]] (nn.Embedding rows: emb_g(sid), emb_l(lid)); ids are
 * clamped to [0, num) (the reference raises IndexError; a device kernel cannot). */
int tts_embedding_rows(const float* d_table, int num, int dim, const int64_t* d_ids, int64_t id_stride, int B,
                       float* d_out, void* hip_stream);
/* out [B][C] = d / max(||d||_2, 1e-12) per row (F.normalize(d_vectors), vits.py:884-886). */
int tts_l2_normalize_rows(const float* d_in, int B, int C, float* d_out, void* hip_stream);

/* ------------------------------------------------------------------------------------ */
/* Single-op entry points (test / tuning surface).  These pack the host weights into a     */
/* temporary device buffer on every call and synchronise; they are not the hot path.        */
/* ------------------------------------------------------------------------------------ */

/* y = epilogue(conv1d(act_in(x_padded), w) + b), "same" conv: pad = dil*(K-1)/2.
 * x_padded[t] = x[clamp(t - rep_pad, 0, Tin-1)] for t in [0, Tin + 2*rep_pad).
 * act_in / act_out = leaky_relu with the given slope (1.0 = identity).
 * Epilogue: v = act_out(acc + b) + (res ? res : 0);
 *   zmode 0: y = v;  1: z = v;  2: z = z + v;  3: z = (z + v) / zdiv. */
typedef struct TtsConv1dDesc {
  int B, Cin, Cout, Tin, K, dil, rep_pad;
  float in_slope, out_slope;
  int zmode;
  float zdiv;
  int math_mode; /* TTS_MATH_FP32 / TTS_MATH_FP32_X6 / TTS_MATH_FP32_F16X3 */
} TtsConv1dDesc;
int tts_op_conv1d(const TtsConv1dDesc* d, const float* d_x, const float* h_w, const float* h_b,
                  const float* d_res, float* d_y, float* d_z, void* hip_stream);

/* Tuning: same computation with an explicit tile configuration (tile < 0: automatic), launched
 * `reps` times; *ms receives the mean kernel time (hipEvents on hip_stream). */
int tts_op_conv1d_bench(const TtsConv1dDesc* d, const float* d_x, const float* h_w, const float* h_b,
                        const float* d_res, float* d_y, float* d_z, int tile, int reps, float* ms,
                        void* hip_stream);
/* The same with a per-item channel vector d_cvec [B][Cout] added to the bias before act_out (the
 * conditioning term the executors fold into a conv's epilogue), one launch of tile configuration
 * `tile` (tile < 0: automatic). */
int tts_op_conv1d_cvec(const TtsConv1dDesc* d, const float* d_x, const float* h_w, const float* h_b,
                       const float* d_cvec, const float* d_res, float* d_y, float* d_z, int tile,
                       void* hip_stream);
/* Number of conv1d tile configurations compiled into the library for a math mode. */
int tts_op_conv1d_num_tiles(int math_mode);

/* y = conv_transpose1d(act_in(x), w[Cin][Cout][K], b, stride, padding=(K-stride)/2);
 * requires K == 2*stride (every HiFiGAN config) with stride 2, 4 or 8; math_mode TTS_MATH_*
 * (the split modes run the polyphase K=2 conv form of the executor). */
int tts_op_conv_transpose1d(const float* d_x, int B, int Cin, int Tin, const float* h_w,
                            const float* h_b, int Cout, int K, int stride, float in_slope,
                            int math_mode, float* d_y, void* hip_stream);

/* y[B][1][T] = tanh(conv1d(leaky_relu(z, in_slope), w[1][Cin][7], b, pad 3)). */
int tts_op_conv_post(const float* d_z, int B, int Cin, int T, const float* h_w, const float* h_b,
                     float in_slope, float* d_y, void* hip_stream);

/* ------------------------------------------------------------------------------------ */
/* MelGAN-family generators: MelGAN, full-band MelGAN, multi-band MelGAN (+ PQMF)          */
/* ------------------------------------------------------------------------------------ */

/* Mirrors MelganGenerator.__init__ (TTS/vocoder/models/melgan_generator.py): reflection pad +
 * conv proj_kernel to base_channels; per upsampling i: leaky_relu(0.2), ConvTranspose1d(base >> i,
 * base >> (i+1), 2u, stride u), ResidualStack(num_res_blocks, res_kernel, dilations res_kernel^j);
 * leaky_relu(0.2), reflection pad, conv proj_kernel to out_channels, tanh.  pqmf_bands > 0
 * (= out_channels): the multi-band generator's PQMF synthesis (layers/pqmf.py) for synth = 1.
 * Implemented: upsample_factors 2, 4 or 8; proj_kernel 3, 5, 7 or 11; res_kernel 3;
 * num_res_blocks <= 4; base_channels <= 512; out_channels <= 4; pqmf_taps even, <= 126;
 * math_mode TTS_MATH_FP32_X6 or TTS_MATH_BF16 (TTS_MATH_FP32 and TTS_MATH_FP32_F16X3 run the
 * fp32x6 kernels: both are held to the fp32 parity gates).  Outside: TTS_ERR_UNSUPPORTED /
 * TTS_ERR_INVALID. */
typedef struct TtsMelganCfg {
  int in_channels;
  int out_channels;
  int proj_kernel;
  int base_channels;
  int num_ups;
  int upsample_factors[TTS_MAX_UPSAMPLES];
  int res_kernel;
  int num_res_blocks;
  int pqmf_bands; /* 0 = none */
  int pqmf_taps;
  int math_mode;
} TtsMelganCfg;

/* Host weights: the convs in state_dict order, folded (remove_weight_norm), weight then bias each:
 *   layers.1.weight [base][in][pk], layers.1.bias
 *   per upsampling i (C = base >> (i+1)): layers.(3+3i).weight [2C][C][2u], .bias [C]; then its stack:
 *     blocks.j.2.weight [C][C][rk], .bias, blocks.j.4.weight [C][C][1], .bias for j < num_res_blocks,
 *     then shortcuts.j.weight [C][C][1], .bias for j < num_res_blocks
 *   layers.(4+3n).weight [out][base >> n][pk], .bias
 *   pqmf_layer.G [1][bands][taps+1]  (only if pqmf_bands > 0) */
int tts_melgan_num_weights(const TtsMelganCfg* cfg);
int64_t tts_melgan_weight_numel(const TtsMelganCfg* cfg, int idx);
int tts_melgan_create(const TtsMelganCfg* cfg, const float* const* host_weights, int device, void** handle);
int tts_melgan_destroy(void* handle);
/* Samples per batch item and output channel: hop (T + 2 pad), times pqmf_bands when synth.
 * -TTS_ERR_INVALID when a reflection pad would be >= the plane it pads (as torch refuses it),
 * -TTS_ERR_UNSUPPORTED beyond the 32-bit plane range; tts_last_error() names the pad. */
int64_t tts_melgan_output_length(const void* handle, int T, int pad, int synth);
int64_t tts_melgan_workspace_bytes(const void* handle, int B, int T, int pad);
/* out = layers(replicate_pad(mel[B][C][T], pad)): [B][out_channels][hop (T + 2 pad)] (synth = 0,
 * MelganGenerator.forward / the sub-bands) or [B][1][bands hop (T + 2 pad)] (synth = 1: the PQMF
 * synthesis fused into the last launch; needs pqmf_bands > 0).  pad = 2 is .inference. */
int tts_melgan_forward(void* handle, const float* d_mel, int B, int C, int T, int pad, int synth, float* d_out,
                       void* hip_stream);
int tts_melgan_forward_profiled(void* handle, const float* d_mel, int B, int C, int T, int pad, int synth,
                                float* d_out, void* hip_stream, TtsLaunchRecord* records, int max_records,
                                int* n_records);

/* One residual block of a MelGAN ResidualStack (layers/melgan.py), kernel 3:
 *   d_out = ws x + bs + w2 lrelu(w1 (*)_dilation reflpad(lrelu(x, 0.2)) + b1, 0.2) + b2
 * x, out [B][C][L] on the device (not aliased); w1 [C][C][3], w2 / ws [C][C][1] and the biases on
 * the host.  math_mode as TtsMelganCfg.  L > dilation (TTS_ERR_INVALID otherwise). */
int tts_op_melgan_block(const float* d_x, int B, int C, int L, int dilation, const float* h_w1, const float* h_b1,
                        const float* h_w2, const float* h_b2, const float* h_ws, const float* h_bs, int math_mode,
                        float* d_out, void* hip_stream);
/* Output columns one workgroup of the block kernel computes. */
int tts_op_melgan_block_tile(void);
/* d_out[B][1][bands L] = PQMF.synthesis(d_x[B][bands][L]) with d_G [bands][taps+1] on the device
 * (polyphase form: bands * sum over the taps j with (n + j - taps/2) % bands == 0, zeros outside). */
int tts_pqmf_synthesis(const float* d_x, int B, int bands, int L, const float* d_G, int taps, float* d_out,
                       void* hip_stream);

/* ---- Multi-head self-attention of nn.MultiheadAttention (the FFTransformer layers of ForwardTTS /
 * FastPitch; TTS/tts/layers/generic/transformer.py), online softmax on the matrix cores ----
 *   d_out[b][h dk + d][i] = sum_j softmax_j((q_i dk^-0.5) . k_j) v_j[d],  dk = E / heads
 * d_qkv [B][3E][T] fp32, rows q | k | v (the in_proj output), head h at channels h dk ...; the dk^-0.5
 * query scale is applied by the op.  d_key_lengths: NULL (every key j < T counts) or [B] int64 on the
 * device, values in [1, T]: keys j >= d_key_lengths[b] get probability exactly 0 (the key padding
 * mask); every query i < T is computed, padded ones included.  A length outside [1, T] is clamped to
 * [0, T]; an item of length 0 has no key to attend to and its d_out is all zeros (an invalid item
 * gives zeros, not the NaN of a softmax over nothing).  d_out [B][E][T] fp32, not aliased.
 * Head sizes dk: 32, 64, 128, 192, 256 or 384, with E <= 512 (TTS_ERR_UNSUPPORTED otherwise); any T
 * with 3 E T 4 bytes below 2 GiB.  math_mode TTS_MATH_FP32_X6 or TTS_MATH_BF16 (TTS_MATH_FP32 and
 * TTS_MATH_FP32_F16X3 run the fp32x6 kernel: both are held to the fp32 parity gates).  Results do
 * not depend on B.  Stream-ordered; does not synchronise. */
int tts_op_mha(const float* d_qkv, const int64_t* d_key_lengths, int B, int E, int heads, int T, int math_mode,
               float* d_out, void* hip_stream);
/* Queries one workgroup of the attention kernel computes. */
int tts_op_mha_tile(void);

/* ---- ForwardTTS (FastPitch / FastSpeech; TTS/tts/models/forward_tts.py, inference) with the
 * "fftransformer" encoder and decoder ----
 * Mirrors ForwardTTSArgs; encoder_* / decoder_* are encoder_params / decoder_params
 * (hidden_channels_ffn, num_heads, num_layers).  The FFN convs have kernel size 3 (FFTransformer's
 * kernel_size_fft default; FFTransformerBlock passes no other).  The text side (encoder, duration
 * and pitch predictors) always runs TTS_MATH_FP32_X6, so the durations do not depend on math_mode;
 * math_mode selects the decoder's arithmetic: TTS_MATH_BF16, or fp32x6 for every other mode.
 * Head sizes hidden_channels / num_heads as tts_op_mha; hidden_channels <= 512. */
#define TTS_FORWARD_TTS_MAX_FRAMES 5000 /* PositionalEncoding max_len: the pe buffer is [1][H][5000] */
typedef struct TtsForwardTtsCfg {
  int num_chars;
  int out_channels;    /* 80 */
  int hidden_channels; /* 384 */
  int encoder_ffn_channels, encoder_num_heads, encoder_num_layers; /* 1024, 1, 6 */
  int decoder_ffn_channels, decoder_num_heads, decoder_num_layers; /* 1024, 1, 6 */
  int duration_predictor_hidden_channels, duration_predictor_kernel_size; /* 256, 3 */
  int use_pitch;                                                      /* 1 (FastPitch); 0: FastSpeech */
  int pitch_predictor_hidden_channels, pitch_predictor_kernel_size;   /* 256, 3 */
  int pitch_embedding_kernel_size;                                    /* 3 */
  int positional_encoding; /* 1: the decoder input is x sqrt(H) + pe * y_mask */
  int num_speakers;        /* rows of emb_g.weight (use_speaker_embedding); 0: no speaker embedding */
  int math_mode;
} TtsForwardTtsCfg;

/* Host weight order, H = hidden_channels, per FFTransformer layer (F = its ffn channels):
 *   self_attn.in_proj_weight [3H][H], in_proj_bias [3H], self_attn.out_proj.weight [H][H], .bias [H],
 *   conv1.weight [F][H][3], conv1.bias [F], conv2.weight [H][F][3], conv2.bias [H],
 *   norm1.weight [H], norm1.bias [H], norm2.weight [H], norm2.bias [H]
 * emb.weight [num_chars][H]; the encoder's layers; pos_encoder.pe [H][5000] (positional_encoding);
 * the decoder's layers; postnet.weight [out][H][1], postnet.bias [out]; duration_predictor (the
 * 10 tensors of TtsVitsDpCfg's order, no cond layers); with use_pitch: pitch_predictor (the same),
 * pitch_emb.weight [H][1][k], pitch_emb.bias [H]; emb_g.weight [num_speakers][H] (num_speakers > 0). */
int tts_forward_tts_num_weights(const TtsForwardTtsCfg* cfg);
int64_t tts_forward_tts_weight_numel(const TtsForwardTtsCfg* cfg, int index);
int tts_forward_tts_create(const TtsForwardTtsCfg* cfg, const float* const* host_weights, int device, void** handle);
int tts_forward_tts_destroy(void* handle);
/* Everything before the host read of y_lengths.  d_tokens [B][T_en] int64, d_x_lengths [B] int64 (the
 * reference takes every token as valid: pass T_en; shorter lengths mask the encoder's keys and give
 * the padded tokens no frames), d_speaker_ids [B] int64 (NULL when num_speakers == 0),
 * d_given_durations [B][T_en] fp32 or NULL (used in place of the predicted ones).  Outputs:
 * d_o_en [B][H][T_en] (encoder(emb) * x_mask + emb_g, + pitch_emb(pitch) with use_pitch), d_x_mask
 * [B][T_en], d_durations_log [B][T_en], d_pitch [B][T_en] (NULL without use_pitch), d_durations
 * [B][T_en] = round(max((exp(log) - 1) * x_mask * length_scale, 1)) (half to even) * x_mask,
 * d_y_lengths [B] int64 = their sums. */
int tts_forward_tts_encode(void* handle, const int64_t* d_tokens, const int64_t* d_x_lengths,
                           const int64_t* d_speaker_ids, const float* d_given_durations, int B, int T_en,
                           float length_scale, float* d_o_en, float* d_x_mask, float* d_durations_log, float* d_pitch,
                           float* d_durations, int64_t* d_y_lengths, void* hip_stream);
int tts_forward_tts_encode_profiled(void* handle, const int64_t* d_tokens, const int64_t* d_x_lengths,
                                    const int64_t* d_speaker_ids, const float* d_given_durations, int B, int T_en,
                                    float length_scale, float* d_o_en, float* d_x_mask, float* d_durations_log,
                                    float* d_pitch, float* d_durations, int64_t* d_y_lengths, void* hip_stream,
                                    TtsLaunchRecord* records, int max_records, int* n_records);
/* The frames: expansion of d_o_en by d_durations, positional encoding, decoder, postnet.  T_de >=
 * max(y_lengths), at most TTS_FORWARD_TTS_MAX_FRAMES with the positional encoding (TTS_ERR_INVALID
 * beyond, the reference's RuntimeError).  mask_decoder_keys = 0 is the reference (its decoder block
 * is called without a mask: queries attend over the padded frames too); 1 masks the keys past
 * y_lengths.  d_out [B][out_channels][T_de], d_attn [B][T_en][T_de] (or NULL), d_y_mask [B][T_de]. */
int tts_forward_tts_decode(void* handle, const float* d_o_en, const float* d_durations, const float* d_x_mask,
                           const int64_t* d_y_lengths, int B, int T_en, int T_de, int mask_decoder_keys, float* d_out,
                           float* d_attn, float* d_y_mask, void* hip_stream);
int tts_forward_tts_decode_profiled(void* handle, const float* d_o_en, const float* d_durations, const float* d_x_mask,
                                    const int64_t* d_y_lengths, int B, int T_en, int T_de, int mask_decoder_keys,
                                    float* d_out, float* d_attn, float* d_y_mask, void* hip_stream,
                                    TtsLaunchRecord* records, int max_records, int* n_records);
/* d_y [B][H][T] = FFTransformerBlock(d_x [B][H][T]) of the encoder (decoder = 0, fp32x6) or the decoder
 * (decoder = 1, its math mode); d_key_lengths [B] int64 or NULL (no key padding mask).  Every column
 * is computed, the padded ones included. */
int tts_forward_tts_block(void* handle, int decoder, const float* d_x, const int64_t* d_key_lengths, int B, int T,
                          float* d_y, void* hip_stream);

/* ---- Tacotron2 (TTS/tts/models/tacotron2.py, inference; location-sensitive attention, "original"
 * prenet) ----
 * The decoder is a chain of dependent steps, each at most 5 launches on the caller's stream:
 * attention RNN, attention, decoder RNN, projection, stop / bookkeeping / next prenet.  Steps are
 * enqueued in chunks of `chunk`; after each chunk the host reads one word and stops when every
 * utterance has ended.  math_mode TTS_MATH_BF16 stores the attention and decoder RNN matrices as
 * bf16 (fp32 state, cell and accumulation) and runs the encoder / postnet convs in bf16; every other
 * mode keeps fp32 weights with exact fp32 FMA products in the recurrent kernels and fp32x6 convs.
 * Limits (TTS_ERR_UNSUPPORTED): B <= TTS_TACOTRON2_MAX_BATCH, T_en <= TTS_TACOTRON2_MAX_TOKENS,
 * encoder_dim / 2 and query_dim multiples of TTS_LSTM_UNIT_BLOCK, attention_dim <= 128,
 * location_filters <= 32, odd location_kernel_size <= 31, query_dim <= 2048, prenet_dim <= 1024,
 * out_channels * r <= 1024. */
#define TTS_TACOTRON2_MAX_BATCH 32
#define TTS_TACOTRON2_MAX_TOKENS 2048
#define TTS_LSTM_UNIT_BLOCK 4 /* hidden units (four gate rows each) one workgroup of the LSTM step owns */
typedef struct TtsTacotron2Cfg {
  int num_chars;
  int out_channels; /* 80 */
  int r;            /* reduction factor: frames per decoder step */
  int encoder_dim, query_dim, prenet_dim, attention_dim; /* 512, 1024, 256, 128 */
  int location_filters, location_kernel_size;           /* 32, 31 */
  int attention_norm; /* 0: sigmoid(e) / sum sigmoid(e) (the config default), 1: softmax */
  int embed_dim;      /* width appended to every encoder output (speaker embedding or d-vector); 0: none */
  int num_speakers;   /* rows of speaker_embedding.weight [num_speakers][embed_dim]; 0: none (d-vectors) */
  int chunk;          /* decoder steps enqueued between two host reads of the all-done word; 0: 32 */
  int math_mode;
} TtsTacotron2Cfg;

/* Host weight order, E = encoder_dim, He = E / 2, Q = query_dim, P = prenet_dim, A = attention_dim,
 * D = E + embed_dim, C = out_channels:
 *   embedding.weight [num_chars][E];
 *   encoder.convolutions.{0,1,2}: convolution1d.weight [E][E][5], .bias, batch_normalization.weight,
 *     .bias, .running_mean, .running_var;
 *   encoder.lstm: weight_ih_l0 [4He][E], weight_hh_l0 [4He][He], bias_ih_l0, bias_hh_l0, then the four
 *     *_reverse;
 *   decoder.prenet.linear_layers.{0,1}.linear_layer.weight [P][C], [P][P];
 *   decoder.attention_rnn: weight_ih [4Q][P + D], weight_hh [4Q][Q], bias_ih, bias_hh;
 *   decoder.attention: query_layer [A][Q], inputs_layer [A][D], v.weight [A], v.bias [1],
 *     location_conv1d.weight [F][2][k], location_dense.weight [A][F];
 *   decoder.decoder_rnn: weight_ih [4Q][Q + D], weight_hh [4Q][Q], bias_ih, bias_hh;
 *   decoder.linear_projection: weight [C r][Q + D], bias; decoder.stopnet.1: weight [Q + C r], bias [1];
 *   postnet.convolutions.{0..4}: as the encoder's (C -> 512 -> 512 -> 512 -> 512 -> C, kernel 5);
 *   speaker_embedding.weight [num_speakers][embed_dim] (num_speakers > 0). */
int tts_tacotron2_num_weights(const TtsTacotron2Cfg* cfg);
int64_t tts_tacotron2_weight_numel(const TtsTacotron2Cfg* cfg, int index);
int tts_tacotron2_create(const TtsTacotron2Cfg* cfg, const float* const* host_weights, int device, void** handle);
int tts_tacotron2_destroy(void* handle);
/* Embedding -> 3 x (conv k5, folded BatchNorm, ReLU) -> biLSTM (one launch per token, both directions),
 * then the speaker vector appended and inputs_layer applied.  d_tokens [B][T_en] int64; d_x_lengths [B]
 * int64 or NULL (every token valid, the reference): with lengths the biLSTM has pack_padded_sequence
 * semantics (the reverse direction starts at each utterance's last token, padded outputs are 0).
 * Token and speaker ids outside their tables read row 0 (no device-side error; the Python module checks
 * them on the host and raises as torch's embedding does).
 * d_speaker_ids [B] int64 (num_speakers > 0) or d_d_vectors [B][embed_dim] (num_speakers == 0 and
 * embed_dim > 0); NULL otherwise.  Outputs: d_inputs [B][T_en][D], d_processed_inputs [B][A][T_en]. */
int tts_tacotron2_encode(void* handle, const int64_t* d_tokens, const int64_t* d_x_lengths,
                         const int64_t* d_speaker_ids, const float* d_d_vectors, int B, int T_en, float* d_inputs,
                         float* d_processed_inputs, void* hip_stream);
/* The step loop.  d_x_lengths [B] or NULL: attention keys at or past the length are masked.  Utterance b
 * ends at its first step t >= 1 with stop > stop_threshold, or after max_decoder_steps; d_steps [B]
 * int32 receives its step count.  d_decoder_outputs [B][max_decoder_steps][C r], d_alignments
 * [B][max_decoder_steps][T_en] and d_stop_tokens [B][max_decoder_steps] are zeroed first and rows past
 * an utterance's end stay zero (the caller sizes them for max_decoder_steps, whatever the utterances end up
 * needing).  Synchronises the stream once per chunk; *steps_run (host, may be
 * NULL) = the largest step count. */
int tts_tacotron2_decode(void* handle, const float* d_inputs, const float* d_processed_inputs,
                         const int64_t* d_x_lengths, int B, int T_en, int max_decoder_steps, float stop_threshold,
                         float* d_decoder_outputs, float* d_alignments, float* d_stop_tokens, int32_t* d_steps,
                         int* steps_run, void* hip_stream);
int tts_tacotron2_decode_profiled(void* handle, const float* d_inputs, const float* d_processed_inputs,
                                  const int64_t* d_x_lengths, int B, int T_en, int max_decoder_steps,
                                  float stop_threshold, float* d_decoder_outputs, float* d_alignments,
                                  float* d_stop_tokens, int32_t* d_steps, int* steps_run, void* hip_stream,
                                  TtsLaunchRecord* records, int max_records, int* n_records);
/* d_model_outputs [B][steps r][C] = decoder_outputs + postnet(decoder_outputs), rows at or past
 * d_steps[b] * r zero; d_decoder_outputs [B][row_stride][C r] of which the first `steps` rows are
 * read (row_stride = decode's max_decoder_steps).  Every utterance sees zero padding past its own end,
 * as a batch of one does. */
int tts_tacotron2_postnet(void* handle, const float* d_decoder_outputs, const int32_t* d_steps, int B, int steps,
                          int row_stride, float* d_model_outputs, void* hip_stream);
/* One LSTMCell step (gate order i, f, g, o), for kernel tests: d_x [B][I], d_h, d_c [B][H] and the
 * outputs d_h_out, d_c_out [B][H] on the device, torch-layout weights on the host (w_ih [4H][I],
 * w_hh [4H][H], b_ih, b_hh [4H]).  math_mode TTS_MATH_BF16: bf16 matrices; else fp32 FMA.
 * B <= 32 and H % TTS_LSTM_UNIT_BLOCK == 0 (TTS_ERR_UNSUPPORTED otherwise).  Column b does not depend on B. */
int tts_op_lstm_cell(const float* d_x, const float* d_h, const float* d_c, int B, int I, int H, const float* h_w_ih,
                     const float* h_w_hh, const float* h_b_ih, const float* h_b_hh, int math_mode, float* d_h_out,
                     float* d_c_out, void* hip_stream);

/* ------------------------------------------------------------------------------------ */
/* Conv2d of the SE-ResNet speaker encoder (TTS/encoder/models/resnet.py)                  */
/* ------------------------------------------------------------------------------------ */

/* One nn.Conv2d with its epilogue, one launch on the matrix cores:
 *   d_out = scale act(conv2d(d_x, w, stride, padding = (ksize - 1) / 2) + bias) + shift
 * act = relu (relu != 0) or the identity; scale / shift per output channel: an eval-mode BatchNorm2d
 * after the ReLU (conv1 / bn1 of the stem and of SEBasicBlock), or bn2 folded by the caller.
 * d_x [B][Cin][F][T] and d_out [B][Cout][ceil(F / stride)][ceil(T / stride)] on the device, fp32,
 * not aliased; w [Cout][Cin][ksize][ksize] and bias / scale / shift [Cout] on the host (NULL: 0 / 1 / 0).
 * ksize 3 (the 3x3 convs) or 1 (the downsample conv); stride 1 or 2; Cout <= 4096; each batch item's
 * input and output plane below 2 GiB; output rows x ceil(Cout / 256) <= 65535; B <= 65535 (TTS_ERR_UNSUPPORTED
 * otherwise, before any launch).  math_mode TTS_MATH_FP32_X6 or TTS_MATH_BF16 (TTS_MATH_FP32 and
 * TTS_MATH_FP32_F16X3 run the fp32x6 kernel: both are held to the fp32 parity gates).  An output
 * element does not depend on B, and a repeated call returns the same bits. */
int tts_op_conv2d_3x3(const float* d_x, int B, int Cin, int F, int T, const float* h_w, int Cout, int ksize,
                      int stride, const float* h_bias, int relu, const float* h_scale, const float* h_shift,
                      int math_mode, float* d_out, void* hip_stream);
/* Output columns one workgroup of the conv2d kernel computes (one output row, every channel). */
int tts_op_conv2d_3x3_tile(void);

/* ------------------------------------------------------------------------------------ */
/* ResNetSpeakerEncoder (TTS/encoder/models/resnet.py): reference wav -> d-vector          */
/* ------------------------------------------------------------------------------------ */

#define TTS_SPK_SAP 0
#define TTS_SPK_ASP 1
/* Limits of the implemented path (TTS_ERR_UNSUPPORTED beyond, before any launch) */
#define TTS_SPK_MAX_FILTERS 256   /* num_filters[i]: multiples of 8 in [8, 256] (the SE reduction is C / 8) */
#define TTS_SPK_MAX_BATCH 4096    /* rows of one forward (compute_embedding's windows count as rows) */
#define TTS_SPK_MAX_FRAMES 65535  /* frames T of one forward */

/* Mirrors ResNetSpeakerEncoder.__init__: the stem conv1 (1 -> num_filters[0], 3x3, bias) -> ReLU -> bn1,
 * layers[i] SEBasicBlocks of num_filters[i] channels (stride 2 on the first block of layers 2-4, a
 * 1x1 downsample conv + BatchNorm wherever the stride or the channel count changes), attentive
 * pooling (SAP / ASP) over time and the fc projection.  use_torch_spec: the front end (pre-emphasis,
 * centred STFT with a win_length window, power, mel filterbank) on the device; then fft_size,
 * win_length and hop_length must satisfy TtsStftCfg's limits.  The log (log_input) and the
 * instance norm run either way.  Implemented: input_dim a multiple of 8 in [8, 512], num_filters as
 * above, layers[i] >= 1 with at most 64 blocks in all, proj_dim in [1, 4096].
 * math_mode: TTS_MATH_BF16 runs the trunk's convs and the two attention convs on bf16 operands;
 * every other mode runs them fp32x6.  The front end, the SE path, the pooling, fc and the
 * normalisation are fp32-faithful in every mode. */
typedef struct TtsSpeakerEncoderCfg {
  int input_dim;
  int proj_dim;
  int layers[4];
  int num_filters[4];
  int encoder_type; /* TTS_SPK_SAP or TTS_SPK_ASP */
  int log_input;
  int use_torch_spec;
  int fft_size;   /* torch_spec only */
  int win_length;
  int hop_length;
  int math_mode;
} TtsSpeakerEncoderCfg;

/* Host weights, fp32, in state_dict order ("BN" = weight, bias, running_mean, running_var):
 *   use_torch_spec only: torch_spec.0.filter [2], torch_spec.1.spectrogram.window [win_length],
 *     torch_spec.1.mel_scale.fb [fft_size/2 + 1][input_dim]
 *   conv1.weight [F0][1][3][3], conv1.bias, bn1 BN
 *   per block of layer L (C = num_filters[L], Ci its input channels):
 *     conv1.weight [C][Ci][3][3], bn1 BN, conv2.weight [C][C][3][3], bn2 BN,
 *     se.fc.0.weight [C/8][C], se.fc.0.bias, se.fc.2.weight [C][C/8], se.fc.2.bias,
 *     then, where the block has one, downsample.0.weight [C][Ci][1][1], downsample.1 BN
 *   attention.0.weight [128][D][1] (D = num_filters[3] * input_dim / 8), attention.0.bias, attention.2 BN,
 *   attention.3.weight [D][128][1], attention.3.bias, fc.weight [proj_dim][D or 2 D], fc.bias */
int tts_speaker_encoder_num_weights(const TtsSpeakerEncoderCfg* cfg);
int64_t tts_speaker_encoder_weight_numel(const TtsSpeakerEncoderCfg* cfg, int idx);
int tts_speaker_encoder_create(const TtsSpeakerEncoderCfg* cfg, const float* const* host_weights, int device,
                               void** handle);
int tts_speaker_encoder_destroy(void* handle);
/* Frames T of an n-sample wav (use_torch_spec: 1 + n / hop_length; else n itself: the input is
 * features); -TTS_ERR_* when the input is outside the limits (shorter than fft_size/2 + 1 samples, a
 * row of 2 GiB or more, more than TTS_SPK_MAX_FRAMES frames). */
int64_t tts_speaker_encoder_num_frames(const void* handle, int64_t n);
/* d_out[B][proj_dim] = forward(x, l2_norm).  d_x: [B][n] wav samples at the model's sample rate
 * (use_torch_spec) or [B][input_dim][n] features, contiguous fp32 on the device.  Row b does not
 * depend on B, and a repeated call returns the same bits.  No host synchronisation. */
int tts_speaker_encoder_forward(void* handle, const float* d_x, int B, int64_t n, int l2_norm, float* d_out,
                                void* hip_stream);
int tts_speaker_encoder_forward_profiled(void* handle, const float* d_x, int B, int64_t n, int l2_norm, float* d_out,
                                         void* hip_stream, TtsLaunchRecord* records, int max_records, int* n_records);
/* d_feat[B][input_dim][T]: the trunk's input (front end, log, instance norm) alone, for tests. */
int tts_speaker_encoder_features(void* handle, const float* d_x, int B, int64_t n, float* d_feat, void* hip_stream);

/* The linear-spectrogram plan of tts_stft_create with torch.stft's frame centring: reflect padding
 * n_fft / 2, T = 1 + N / hop_length frames (tts_stft_num_frames_centered), N > n_fft / 2.  The handle
 * is used and destroyed like tts_stft_create's; the output is sqrt(|X|^2 + 1e-6) all the same. */
int tts_stft_create_centered(const TtsStftCfg* cfg, const float* h_window, int device, void** handle);
int tts_stft_num_frames_centered(const TtsStftCfg* cfg, int64_t N);

/* ---- XTTS GPT (TTS/tts/layers/xtts/gpt.py, gpt_inference.py: the autoregressive GPT-2 trunk that
 * turns text tokens and conditioning latents into audio codes and the decoder's latents) ----
 * A step is a chain of launches on the caller's stream: 5 per layer (c_attn with ln_1 -> q and the
 * cache row, attention over the cache, c_proj + residual, c_fc with ln_2 + gelu_new, mlp c_proj +
 * residual) and 2 beyond the layers (ln_f / final_norm / mel_head; logits -> token with the
 * bookkeeping and the next input).  Steps are enqueued in chunks of `chunk`; after each chunk the
 * host reads one word and stops when every utterance has ended.  math_mode TTS_MATH_BF16 stores the
 * layers' matrices and mel_head as bf16 (fp32 accumulation); every other mode keeps fp32 matrices with
 * exact fp32 FMA products.  The KV cache, the residual stream, LayerNorm and the softmax are fp32 in
 * every mode.  Utterance b of a batch is bitwise its own batch of one.
 * Limits (TTS_ERR_UNSUPPORTED, before any launch): B <= TTS_XTTS_GPT_MAX_BATCH, head size
 * model_dim / heads of 32, 64 or 128, model_dim a multiple of 64, n_audio_tokens <=
 * TTS_XTTS_GPT_MAX_AUDIO_TOKENS.  A sequence past the position tables is TTS_ERR_INVALID (the
 * reference's assert). */
#define TTS_XTTS_GPT_MAX_BATCH 32
#define TTS_XTTS_GPT_MAX_AUDIO_TOKENS 8194
typedef struct TtsXttsGptCfg {
  int layers, model_dim, heads;      /* 30, 1024, 16 */
  int n_text_tokens, n_audio_tokens; /* rows of text_embedding / mel_embedding (and of mel_head) */
  int start_text_token, stop_text_token, start_audio_token, stop_audio_token;
  int text_positions;   /* rows of text_pos_embedding.emb.weight (max_text_tokens + 2) */
  int mel_positions;    /* rows of mel_pos_embedding.emb.weight */
  int prompt_positions; /* P: conditioning latent rows in front of every utterance's text */
  int chunk;            /* steps enqueued between two host reads of the all-done word; 0: 32 */
  int math_mode;
} TtsXttsGptCfg;

/* Host weight order, E = model_dim:
 *   text_embedding.weight [n_text][E]; mel_embedding.weight [n_audio][E];
 *   text_pos_embedding.emb.weight [text_positions][E]; mel_pos_embedding.emb.weight [mel_positions][E];
 *   per layer gpt.h.{i}: ln_1.weight, ln_1.bias, attn.c_attn.weight [E][3E], .bias, attn.c_proj.weight
 *     [E][E], .bias, ln_2.weight, ln_2.bias, mlp.c_fc.weight [E][4E], .bias, mlp.c_proj.weight [4E][E],
 *     .bias (HF Conv1D: [in][out], y = x W + b, passed as stored);
 *   gpt.ln_f.weight, .bias; final_norm.weight, .bias; mel_head.weight [n_audio][E], .bias. */
int tts_xtts_gpt_num_weights(const TtsXttsGptCfg* cfg);
int64_t tts_xtts_gpt_weight_numel(const TtsXttsGptCfg* cfg, int index);
int tts_xtts_gpt_create(const TtsXttsGptCfg* cfg, const float* const* host_weights, int device, void** handle);
int tts_xtts_gpt_destroy(void* handle);
/* The prefix of utterance b, [cond latents (P rows) | start_text, text_b, stop_text] with the text
 * position embedding, through the layers into the cache rows [0, P + L_b + 2).  d_cond [B][P][E],
 * d_tokens [B][T_text] int64, d_text_lengths [B] int64 or NULL (L_b = T_text).  The handle keeps the
 * prefix (and room for max_new_tokens steps behind it) until the next prefill; tts_xtts_gpt_generate
 * and tts_xtts_gpt_latents may follow it any number of times.  Token ids outside the table are clamped
 * (the Python module raises IndexError on the host, as torch's embedding does).  No host
 * synchronisation.  One whole-sequence pass on the conv path: per layer LayerNorm, c_attn as a 1x1 conv
 * (fp32x6; in TTS_MATH_BF16 on the bf16-rounded matrix the steps stream, activations stay fp32), K and V
 * from the planes into the cache layout, causal MFMA
 * attention (tts_op_mha_causal's kernel), c_proj + residual, LayerNorm, c_fc, gelu_new, mlp c_proj +
 * residual.  The _profiled form is an extension for the step benchmark. */
int tts_xtts_gpt_prefill(void* handle, const float* d_cond, const int64_t* d_tokens, const int64_t* d_text_lengths,
                         int B, int T_text, int max_new_tokens, void* hip_stream);
int tts_xtts_gpt_prefill_profiled(void* handle, const float* d_cond, const int64_t* d_tokens,
                                  const int64_t* d_text_lengths, int B, int T_text, int max_new_tokens,
                                  void* hip_stream, TtsLaunchRecord* records, int max_records, int* n_records);
/* The step loop.  Step s reads the hidden state of mel position s (the start token at s = 0) and
 * chooses code s: repetition penalty over {1, start_audio} and the codes so far, then with d_uniforms
 * [B][max_new_tokens] (in [0, 1)): temperature, top-k (<= 0: off), top-p and a draw by inverse CDF in
 * token order; with d_uniforms NULL: the argmax after the penalty, the lowest id on ties.  Utterance
 * b ends at its first stop_audio or after max_new_tokens (<= the prefill's); d_codes [B][max_new_tokens]
 * int32 holds stop_audio past its end and d_lengths [B] int32 its code count, the stop included.
 * Optional (NULL: not written), zero past an utterance's end: d_logits [B][max_new_tokens][n_audio],
 * the logits after mel_head, and d_latents [B][max_new_tokens][E], final_norm(ln_f(h)) of every
 * step's position.  d_latents is an extension: it holds what the reference's second pass
 * (tts_xtts_gpt_latents over the generated codes) recomputes, so a caller that passes it can skip that
 * pass, as Xtts.inference does.  Synchronises the stream once per chunk; *steps_run (host, may be NULL) = steps
 * enqueued. */
int tts_xtts_gpt_generate(void* handle, int max_new_tokens, float repetition_penalty, float temperature, int top_k,
                          float top_p, const float* d_uniforms, int32_t* d_codes, int32_t* d_lengths, float* d_logits,
                          float* d_latents, int* steps_run, void* hip_stream);
int tts_xtts_gpt_generate_profiled(void* handle, int max_new_tokens, float repetition_penalty, float temperature,
                                   int top_k, float top_p, const float* d_uniforms, int32_t* d_codes,
                                   int32_t* d_lengths, float* d_logits, float* d_latents, int* steps_run,
                                   void* hip_stream, TtsLaunchRecord* records, int max_records, int* n_records);
/* The teacher-forced pass over the mel inputs [start_audio, c_0 .. c_{n_b - 1}, stop_audio] of given
 * codes d_codes [B][S] int32 with d_lengths [B] int32 (n_b), mel positions [0, rows), rows <= the
 * prefill's max_new_tokens.  d_latents [B][rows][E] (or NULL): final_norm(ln_f(h)), rows at or past
 * n_b - 2 zero (the reference drops the last 4 of its n_b + 2 positions); d_logits
 * [B][rows][n_audio] (or NULL), rows at or past n_b + 2 zero.  No host synchronisation.  One
 * whole-sequence pass over [prefix | mel rows] on the conv path, as the prefill (the prefix from the input
 * rows the prefill kept), then ln_f / final_norm / mel_head per mel position. */
int tts_xtts_gpt_latents(void* handle, const int32_t* d_codes, const int32_t* d_lengths, int S, int rows,
                         float* d_latents, float* d_logits, void* hip_stream);
int tts_xtts_gpt_latents_profiled(void* handle, const int32_t* d_codes, const int32_t* d_lengths, int S, int rows,
                                  float* d_latents, float* d_logits, void* hip_stream, TtsLaunchRecord* records,
                                  int max_records, int* n_records);
/* Single-query attention over a KV cache, for kernel tests: d_q [B][E], d_k / d_v [B][cap][E],
 * d_lengths [B] int32 (keys [0, len_b), 1 <= len_b <= cap), d_out [B][E].  A workgroup of
 * tts_op_gpt_decode_attn_waves() waves per (utterance, head); wave w takes the 64-key tiles w, w + waves,
 * ... and the waves' partial results are merged in wave order.  Row b does not depend on B. */
int tts_op_gpt_decode_attn(const float* d_q, const float* d_k, const float* d_v, const int32_t* d_lengths, int B,
                           int E, int heads, int cap, float* d_out, void* hip_stream);
int tts_op_gpt_decode_attn_waves(void);
/* tts_op_mha with a causal mask (the GPT's attention over a whole sequence): query i attends to the
 * keys j <= i with j < key_lengths[b].  Key tiles wholly above a workgroup's diagonal are skipped, the
 * diagonal tiles are masked, so the outputs at positions <= i are bitwise independent of everything
 * at a position > i.  Arguments, layouts and math modes as tts_op_mha (tile: tts_op_mha_tile()); head
 * sizes 32, 64 or 128 with E <= 2048 (TTS_ERR_UNSUPPORTED otherwise).  It is the attention of the XTTS
 * GPT's prefill and latent pass. */
int tts_op_mha_causal(const float* d_qkv, const int64_t* d_key_lengths, int B, int E, int heads, int T,
                      int math_mode, float* d_out, void* hip_stream);
/* The logits -> token step alone, for kernel tests: d_logits [B][V], d_codes [B][n_prev + 1] int32
 * (the earlier codes, then the slot that receives the token), d_uniforms [B] or NULL (greedy). */
int tts_op_gpt_sample(const float* d_logits, int B, int V, int32_t* d_codes, int n_prev, int start_audio_token,
                      float repetition_penalty, float temperature, int top_k, float top_p, const float* d_uniforms,
                      void* hip_stream);

/* ---- XTTS conditioning (TTS/tts/layers/xtts/latent_encoder.py ConditioningEncoder, perceiver_encoder.py
 * PerceiverResampler, TTS/tts/models/xtts.py wav_to_mel_cloning): reference mel -> the GPT's
 * conditioning latents, the GPT half of Xtts.get_conditioning_latents ----
 * style_emb is a chain of launches on the caller's stream:
 *   init:       the 1x1 conv spec_dim -> model_dim (1 launch);
 *   per block:  GroupNorm | qkv conv (rows permuted at pack time from the reference's head-major interleaved
 *               order into q | k | v) | flash attention (tts_op_mha_wide) | proj_out conv + the normalised
 *               input as residual (4 launches);
 *   latents:    the learned latents copied to every batch item (1 launch);
 *   per layer:  to_q | to_kv on the latents | to_kv on the context | cross-attention over the two key buffers |
 *               to_out + residual | FF product with the GEGLU epilogue | FF product + residual (7 launches);
 *   RMSNorm (1 launch).
 * The latents are kept as planes [B][E][num_latents].  The encoder's products and to_kv on the context are
 * 1x1 convs of the shared conv path; the products over the latent columns are a kernel of their own.
 * math_mode TTS_MATH_BF16: the convs and the self-attention take bf16 operands, the products over the latent
 * columns stream bf16-stored matrices against fp32 activations; every other mode runs the convs and the
 * attention fp32x6 and those products in fp32 FMA.  GroupNorm, the cross-attention, GEGLU, RMSNorm and the
 * mel front end are fp32-faithful in every mode.  Row b does not depend on B and a repeated call returns the
 * same bits.
 * Limits (TTS_ERR_UNSUPPORTED, before any launch): model_dim <= 2048 with a head size model_dim / heads
 * of 32, 64 or 128; num_latents <= TTS_XTTS_COND_MAX_LATENTS; perceiver_dim_head <= 256 and
 * perceiver_heads * perceiver_dim_head <= 4096; attn_blocks <= 64; perceiver_depth <= 64; spec_dim <= 1024;
 * ff_mult <= 16; n_fft, hop_length and win_length inside TtsStftCfg's limits; per call B <=
 * TTS_XTTS_COND_MAX_BATCH and num_latents + T <= TTS_XTTS_COND_MAX_KEYS (the cross-attention keeps a score
 * row in LDS); a clip of at least n_fft / 2 + 1 samples (the reflect padding) and below 2 GiB. */
#define TTS_XTTS_COND_MAX_BATCH 64
#define TTS_XTTS_COND_MAX_LATENTS 64
#define TTS_XTTS_COND_MAX_KEYS 8192
typedef struct TtsXttsCondCfg {
  int spec_dim;                 /* 80 */
  int model_dim, heads;         /* 1024, 16 */
  int attn_blocks;              /* 6 */
  int perceiver_depth;          /* 2 */
  int num_latents;              /* 32 */
  int perceiver_dim_head;       /* 64 */
  int perceiver_heads;          /* 8 */
  int ff_mult;                  /* 4: the FF's inner width is int(model_dim * ff_mult * 2 / 3) */
  int n_fft, hop_length, win_length; /* 2048, 256, 1024 */
  int math_mode;
} TtsXttsCondCfg;

/* Host weight order, E = model_dim, inner = perceiver_heads * perceiver_dim_head, I the FF's inner width:
 *   conditioning_encoder: init.weight [E][spec_dim][1], init.bias; per block attn.{i}: norm.weight,
 *     norm.bias, qkv.weight [3E][E][1], qkv.bias, proj_out.weight [E][E][1], proj_out.bias (as stored);
 *   conditioning_perceiver: latents [num_latents][E]; per layer layers.{i}: 0.to_q.weight [inner][E],
 *     0.to_kv.weight [2 inner][E], 0.to_out.weight [E][inner], 1.0.weight [2I][E], 1.0.bias,
 *     1.2.weight [E][I], 1.2.bias; norm.gamma [E];
 *   the front end: the STFT window [win_length], the mel filterbank fb [n_fft/2 + 1][spec_dim]. */
int tts_xtts_cond_num_weights(const TtsXttsCondCfg* cfg);
int64_t tts_xtts_cond_weight_numel(const TtsXttsCondCfg* cfg, int index);
int tts_xtts_cond_create(const TtsXttsCondCfg* cfg, const float* const* host_weights, int device, void** handle);
int tts_xtts_cond_destroy(void* handle);
/* Frames T = 1 + N / hop_length of an N-sample clip (centred STFT, reflect padding n_fft / 2: N > n_fft / 2);
 * -TTS_ERR_* outside the limits. */
int64_t tts_xtts_cond_num_frames(const void* handle, int64_t N);
/* wav_to_mel_cloning: d_mel [B][spec_dim][T] = log(max(fb^T |STFT(d_wav)|^2, 1e-5)) / d_mel_norms[:, None];
 * d_wav [B][N] at the clip's 22 050 Hz, d_mel_norms [spec_dim] (the checkpoint's mel_stats). */
int tts_xtts_cond_mel(void* handle, const float* d_wav, int B, int64_t N, const float* d_mel_norms, float* d_mel,
                      void* hip_stream);
/* get_style_emb: d_mel [B][spec_dim][T] -> d_out [B][E][num_latents].  No host synchronisation. */
int tts_xtts_cond_style_emb(void* handle, const float* d_mel, int B, int T, float* d_out, void* hip_stream);
int tts_xtts_cond_style_emb_profiled(void* handle, const float* d_mel, int B, int T, float* d_out, void* hip_stream,
                                     TtsLaunchRecord* records, int max_records, int* n_records);

/* torchaudio.functional.resample (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) as a polyphase
 * product: with o = orig_freq / gcd, n = new_freq / gcd, base = min(o, n) 0.99 and w = ceil(6 o / base),
 * y[f n + p] = sum_k kern[p][k] xpad[f o + k] over the 2 w + o taps, xpad = x with w zeros in front, cut to
 * ceil(n N / o) samples (tts_resample_num_samples).  The table is built on the host in fp64 and stored
 * fp32; a sample's sum runs in fp64 in tap order.  o, n <= TTS_RESAMPLE_MAX_FACTOR, rows below 2^31
 * samples (TTS_ERR_UNSUPPORTED otherwise).  d_x [B][N] -> d_y [B][ceil(n N / o)]. */
#define TTS_RESAMPLE_MAX_FACTOR 1024
int tts_resample_create(int orig_freq, int new_freq, int device, void** handle);
int tts_resample_destroy(void* handle);
int64_t tts_resample_num_samples(const void* handle, int64_t N);
int tts_resample_forward(void* handle, const float* d_x, int B, int64_t N, float* d_y, void* hip_stream);

/* Kernel-test entries of the conditioning path; all device pointers unless named h_.
 * GroupNorm(groups, C, eps) with the affine over planes d_x [B][C][T]: two-pass statistics per
 * (b, group), one workgroup each; C % groups == 0, planes below 2 GiB. */
int tts_op_groupnorm(const float* d_x, int B, int C, int T, int groups, const float* d_gamma, const float* d_beta,
                     float eps, float* d_y, void* hip_stream);
/* tts_op_mha past its 512 channels: head sizes 32, 64 or 128 with E <= 2048 (TTS_ERR_UNSUPPORTED
 * otherwise); arguments, layouts, math modes and tile as tts_op_mha, and the same bits where both accept.
 * What tts_op_mha and tts_op_mha_causal accept is unchanged. */
int tts_op_mha_wide(const float* d_qkv, const int64_t* d_key_lengths, int B, int E, int heads, int T, int math_mode,
                    float* d_out, void* hip_stream);
/* The perceiver's attention: L latent queries d_q [B][heads dim_head][L] against the L + T keys of
 * d_kv_lat [B][2 heads dim_head][L] (first) and d_kv_ctx [B][2 heads dim_head][T] (k rows, then v rows),
 * softmax(q k^T dim_head^-0.5) v -> d_out [B][heads dim_head][L]; fp32.  L <= TTS_XTTS_COND_MAX_LATENTS,
 * dim_head <= 256, L + T <= TTS_XTTS_COND_MAX_KEYS. */
int tts_op_cross_attn(const float* d_q, const float* d_kv_lat, const float* d_kv_ctx, int B, int heads, int dim_head,
                      int L, int T, float* d_out, void* hip_stream);
/* The perceiver's feed-forward with its residual over planes d_x [B][E][L]: d_out = d_x + W2 (gelu_erf(gate)
 * a) + b2 with [a | gate] = W0 d_x + b0; h_w0 [2I][E], h_b0 [2I], h_w2 [E][I], h_b2 [E] on the host;
 * B <= TTS_XTTS_COND_MAX_BATCH, E <= 4096, 1 <= I <= 16384, L <= TTS_XTTS_COND_MAX_LATENTS
 * (TTS_ERR_UNSUPPORTED otherwise); I need not be a multiple of anything.
 * Two launches of the perceiver's product kernel: W0 with the GEGLU epilogue, then W2 with the bias and the
 * residual.  math_mode TTS_MATH_BF16: bf16-stored matrices, fp32 activations and accumulation. */
int tts_op_cond_ff(const float* d_x, int B, int E, int I, int L, const float* h_w0, const float* h_b0,
                   const float* h_w2, const float* h_b2, int math_mode, float* d_out, void* hip_stream);
/* d_y[b][:][l] = d_x[b][:][l] / max(||d_x[b][:][l]||_2, 1e-12) sqrt(E) d_gamma over planes [B][E][L]. */
int tts_op_rmsnorm(const float* d_x, int B, int E, int L, const float* d_gamma, float* d_y, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* TTS_MI355X_H */
