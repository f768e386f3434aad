// extern "C" entry points of libtts_mi355x.so (declared in include/tts_mi355x.h).
// Every call converts library exceptions into a status code + thread-local message.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "conv2d.hpp"
#include "fft_attn.hpp"
#include "forward_tts.hpp"
#include "glow.hpp"
#include "handoff.hpp"
#include "hifigan.hpp"
#include "mas.hpp"
#include "melgan.hpp"
#include "speaker_encoder.hpp"
#include "stft.hpp"
#include "tacotron2.hpp"
#include "text.hpp"
#include "vits.hpp"
#include "xtts_cond.hpp"
#include "xtts_gpt.hpp"
#include "tts_mi355x.h"

namespace {
thread_local std::string g_last_error;

template <class F>
int guarded(F&& f) {
  try {
    g_last_error.clear();
    f();
    return TTS_OK;
  } catch (const tts::Error& e) {
    g_last_error = e.what();
    return e.code;
  } catch (const std::bad_alloc&) {
    g_last_error = "host allocation failed";
    return TTS_ERR_OOM;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return TTS_ERR_INVALID;
  } catch (...) {
    g_last_error = "unknown error";
    return TTS_ERR_INVALID;
  }
}

void export_records(const tts::Profiler& prof, TtsLaunchRecord* records, int max_records, int* n_records) {
  *n_records = (int)prof.recs.size();
  for (int i = 0; i < (int)prof.recs.size() && i < max_records && records; ++i) {
    const auto& r = prof.recs[i];
    std::memset(records[i].name, 0, sizeof(records[i].name));
    std::strncpy(records[i].name, r.name.c_str(), sizeof(records[i].name) - 1);
    records[i].flops = r.flops;
    records[i].bytes = r.bytes;
    float ms = 0.f;
    TTS_HIP_CHECK(hipEventElapsedTime(&ms, r.a, r.b));
    records[i].ms = ms;
  }
}

// Device copy of n host floats on the current device (host == nullptr: left uninitialised), for
// the single-op entry points.
tts::DeviceBuffer to_device(const float* host, size_t n) {
  tts::DeviceBuffer b;
  int dev = 0;
  TTS_HIP_CHECK(hipGetDevice(&dev));
  b.grow(dev, n * sizeof(float), "operand");
  if (host && n) TTS_HIP_CHECK(hipMemcpy(b.as<>(), host, n * sizeof(float), hipMemcpyHostToDevice));
  return b;
}

// The entry points every handle family repeats.  validate and shapes take the cfg by reference.
template <class Cfg, class Validate, class Shapes>
int num_weights(const Cfg* cfg, Validate validate, Shapes shapes) {
  int n = -1;
  int st = guarded([&] {
    TTS_REQUIRE(cfg, 1, "NULL cfg");
    validate(*cfg);
    n = (int)shapes(*cfg).size();
  });
  return st == TTS_OK ? n : -st;
}

template <class Cfg, class Validate, class Shapes>
int64_t weight_numel(const Cfg* cfg, int idx, Validate validate, Shapes shapes) {
  int64_t n = -1;
  guarded([&] {
    TTS_REQUIRE(cfg, 1, "NULL cfg");
    validate(*cfg);
    auto s = shapes(*cfg);
    TTS_REQUIRE(idx >= 0 && idx < (int)s.size(), 1, "weight index out of range");
    n = s[idx];
  });
  return n;
}

// host_weights: the weight pointer array, or the STFT's window
template <class T, class Cfg, class W>
int create(const Cfg* cfg, const W* host_weights, int device, void** handle) {
  return guarded([&] {
    TTS_REQUIRE(cfg && host_weights && handle, 1, "NULL argument");
    *handle = nullptr;
    *handle = new T(*cfg, host_weights, device);
  });
}

template <class T>
int destroy(void* handle) {
  return guarded([&] { delete static_cast<T*>(handle); });
}

// A *_profiled entry point: body(T&, hipStream_t, Profiler*) is the executor call, timed per launch.
template <class T, class Body>
int profiled(void* handle, void* hip_stream, TtsLaunchRecord* records, int max_records, int* n_records, Body body) {
  return guarded([&] {
    TTS_REQUIRE(handle && n_records, 1, "NULL argument");
    auto* h = static_cast<T*>(handle);
    auto s = static_cast<hipStream_t>(hip_stream);
    tts::Profiler prof;
    {
      tts::DeviceGuard g(h->device());
      body(*h, s, &prof);
      TTS_HIP_CHECK(hipStreamSynchronize(s));
    }
    export_records(prof, records, max_records, n_records);
  });
}
}  // namespace

extern "C" {

const char* tts_last_error(void) { return g_last_error.c_str(); }
int tts_abi_version(void) { return 115; }
const char* tts_build_target(void) { return "gfx950"; }

// ----------------------------------------------------------------------------- HiFiGAN
int tts_hifigan_num_weights(const TtsHifiganCfg* cfg) {
  return num_weights(cfg, tts::hifigan_validate, tts::hifigan_weight_shapes);
}

int64_t tts_hifigan_weight_numel(const TtsHifiganCfg* cfg, int idx) {
  return weight_numel(cfg, idx, tts::hifigan_validate, tts::hifigan_weight_shapes);
}

int tts_hifigan_create(const TtsHifiganCfg* cfg, const float* const* host_weights, int device,
                       void** handle) {
  return create<tts::Hifigan>(cfg, host_weights, device, handle);
}

int tts_hifigan_destroy(void* handle) { return destroy<tts::Hifigan>(handle); }

int64_t tts_hifigan_output_length(const void* handle, int T, int pad) {
  if (!handle) return -1;
  return static_cast<const tts::Hifigan*>(handle)->out_len(T, pad);
}

int64_t tts_hifigan_workspace_bytes(const void* handle, int B, int T, int pad) {
  if (!handle) return -1;
  return static_cast<const tts::Hifigan*>(handle)->workspace_bytes(B, T, pad);
}

int tts_hifigan_reserve(void* handle, int B, int T, int pad) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    TTS_REQUIRE(B >= 1 && T >= 1 && pad >= 0, 1, "bad shape");
    static_cast<tts::Hifigan*>(handle)->reserve(B, T, pad);
  });
}

int tts_hifigan_forward(void* handle, const float* d_mel, int B, int C, int T, int pad,
                        const float* d_g, float* d_wav, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::Hifigan*>(handle)->forward(d_mel, B, C, T, pad, d_g, d_wav,
                                                static_cast<hipStream_t>(hip_stream), nullptr);
  });
}

int tts_hifigan_forward_profiled(void* handle, const float* d_mel, int B, int C, int T, int pad,
                                 const float* d_g, float* d_wav, void* hip_stream,
                                 TtsLaunchRecord* records, int max_records, int* n_records) {
  auto body = [&](tts::Hifigan& h, hipStream_t s, tts::Profiler* prof) {
    h.forward(d_mel, B, C, T, pad, d_g, d_wav, s, prof);
  };
  return profiled<tts::Hifigan>(handle, hip_stream, records, max_records, n_records, body);
}

// ----------------------------------------------------------------------------- Glow encoder + glue
// with its defaults: the duration predictor included, the embedding as wide as the encoder
static std::vector<int64_t> glow_encoder_shapes(const TtsGlowEncoderCfg& c) {
  return tts::glow_encoder_weight_shapes(c);
}

int tts_glow_encoder_num_weights(const TtsGlowEncoderCfg* cfg) {
  return num_weights(cfg, tts::glow_encoder_validate, glow_encoder_shapes);
}

int64_t tts_glow_encoder_weight_numel(const TtsGlowEncoderCfg* cfg, int idx) {
  return weight_numel(cfg, idx, tts::glow_encoder_validate, glow_encoder_shapes);
}

int tts_glow_encoder_create(const TtsGlowEncoderCfg* cfg, const float* const* host_weights, int device,
                            void** handle) {
  return create<tts::GlowEncoder>(cfg, host_weights, device, handle);
}

int tts_glow_encoder_destroy(void* handle) { return destroy<tts::GlowEncoder>(handle); }

int tts_glow_encoder_forward(void* handle, const int64_t* d_tokens, const int64_t* d_lengths, const float* d_g,
                             int B, int T, float* d_x_m, float* d_x_logs, float* d_logw, float* d_x_mask,
                             void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::GlowEncoder*>(handle)->forward(d_tokens, d_lengths, d_g, B, T, d_x_m, d_x_logs, d_logw,
                                                    d_x_mask, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_glow_encoder_forward_profiled(void* handle, const int64_t* d_tokens, const int64_t* d_lengths,
                                      const float* d_g, int B, int T, float* d_x_m, float* d_x_logs, float* d_logw,
                                      float* d_x_mask,
                                      void* hip_stream, TtsLaunchRecord* records, int max_records,
                                      int* n_records) {
  auto body = [&](tts::GlowEncoder& h, hipStream_t s, tts::Profiler* prof) {
    h.forward(d_tokens, d_lengths, d_g, B, T, d_x_m, d_x_logs, d_logw, d_x_mask, s, prof);
  };
  return profiled<tts::GlowEncoder>(handle, hip_stream, records, max_records, n_records, body);
}

int tts_glow_durations(const float* d_logw, const float* d_x_mask, int B, int T_x, float length_scale,
                       float* d_w_ceil, int64_t* d_y_lengths, float* d_o_attn_dur, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_logw && d_x_mask && d_w_ceil && d_y_lengths, 1, "NULL argument");
    TTS_REQUIRE(B >= 1 && T_x >= 1, 1, "batch and token count must be >= 1");
    tts::launch_durations(d_logw, d_x_mask, d_w_ceil, d_y_lengths, d_o_attn_dur, B, T_x, length_scale,
                          static_cast<hipStream_t>(hip_stream));
    TTS_HIP_CHECK(hipGetLastError());
  });
}

int tts_glow_expand(const float* d_w_ceil, const float* d_x_mask, const int64_t* d_y_lengths,
                    const float* d_o_mean, const float* d_o_log_scale, const float* d_noise, float noise_scale,
                    int B, int C, int T_x, int T_y, float* d_z, float* d_y_mask, float* d_y_mean,
                    float* d_y_log_scale, float* d_attn, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_w_ceil && d_x_mask && d_y_lengths && d_o_mean && d_z && d_y_mask, 1, "NULL argument");
    TTS_REQUIRE(B >= 1 && C >= 1 && T_x >= 1 && T_y >= 1, 1, "bad expand shape");
    tts::ExpandArgs a{};
    a.w_ceil = d_w_ceil; a.x_mask = d_x_mask; a.y_len = d_y_lengths; a.o_mean = d_o_mean;
    a.o_log_scale = d_o_log_scale; a.noise = d_noise; a.noise_scale = noise_scale;
    a.C = C; a.T_x = T_x; a.T_y = T_y;
    a.z = d_z; a.y_mask = d_y_mask; a.y_mean = d_y_mean; a.y_log_scale = d_y_log_scale; a.attn = d_attn;
    tts::launch_expand(a, B, static_cast<hipStream_t>(hip_stream));
    TTS_HIP_CHECK(hipGetLastError());
  });
}

int tts_glow_mas_logp(const float* d_o_mean, const float* d_o_log_scale, const float* d_z, int B, int C, int T_en,
                      int T_de, float* d_logp, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_o_mean && d_z && d_logp, 1, "NULL argument");
    TTS_REQUIRE(B >= 1 && C >= 1 && T_en >= 1 && T_de >= 1, 1, "bad logp shape");
    tts::launch_mas_logp(d_o_mean, d_o_log_scale, d_z, B, C, T_en, T_de, d_logp, static_cast<hipStream_t>(hip_stream));
  });
}

int64_t tts_maximum_path_workspace_bytes(int B, int T_en, int T_de) {
  if (B < 1 || T_en < 1 || T_de < 1 || T_en > tts::MAS_MAX_TEN) return -1;
  return (int64_t)tts::mas_workspace_bytes(B, T_en, T_de);
}

int tts_maximum_path(const float* d_value, const float* d_mask, const int64_t* d_t_x, const int64_t* d_t_y, int B,
                     int T_en, int T_de, void* d_workspace, float* d_path, float* d_durations, float* d_log_dur,
                     void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_value && d_t_x && d_t_y && d_workspace, 1, "NULL argument");
    TTS_REQUIRE(B >= 1 && T_en >= 1 && T_de >= 1, 1, "bad maximum_path shape");
    tts::launch_maximum_path(d_value, d_mask, d_t_x, d_t_y, B, T_en, T_de, d_workspace, d_path, d_durations, d_log_dur,
                             static_cast<hipStream_t>(hip_stream));
  });
}

// ----------------------------------------------------------------------------- VITS text side
int tts_vits_text_encoder_num_weights(const TtsVitsTextEncoderCfg* cfg) {
  return num_weights(cfg, tts::vits_text_encoder_validate, tts::vits_text_encoder_weight_shapes);
}

int64_t tts_vits_text_encoder_weight_numel(const TtsVitsTextEncoderCfg* cfg, int idx) {
  return weight_numel(cfg, idx, tts::vits_text_encoder_validate, tts::vits_text_encoder_weight_shapes);
}

int tts_vits_text_encoder_create(const TtsVitsTextEncoderCfg* cfg, const float* const* host_weights, int device,
                                 void** handle) {
  return create<tts::VitsTextEncoder>(cfg, host_weights, device, handle);
}

int tts_vits_text_encoder_destroy(void* handle) { return destroy<tts::VitsTextEncoder>(handle); }

int tts_vits_text_encoder_forward(void* handle, const int64_t* d_tokens, const int64_t* d_lengths,
                                  const float* d_lang_emb, int B, int T, float* d_x, float* d_m, float* d_logs,
                                  float* d_x_mask, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::VitsTextEncoder*>(handle)->forward(d_tokens, d_lengths, d_lang_emb, B, T, d_x, d_m, d_logs,
                                                        d_x_mask, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_vits_text_encoder_forward_profiled(void* handle, const int64_t* d_tokens, const int64_t* d_lengths,
                                           const float* d_lang_emb, int B, int T, float* d_x, float* d_m,
                                           float* d_logs, float* d_x_mask, void* hip_stream,
                                           TtsLaunchRecord* records, int max_records, int* n_records) {
  auto body = [&](tts::VitsTextEncoder& h, hipStream_t s, tts::Profiler* prof) {
    h.forward(d_tokens, d_lengths, d_lang_emb, B, T, d_x, d_m, d_logs, d_x_mask, s, prof);
  };
  return profiled<tts::VitsTextEncoder>(handle, hip_stream, records, max_records, n_records, body);
}

int tts_vits_sdp_num_weights(const TtsVitsSdpCfg* cfg) {
  return num_weights(cfg, tts::vits_sdp_validate, tts::vits_sdp_weight_shapes);
}

int64_t tts_vits_sdp_weight_numel(const TtsVitsSdpCfg* cfg, int idx) {
  return weight_numel(cfg, idx, tts::vits_sdp_validate, tts::vits_sdp_weight_shapes);
}

int tts_vits_sdp_create(const TtsVitsSdpCfg* cfg, const float* const* host_weights, int device, void** handle) {
  return create<tts::VitsSdp>(cfg, host_weights, device, handle);
}

int tts_vits_sdp_destroy(void* handle) { return destroy<tts::VitsSdp>(handle); }

int tts_vits_sdp_reverse(void* handle, const float* d_x, const float* d_x_mask, const float* d_g,
                         const float* d_lang_emb, const float* d_noise, float noise_scale, int B, int T,
                         float* d_logw, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::VitsSdp*>(handle)->reverse(d_x, d_x_mask, d_g, d_lang_emb, d_noise, noise_scale, B, T, d_logw,
                                                static_cast<hipStream_t>(hip_stream));
  });
}

int tts_vits_sdp_reverse_profiled(void* handle, const float* d_x, const float* d_x_mask, const float* d_g,
                                  const float* d_lang_emb, const float* d_noise, float noise_scale, int B, int T,
                                  float* d_logw, void* hip_stream, TtsLaunchRecord* records, int max_records,
                                  int* n_records) {
  auto body = [&](tts::VitsSdp& h, hipStream_t s, tts::Profiler* prof) {
    h.reverse(d_x, d_x_mask, d_g, d_lang_emb, d_noise, noise_scale, B, T, d_logw, s, prof);
  };
  return profiled<tts::VitsSdp>(handle, hip_stream, records, max_records, n_records, body);
}

int tts_vits_dp_num_weights(const TtsVitsDpCfg* cfg) {
  return num_weights(cfg, tts::vits_dp_validate, tts::vits_dp_weight_shapes);
}

int64_t tts_vits_dp_weight_numel(const TtsVitsDpCfg* cfg, int idx) {
  return weight_numel(cfg, idx, tts::vits_dp_validate, tts::vits_dp_weight_shapes);
}

int tts_vits_dp_create(const TtsVitsDpCfg* cfg, const float* const* host_weights, int device, void** handle) {
  return create<tts::VitsDp>(cfg, host_weights, device, handle);
}

int tts_vits_dp_destroy(void* handle) { return destroy<tts::VitsDp>(handle); }

int tts_vits_dp_forward(void* handle, const float* d_x, const float* d_x_mask, const float* d_g,
                        const float* d_lang_emb, int B, int T, float* d_logw, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::VitsDp*>(handle)->forward(d_x, d_x_mask, d_g, d_lang_emb, B, T, d_logw,
                                               static_cast<hipStream_t>(hip_stream));
  });
}

int tts_vits_dp_forward_profiled(void* handle, const float* d_x, const float* d_x_mask, const float* d_g,
                                 const float* d_lang_emb, int B, int T, float* d_logw, void* hip_stream,
                                 TtsLaunchRecord* records, int max_records, int* n_records) {
  auto body = [&](tts::VitsDp& h, hipStream_t s, tts::Profiler* prof) {
    h.forward(d_x, d_x_mask, d_g, d_lang_emb, B, T, d_logw, s, prof);
  };
  return profiled<tts::VitsDp>(handle, hip_stream, records, max_records, n_records, body);
}

int tts_vits_durations(const float* d_logw, const float* d_x_mask, int B, int T_x, float length_scale,
                       float* d_w_ceil, int64_t* d_y_lengths, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_logw && d_x_mask && d_w_ceil && d_y_lengths, 1, "NULL argument");
    TTS_REQUIRE(B >= 1 && T_x >= 1, 1, "batch and token count must be >= 1");
    tts::launch_durations(d_logw, d_x_mask, d_w_ceil, d_y_lengths, nullptr, B, T_x, length_scale,
                          static_cast<hipStream_t>(hip_stream), 1);
    TTS_HIP_CHECK(hipGetLastError());
  });
}

int tts_vits_expand(const float* d_w_ceil, const float* d_x_mask, const int64_t* d_y_lengths, const float* d_m_p,
                    const float* d_logs_p, const float* d_noise, float noise_scale, int B, int C, int T_x, int T_y,
                    float* d_z_p, float* d_y_mask, float* d_m_p_out, float* d_logs_p_out, float* d_attn,
                    void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_w_ceil && d_x_mask && d_y_lengths && d_m_p && d_logs_p && d_z_p && d_y_mask, 1, "NULL argument");
    TTS_REQUIRE(B >= 1 && C >= 1 && T_x >= 1 && T_y >= 1, 1, "bad expand shape");
    tts::ExpandArgs a{};
    a.w_ceil = d_w_ceil; a.x_mask = d_x_mask; a.y_len = d_y_lengths; a.o_mean = d_m_p;
    a.o_log_scale = d_logs_p; a.noise = d_noise; a.noise_scale = noise_scale;
    a.C = C; a.T_x = T_x; a.T_y = T_y;
    a.z = d_z_p; a.y_mask = d_y_mask; a.y_mean = d_m_p_out; a.y_log_scale = d_logs_p_out; a.attn = d_attn;
    a.vits = 1;
    tts::launch_expand(a, B, static_cast<hipStream_t>(hip_stream));
    TTS_HIP_CHECK(hipGetLastError());
  });
}

int tts_vits_durations_given(const float* d_durations, int64_t dur_bstride, int B, int T_x, float* d_w_ceil,
                             int64_t* d_y_lengths, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_durations && d_w_ceil && d_y_lengths, 1, "NULL argument");
    TTS_REQUIRE(B >= 1 && T_x >= 1 && (dur_bstride == 0 || dur_bstride >= T_x), 1, "bad durations shape");
    tts::launch_given_durations(d_durations, dur_bstride, d_w_ceil, d_y_lengths, B, T_x,
                                static_cast<hipStream_t>(hip_stream));
  });
}

int tts_vits_mask_slice(const float* d_z, const float* d_y_mask, int B, int C, int T, int T_out, float* d_out,
                        void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_z && d_y_mask && d_out, 1, "NULL argument");
    tts::launch_mask_slice(d_z, d_y_mask, d_out, B, C, T, T_out, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_vits_upsample_z(const float* d_z, const int64_t* d_y_lengths, int B, int C, int T, double factor, int T2,
                        float* d_z2, float* d_y_mask2, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_z && d_z2 && (d_y_lengths || !d_y_mask2), 1, "NULL argument");
    TTS_REQUIRE(factor > 0.0 && T2 == (int)std::floor((double)T * factor), 1,
                "upsample_z: T2 must be floor(T * factor) (F.interpolate's output length)");
    tts::launch_upsample_z(d_z, d_y_lengths, d_z2, d_y_mask2, B, C, T, T2, factor,
                           static_cast<hipStream_t>(hip_stream));
  });
}

int tts_embedding_rows(const float* d_table, int num, int dim, const int64_t* d_ids, int64_t id_stride, int B,
                       float* d_out, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_table && d_ids && d_out, 1, "NULL argument");
    tts::launch_embedding_rows(d_table, d_ids, id_stride, d_out, B, dim, num, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_l2_normalize_rows(const float* d_in, int B, int C, float* d_out, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_in && d_out, 1, "NULL argument");
    tts::launch_l2_normalize(d_in, d_out, B, C, static_cast<hipStream_t>(hip_stream));
  });
}

// ----------------------------------------------------------------------------- hand-off / wav writer
namespace {
tts::AudioNormDev to_dev(const TtsAudioNormCfg* c) {
  tts::AudioNormDev d{};
  if (!c || !c->signal_norm) return d;  // signal_norm = 0: identity
  TTS_REQUIRE((c->d_mel_mean == nullptr) == (c->d_mel_scale == nullptr), 1,
              "mel_scaler needs both d_mel_mean and d_mel_scale");
  d.signal_norm = 1;
  d.symmetric_norm = c->symmetric_norm;
  d.clip_norm = c->clip_norm;
  d.max_norm = (float)c->max_norm;
  d.two_max_norm = (float)(2.0 * c->max_norm);       // (2 * self.max_norm) in Python
  d.min_level_db = (float)c->min_level_db;
  d.neg_min_level_db = (float)(-c->min_level_db);   // -self.min_level_db in Python
  d.ref_level_db = (float)c->ref_level_db;
  d.mean = c->d_mel_mean;
  d.scale = c->d_mel_scale;
  return d;
}
}  // namespace

int tts_mel_handoff(const float* d_in, int B, int T, int C, int time_major, const TtsAudioNormCfg* denorm,
                    const TtsAudioNormCfg* norm, int T_out, float src_scale, float* d_out, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_in && d_out, 1, "NULL argument");
    TTS_REQUIRE(B >= 1 && T >= 1 && C >= 1 && T_out >= 1, 1, "bad hand-off shape");
    TTS_REQUIRE(C <= 65535 && B <= 65535, 3, "hand-off: C and B must be <= 65535");
    tts::HandoffArgs a{};
    a.in = d_in; a.out = d_out; a.T = T; a.C = C; a.T_out = T_out; a.time_major = time_major ? 1 : 0;
    a.src_scale = src_scale;
    a.de = to_dev(denorm);
    a.no = to_dev(norm);
    tts::launch_handoff(a, B, static_cast<hipStream_t>(hip_stream));
    TTS_HIP_CHECK(hipGetLastError());
  });
}

int tts_wav_to_int16(const float* d_wav, int B, int64_t n, const int64_t* d_lengths, unsigned* d_scratch,
                     int16_t* d_out, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_wav && d_scratch && d_out, 1, "NULL argument");
    TTS_REQUIRE(B >= 1 && B <= 65535 && n >= 1, 1, "bad wav shape");
    tts::launch_wav_int16(d_wav, B, n, d_lengths, d_scratch, d_out, static_cast<hipStream_t>(hip_stream));
    TTS_HIP_CHECK(hipGetLastError());
  });
}

// ----------------------------------------------------------------------------- Glow decoder
int tts_glow_decoder_num_weights(const TtsGlowDecoderCfg* cfg) {
  return num_weights(cfg, tts::glow_validate, tts::glow_weight_shapes);
}

int64_t tts_glow_decoder_weight_numel(const TtsGlowDecoderCfg* cfg, int idx) {
  return weight_numel(cfg, idx, tts::glow_validate, tts::glow_weight_shapes);
}

int tts_glow_decoder_create(const TtsGlowDecoderCfg* cfg, const float* const* host_weights,
                            int device, void** handle) {
  return create<tts::GlowDecoder>(cfg, host_weights, device, handle);
}

int tts_glow_decoder_destroy(void* handle) { return destroy<tts::GlowDecoder>(handle); }

int tts_glow_decoder_forward(void* handle, const float* d_x, const float* d_mask, const float* d_g, int B,
                             int C, int T, int reverse, float* d_y, float* d_logdet, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    TTS_REQUIRE(reverse == 0 || reverse == 1, 1, "reverse must be 0 or 1");
    auto* h = static_cast<tts::GlowDecoder*>(handle);
    if (reverse) h->reverse(d_x, d_mask, d_g, B, C, T, d_y, static_cast<hipStream_t>(hip_stream));
    else h->forward(d_x, d_mask, d_g, B, C, T, d_y, d_logdet, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_glow_decoder_forward_profiled(void* handle, const float* d_x, const float* d_mask, const float* d_g,
                                      int B, int C, int T, int reverse, float* d_y, float* d_logdet,
                                      void* hip_stream, TtsLaunchRecord* records, int max_records, int* n_records) {
  auto body = [&](tts::GlowDecoder& h, hipStream_t s, tts::Profiler* prof) {
    TTS_REQUIRE(reverse == 0 || reverse == 1, 1, "reverse must be 0 or 1");
    if (reverse) h.reverse(d_x, d_mask, d_g, B, C, T, d_y, s, prof);
    else h.forward(d_x, d_mask, d_g, B, C, T, d_y, d_logdet, s, prof);
  };
  return profiled<tts::GlowDecoder>(handle, hip_stream, records, max_records, n_records, body);
}

// ----------------------------------------------------------------------------- VITS flow
int tts_vits_flow_num_weights(const TtsVitsFlowCfg* cfg) {
  return num_weights(cfg, tts::vits_flow_validate, tts::vits_flow_weight_shapes);
}

int64_t tts_vits_flow_weight_numel(const TtsVitsFlowCfg* cfg, int idx) {
  return weight_numel(cfg, idx, tts::vits_flow_validate, tts::vits_flow_weight_shapes);
}

int tts_vits_flow_create(const TtsVitsFlowCfg* cfg, const float* const* host_weights, int device, void** handle) {
  return create<tts::VitsFlow>(cfg, host_weights, device, handle);
}

int tts_vits_flow_destroy(void* handle) { return destroy<tts::VitsFlow>(handle); }

int tts_vits_flow_forward(void* handle, const float* d_x, const float* d_mask, const float* d_g, int B, int C,
                          int T, int reverse, float* d_y, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    TTS_REQUIRE(reverse == 0 || reverse == 1, 1, "reverse must be 0 or 1");
    auto* h = static_cast<tts::VitsFlow*>(handle);
    if (reverse) h->reverse(d_x, d_mask, d_g, B, C, T, d_y, static_cast<hipStream_t>(hip_stream));
    else h->forward(d_x, d_mask, d_g, B, C, T, d_y, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_vits_flow_forward_profiled(void* handle, const float* d_x, const float* d_mask, const float* d_g, int B,
                                   int C, int T, int reverse, float* d_y, void* hip_stream,
                                   TtsLaunchRecord* records, int max_records, int* n_records) {
  auto body = [&](tts::VitsFlow& h, hipStream_t s, tts::Profiler* prof) {
    TTS_REQUIRE(reverse == 0 || reverse == 1, 1, "reverse must be 0 or 1");
    if (reverse) h.reverse(d_x, d_mask, d_g, B, C, T, d_y, s, prof);
    else h.forward(d_x, d_mask, d_g, B, C, T, d_y, s, prof);
  };
  return profiled<tts::VitsFlow>(handle, hip_stream, records, max_records, n_records, body);
}

// ----------------------------------------------------------------------------- VITS posterior encoder
int tts_vits_posterior_num_weights(const TtsVitsPosteriorCfg* cfg) {
  return num_weights(cfg, tts::vits_posterior_validate, tts::vits_posterior_weight_shapes);
}

int64_t tts_vits_posterior_weight_numel(const TtsVitsPosteriorCfg* cfg, int idx) {
  return weight_numel(cfg, idx, tts::vits_posterior_validate, tts::vits_posterior_weight_shapes);
}

int tts_vits_posterior_create(const TtsVitsPosteriorCfg* cfg, const float* const* host_weights, int device,
                              void** handle) {
  return create<tts::VitsPosterior>(cfg, host_weights, device, handle);
}

int tts_vits_posterior_destroy(void* handle) { return destroy<tts::VitsPosterior>(handle); }

int tts_vits_posterior_forward(void* handle, const float* d_x, const float* d_mask, const float* d_g,
                               const float* d_eps, int B, int C, int T, float* d_z, float* d_m, float* d_logs,
                               void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::VitsPosterior*>(handle)->forward(d_x, d_mask, d_g, d_eps, B, C, T, d_z, d_m, d_logs,
                                                      static_cast<hipStream_t>(hip_stream));
  });
}

int tts_vits_posterior_forward_profiled(void* handle, const float* d_x, const float* d_mask, const float* d_g,
                                        const float* d_eps, int B, int C, int T, float* d_z, float* d_m,
                                        float* d_logs, void* hip_stream, TtsLaunchRecord* records,
                                        int max_records, int* n_records) {
  auto body = [&](tts::VitsPosterior& h, hipStream_t s, tts::Profiler* prof) {
    h.forward(d_x, d_mask, d_g, d_eps, B, C, T, d_z, d_m, d_logs, s, prof);
  };
  return profiled<tts::VitsPosterior>(handle, hip_stream, records, max_records, n_records, body);
}

// ----------------------------------------------------------------------------- linear spectrogram
int tts_stft_create(const TtsStftCfg* cfg, const float* h_window, int device, void** handle) {
  return create<tts::Stft>(cfg, h_window, device, handle);
}

int tts_stft_destroy(void* handle) { return destroy<tts::Stft>(handle); }

int tts_stft_num_frames(const TtsStftCfg* cfg, int64_t N) {
  int n = -1;
  int st = guarded([&] {
    TTS_REQUIRE(cfg, 1, "NULL cfg");
    n = tts::stft_num_frames(*cfg, N);
  });
  return st == TTS_OK ? n : -st;
}

int tts_stft_forward(void* handle, const float* d_wav, int B, int64_t N, int64_t wav_bstride, float* d_spec,
                     void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::Stft*>(handle)->forward(d_wav, B, N, wav_bstride, d_spec, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_stft_forward_profiled(void* handle, const float* d_wav, int B, int64_t N, int64_t wav_bstride,
                              float* d_spec, void* hip_stream, TtsLaunchRecord* records, int max_records,
                              int* n_records) {
  auto body = [&](tts::Stft& h, hipStream_t s, tts::Profiler* prof) {
    h.forward(d_wav, B, N, wav_bstride, d_spec, s, prof);
  };
  return profiled<tts::Stft>(handle, hip_stream, records, max_records, n_records, body);
}

// ----------------------------------------------------------------------------- single ops
static void op_conv1d_impl(const TtsConv1dDesc* d, const float* d_x, const float* h_w, const float* h_b,
                           const float* d_res, float* d_y, float* d_z, int tile, int reps, float* ms,
                           void* hip_stream, const float* d_cvec = nullptr) {
  TTS_REQUIRE(d && d_x && h_w && h_b, 1, "NULL argument");
  TTS_REQUIRE(d->B >= 1 && d->Cin >= 1 && d->Cout >= 1 && d->Tin >= 1 && d->K >= 1 && d->dil >= 1, 1,
              "bad conv1d shape");
  TTS_REQUIRE((d->K % 2) == 1, 3, "conv1d: only odd kernel sizes ('same' padding)");
  TTS_REQUIRE(d->zmode >= 0 && d->zmode <= 3, 1, "bad zmode");
  TTS_REQUIRE(d->zmode == 0 ? d_y != nullptr : d_z != nullptr, 1, "missing output pointer");
  const int mode = d->math_mode;
  TTS_REQUIRE(mode >= tts::MATH_FP32 && mode <= tts::MATH_LAST, 1, "unknown math_mode");
  if (tile < 0) tile = tts::conv_tile_for(mode, d->Cout, d->K, d->Cin, d->dil, d_res != nullptr);
  const tts::ConvTile t = tts::conv_tile(mode, tile);
  std::vector<float> packed(tts::packed_conv_numel(mode, d->Cout, d->Cin, d->K, t));
  const int w_exp = tts::pack_conv(mode, h_w, d->Cout, d->Cin, d->K, t, packed.data());
  std::vector<float> bias((size_t)tts::ceil_div(d->Cout, t.BM) * t.BM, 0.f);
  std::memcpy(bias.data(), h_b, sizeof(float) * d->Cout);
  const tts::DeviceBuffer w = to_device(packed.data(), packed.size()), b = to_device(bias.data(), bias.size());
  tts::Conv1dArgs a{};
  a.x = d_x; a.w = w.as<>(); a.bias = b.as<>(); a.res = d_res; a.y = d_y; a.z = d_z; a.cvec = d_cvec;
  a.Cin = d->Cin; a.Cout = d->Cout; a.Tin = d->Tin; a.Tout = d->Tin + 2 * d->rep_pad;
  a.dil = d->dil; a.pad = d->dil * (d->K - 1) / 2; a.rep_pad = d->rep_pad;
  a.n_chunks = tts::ceil_div(d->Cin, t.CK);
  a.in_slope = d->in_slope; a.out_slope = d->out_slope; a.zmode = d->zmode; a.zdiv = d->zdiv;
  a.w_exp = w_exp;
  auto s = static_cast<hipStream_t>(hip_stream);
  // fp16 hi/lo mode: the input's max-abs statistic (the executors get it from the producer)
  tts::DeviceBuffer slots;
  if (mode == tts::MATH_FP32_F16X3) {
    slots = to_device(nullptr, (size_t)d->B * 64);
    TTS_HIP_CHECK(hipMemsetAsync(slots.as<>(), 0, (size_t)d->B * 64 * sizeof(float), s));
    tts::launch_amax(d_x, (int64_t)d->Cin * d->Tin, d->B, slots.as<unsigned>(), s);
    a.amax_in = slots.as<unsigned>();
  }
  if (reps <= 0) {
    tts::launch_conv(mode, a, d->B, d->K, tile, s);
  } else {
    tts::launch_conv(mode, a, d->B, d->K, tile, s);  // warm-up
    hipEvent_t e0, e1;
    TTS_HIP_CHECK(hipEventCreate(&e0));
    TTS_HIP_CHECK(hipEventCreate(&e1));
    TTS_HIP_CHECK(hipEventRecord(e0, s));
    for (int r = 0; r < reps; ++r) tts::launch_conv(mode, a, d->B, d->K, tile, s);
    TTS_HIP_CHECK(hipEventRecord(e1, s));
    TTS_HIP_CHECK(hipEventSynchronize(e1));
    float total = 0.f;
    TTS_HIP_CHECK(hipEventElapsedTime(&total, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (ms) *ms = total / reps;
  }
  TTS_HIP_CHECK(hipStreamSynchronize(s));
}

int tts_op_conv1d(const TtsConv1dDesc* d, const float* d_x, const float* h_w, const float* h_b,
                  const float* d_res, float* d_y, float* d_z, void* hip_stream) {
  return guarded([&] { op_conv1d_impl(d, d_x, h_w, h_b, d_res, d_y, d_z, -1, 0, nullptr, hip_stream); });
}

int tts_op_conv1d_bench(const TtsConv1dDesc* d, const float* d_x, const float* h_w, const float* h_b,
                        const float* d_res, float* d_y, float* d_z, int tile, int reps, float* ms,
                        void* hip_stream) {
  return guarded([&] { op_conv1d_impl(d, d_x, h_w, h_b, d_res, d_y, d_z, tile, reps, ms, hip_stream); });
}

int tts_op_conv1d_cvec(const TtsConv1dDesc* d, const float* d_x, const float* h_w, const float* h_b,
                       const float* d_cvec, const float* d_res, float* d_y, float* d_z, int tile,
                       void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_cvec, 1, "NULL cvec");
    op_conv1d_impl(d, d_x, h_w, h_b, d_res, d_y, d_z, tile, 0, nullptr, hip_stream, d_cvec);
  });
}

int tts_op_conv1d_num_tiles(int math_mode) {
  if (math_mode < tts::MATH_FP32 || math_mode > tts::MATH_LAST) {
    g_last_error = "unknown math_mode";
    return -TTS_ERR_INVALID;
  }
  return tts::conv_num_tiles(math_mode);
}

int tts_op_conv_transpose1d(const float* d_x, int B, int Cin, int Tin, const float* h_w,
                            const float* h_b, int Cout, int K, int stride, float in_slope,
                            int math_mode, float* d_y, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_x && h_w && h_b && d_y, 1, "NULL argument");
    TTS_REQUIRE(B >= 1 && Cin >= 1 && Cout >= 1 && Tin >= 1, 1, "bad conv_transpose1d shape");
    TTS_REQUIRE(K == 2 * stride, 3, "conv_transpose1d: requires kernel_size == 2*stride");
    TTS_REQUIRE(stride == 2 || stride == 4 || stride == 8, 3, "conv_transpose1d: stride must be 2, 4 or 8");
    TTS_REQUIRE(math_mode >= tts::MATH_FP32 && math_mode <= tts::MATH_LAST, 1, "unknown math_mode");
    auto s = static_cast<hipStream_t>(hip_stream);
    if (tts::is_split_mode(math_mode)) {
      const int tile = tts::conv_tile_for(math_mode, stride * Cout, 2, Cin, 1, false);
      const tts::ConvTile t = tts::conv_tile(math_mode, tile);
      std::vector<float> packed(tts::packed_conv_numel(math_mode, stride * Cout, Cin, 2, t));
      const int w_exp = tts::pack_convT_split(math_mode, h_w, Cin, Cout, stride, t, packed.data());
      std::vector<float> bias((size_t)tts::ceil_div(stride * Cout, t.BM) * t.BM, 0.f);
      for (int co = 0; co < Cout; ++co)
        for (int ph = 0; ph < stride; ++ph) bias[(size_t)co * stride + ph] = h_b[co];
      const tts::DeviceBuffer w = to_device(packed.data(), packed.size()), b = to_device(bias.data(), bias.size());
      tts::Conv1dArgs a{};
      a.x = d_x; a.w = w.as<>(); a.bias = b.as<>(); a.y = d_y;
      a.Cin = Cin; a.Cout = stride * Cout; a.Tin = Tin; a.Tout = Tin + 1;
      a.dil = 1; a.pad = 1; a.n_chunks = tts::ceil_div(Cin, t.CK);
      a.in_slope = in_slope; a.out_slope = 1.f; a.zdiv = 1.f; a.w_exp = w_exp; a.ups = stride;
      tts::DeviceBuffer slots;
      if (math_mode == tts::MATH_FP32_F16X3) {
        slots = to_device(nullptr, (size_t)B * 64);
        TTS_HIP_CHECK(hipMemsetAsync(slots.as<>(), 0, (size_t)B * 64 * sizeof(float), s));
        tts::launch_amax(d_x, (int64_t)Cin * Tin, B, slots.as<unsigned>(), s);
        a.amax_in = slots.as<unsigned>();
      }
      tts::launch_conv(math_mode, a, B, 2, tile, s);
      TTS_HIP_CHECK(hipStreamSynchronize(s));
      return;
    }
    const int tile = tts::convT_tile_for(Cout, stride);
    const tts::ConvTile t = tts::convT_tile(tile, stride);
    std::vector<float> packed(tts::packed_convT_numel(Cin, Cout, stride, t));
    tts::pack_convT(h_w, Cin, Cout, stride, t, packed.data());
    std::vector<float> bias((size_t)tts::ceil_div(Cout, t.BM) * t.BM, 0.f);
    std::memcpy(bias.data(), h_b, sizeof(float) * Cout);
    const tts::DeviceBuffer w = to_device(packed.data(), packed.size()), b = to_device(bias.data(), bias.size());
    tts::ConvTArgs a{};
    a.x = d_x; a.w = w.as<>(); a.bias = b.as<>(); a.y = d_y;
    a.Cin = Cin; a.Cout = Cout; a.Tin = Tin; a.n_chunks = tts::ceil_div(Cin, t.CK); a.in_slope = in_slope;
    tts::launch_convT(a, B, stride, tile, s);
    TTS_HIP_CHECK(hipStreamSynchronize(s));
  });
}

int tts_op_conv_post(const float* d_z, int B, int Cin, int T, const float* h_w, const float* h_b,
                     float in_slope, float* d_y, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_z && h_w && d_y, 1, "NULL argument");
    TTS_REQUIRE(B >= 1 && Cin >= 1 && T >= 1, 1, "bad conv_post shape");
    const tts::DeviceBuffer w = to_device(h_w, (size_t)Cin * 7);
    tts::PostArgs a{};
    a.z = d_z; a.w = w.as<>(); a.bias = h_b ? h_b[0] : 0.f; a.y = d_y; a.Cin = Cin; a.T = T; a.in_slope = in_slope;
    auto s = static_cast<hipStream_t>(hip_stream);
    tts::launch_conv_post(a, B, s);
    TTS_HIP_CHECK(hipStreamSynchronize(s));
  });
}

// ----------------------------------------------------------------------------- MelGAN family
int tts_melgan_num_weights(const TtsMelganCfg* cfg) {
  return num_weights(cfg, [](const TtsMelganCfg&) {}, tts::melgan_weight_shapes);
}

int64_t tts_melgan_weight_numel(const TtsMelganCfg* cfg, int idx) {
  return weight_numel(cfg, idx, [](const TtsMelganCfg&) {}, tts::melgan_weight_shapes);
}

int tts_melgan_create(const TtsMelganCfg* cfg, const float* const* host_weights, int device, void** handle) {
  return create<tts::Melgan>(cfg, host_weights, device, handle);
}

int tts_melgan_destroy(void* handle) { return destroy<tts::Melgan>(handle); }

int64_t tts_melgan_output_length(const void* handle, int T, int pad, int synth) {
  int64_t n = -1;
  int st = guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    n = static_cast<const tts::Melgan*>(handle)->out_len(T, pad, synth);
  });
  return st == TTS_OK ? n : -st;
}

int64_t tts_melgan_workspace_bytes(const void* handle, int B, int T, int pad) {
  int64_t n = -1;
  int st = guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    n = static_cast<const tts::Melgan*>(handle)->workspace_bytes(B, T, pad);
  });
  return st == TTS_OK ? n : -st;
}

int tts_melgan_forward(void* handle, const float* d_mel, int B, int C, int T, int pad, int synth, float* d_out,
                       void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::Melgan*>(handle)->forward(d_mel, B, C, T, pad, synth, d_out, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_melgan_forward_profiled(void* handle, const float* d_mel, int B, int C, int T, int pad, int synth,
                                float* d_out, void* hip_stream, TtsLaunchRecord* records, int max_records,
                                int* n_records) {
  auto body = [&](tts::Melgan& h, hipStream_t s, tts::Profiler* prof) {
    h.forward(d_mel, B, C, T, pad, synth, d_out, s, prof);
  };
  return profiled<tts::Melgan>(handle, hip_stream, records, max_records, n_records, body);
}

int tts_op_melgan_block(const float* d_x, int B, int C, int L, int dilation, const float* h_w1, const float* h_b1,
                        const float* h_w2, const float* h_b2, const float* h_ws, const float* h_bs, int math_mode,
                        float* d_out, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_x && h_w1 && h_b1 && h_w2 && h_b2 && h_ws && h_bs && d_out, 1, "NULL argument");
    TTS_REQUIRE(math_mode >= tts::MATH_FP32 && math_mode <= tts::MATH_LAST, 1, "unknown math_mode");
    TTS_REQUIRE(B >= 1 && C >= 1 && L >= 1 && dilation >= 1, 1, "bad melgan block shape");
    const int mode = math_mode == tts::MATH_BF16 ? tts::MATH_BF16 : tts::MATH_FP32_X6;
    TTS_REQUIRE(C <= tts::kMelganMaxC, 3, "melgan block: channels must lie in [1, 256]");
    const int64_t n1 = tts::packed_melgan_a1_numel16(mode, C), n2 = tts::packed_melgan_a2_numel16(mode, C);
    const size_t nb = (size_t)32 * tts::melgan_mblocks(C);
    std::vector<float> a1((size_t)n1 / 2), a2((size_t)n2 / 2), bias1(nb), bias2(nb);
    tts::pack_melgan_block(mode, h_w1, h_b1, h_w2, h_b2, h_ws, h_bs, C, reinterpret_cast<uint16_t*>(a1.data()),
                           reinterpret_cast<uint16_t*>(a2.data()), bias1.data(), bias2.data());
    const tts::DeviceBuffer da1 = to_device(a1.data(), a1.size()), da2 = to_device(a2.data(), a2.size());
    const tts::DeviceBuffer db1 = to_device(bias1.data(), nb), db2 = to_device(bias2.data(), nb);
    tts::MelganBlockArgs a{};
    a.x = d_x; a.y = d_out; a.a1 = da1.as<>(); a.a2 = da2.as<>(); a.bias1 = db1.as<>(); a.bias2 = db2.as<>();
    a.a1_bytes = (unsigned)(n1 * 2); a.a2_bytes = (unsigned)(n2 * 2);
    a.C = C; a.L = L; a.dil = dilation;
    auto s = static_cast<hipStream_t>(hip_stream);
    tts::launch_melgan_block(mode, a, B, s);
    TTS_HIP_CHECK(hipStreamSynchronize(s));
  });
}

int tts_op_melgan_block_tile(void) { return tts::kMelganBlockTile; }

int tts_pqmf_synthesis(const float* d_x, int B, int bands, int L, const float* d_G, int taps, float* d_out,
                       void* hip_stream) {
  return guarded([&] {
    tts::launch_pqmf_synthesis(d_x, B, bands, L, d_G, taps, d_out, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_op_mha(const float* d_qkv, const int64_t* d_key_lengths, int B, int E, int heads, int T, int math_mode,
               float* d_out, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_qkv && d_out, 1, "NULL argument");
    TTS_REQUIRE(math_mode >= tts::MATH_FP32 && math_mode <= tts::MATH_LAST, 1, "unknown math_mode");
    const int mode = math_mode == tts::MATH_BF16 ? tts::MATH_BF16 : tts::MATH_FP32_X6;
    tts::launch_mha(mode, d_qkv, d_key_lengths, d_out, B, E, heads, T, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_op_mha_tile(void) { return tts::kMhaTile; }

int tts_forward_tts_num_weights(const TtsForwardTtsCfg* cfg) {
  return num_weights(cfg, tts::forward_tts_validate, tts::forward_tts_weight_shapes);
}

int64_t tts_forward_tts_weight_numel(const TtsForwardTtsCfg* cfg, int idx) {
  return weight_numel(cfg, idx, tts::forward_tts_validate, tts::forward_tts_weight_shapes);
}

int tts_forward_tts_create(const TtsForwardTtsCfg* cfg, const float* const* host_weights, int device, void** handle) {
  return create<tts::ForwardTts>(cfg, host_weights, device, handle);
}

int tts_forward_tts_destroy(void* handle) { return destroy<tts::ForwardTts>(handle); }

int tts_forward_tts_encode(void* handle, const int64_t* d_tokens, const int64_t* d_x_lengths,
                           const int64_t* d_speaker_ids, const float* d_given_durations, int B, int T_en,
                           float length_scale, float* d_o_en, float* d_x_mask, float* d_durations_log, float* d_pitch,
                           float* d_durations, int64_t* d_y_lengths, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::ForwardTts*>(handle)->encode(d_tokens, d_x_lengths, d_speaker_ids, d_given_durations, B, T_en,
                                                  length_scale, d_o_en, d_x_mask, d_durations_log, d_pitch,
                                                  d_durations, d_y_lengths, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_forward_tts_encode_profiled(void* handle, const int64_t* d_tokens, const int64_t* d_x_lengths,
                                    const int64_t* d_speaker_ids, const float* d_given_durations, int B, int T_en,
                                    float length_scale, float* d_o_en, float* d_x_mask, float* d_durations_log,
                                    float* d_pitch, float* d_durations, int64_t* d_y_lengths, void* hip_stream,
                                    TtsLaunchRecord* records, int max_records, int* n_records) {
  auto body = [&](tts::ForwardTts& h, hipStream_t s, tts::Profiler* prof) {
    h.encode(d_tokens, d_x_lengths, d_speaker_ids, d_given_durations, B, T_en, length_scale, d_o_en, d_x_mask,
             d_durations_log, d_pitch, d_durations, d_y_lengths, s, prof);
  };
  return profiled<tts::ForwardTts>(handle, hip_stream, records, max_records, n_records, body);
}

int tts_forward_tts_decode(void* handle, const float* d_o_en, const float* d_durations, const float* d_x_mask,
                           const int64_t* d_y_lengths, int B, int T_en, int T_de, int mask_decoder_keys, float* d_out,
                           float* d_attn, float* d_y_mask, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::ForwardTts*>(handle)->decode(d_o_en, d_durations, d_x_mask, d_y_lengths, B, T_en, T_de,
                                                  mask_decoder_keys != 0, d_out, d_attn, d_y_mask,
                                                  static_cast<hipStream_t>(hip_stream));
  });
}

int tts_forward_tts_decode_profiled(void* handle, const float* d_o_en, const float* d_durations, const float* d_x_mask,
                                    const int64_t* d_y_lengths, int B, int T_en, int T_de, int mask_decoder_keys,
                                    float* d_out, float* d_attn, float* d_y_mask, void* hip_stream,
                                    TtsLaunchRecord* records, int max_records, int* n_records) {
  auto body = [&](tts::ForwardTts& h, hipStream_t s, tts::Profiler* prof) {
    h.decode(d_o_en, d_durations, d_x_mask, d_y_lengths, B, T_en, T_de, mask_decoder_keys != 0, d_out, d_attn,
             d_y_mask, s, prof);
  };
  return profiled<tts::ForwardTts>(handle, hip_stream, records, max_records, n_records, body);
}

int tts_forward_tts_block(void* handle, int decoder, const float* d_x, const int64_t* d_key_lengths, int B, int T,
                          float* d_y, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::ForwardTts*>(handle)->block(decoder != 0, d_x, d_key_lengths, B, T, d_y,
                                                 static_cast<hipStream_t>(hip_stream));
  });
}

// ----------------------------------------------------------------------------- Tacotron2
int tts_tacotron2_num_weights(const TtsTacotron2Cfg* cfg) {
  return num_weights(cfg, tts::tacotron2_validate, tts::tacotron2_weight_shapes);
}

int64_t tts_tacotron2_weight_numel(const TtsTacotron2Cfg* cfg, int idx) {
  return weight_numel(cfg, idx, tts::tacotron2_validate, tts::tacotron2_weight_shapes);
}

int tts_tacotron2_create(const TtsTacotron2Cfg* cfg, const float* const* host_weights, int device, void** handle) {
  return create<tts::Tacotron2>(cfg, host_weights, device, handle);
}

int tts_tacotron2_destroy(void* handle) { return destroy<tts::Tacotron2>(handle); }

int tts_tacotron2_encode(void* handle, const int64_t* d_tokens, const int64_t* d_x_lengths,
                         const int64_t* d_speaker_ids, const float* d_d_vectors, int B, int T_en, float* d_inputs,
                         float* d_processed_inputs, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::Tacotron2*>(handle)->encode(d_tokens, d_x_lengths, d_speaker_ids, d_d_vectors, B, T_en, d_inputs,
                                                 d_processed_inputs, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_tacotron2_decode(void* handle, const float* d_inputs, const float* d_processed_inputs,
                         const int64_t* d_x_lengths, int B, int T_en, int max_decoder_steps, float stop_threshold,
                         float* d_decoder_outputs, float* d_alignments, float* d_stop_tokens, int32_t* d_steps,
                         int* steps_run, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    const int n = static_cast<tts::Tacotron2*>(handle)->decode(
        d_inputs, d_processed_inputs, d_x_lengths, B, T_en, max_decoder_steps, stop_threshold, d_decoder_outputs,
        d_alignments, d_stop_tokens, d_steps, static_cast<hipStream_t>(hip_stream));
    if (steps_run) *steps_run = n;
  });
}

int tts_tacotron2_decode_profiled(void* handle, const float* d_inputs, const float* d_processed_inputs,
                                  const int64_t* d_x_lengths, int B, int T_en, int max_decoder_steps,
                                  float stop_threshold, float* d_decoder_outputs, float* d_alignments,
                                  float* d_stop_tokens, int32_t* d_steps, int* steps_run, void* hip_stream,
                                  TtsLaunchRecord* records, int max_records, int* n_records) {
  auto body = [&](tts::Tacotron2& h, hipStream_t s, tts::Profiler* prof) {
    const int n = h.decode(d_inputs, d_processed_inputs, d_x_lengths, B, T_en, max_decoder_steps, stop_threshold,
                           d_decoder_outputs, d_alignments, d_stop_tokens, d_steps, s, prof);
    if (steps_run) *steps_run = n;
  };
  return profiled<tts::Tacotron2>(handle, hip_stream, records, max_records, n_records, body);
}

int tts_tacotron2_postnet(void* handle, const float* d_decoder_outputs, const int32_t* d_steps, int B, int steps,
                          int row_stride, float* d_model_outputs, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::Tacotron2*>(handle)->postnet(d_decoder_outputs, d_steps, B, steps, row_stride, d_model_outputs,
                                                  static_cast<hipStream_t>(hip_stream));
  });
}

int tts_op_lstm_cell(const float* d_x, const float* d_h, const float* d_c, int B, int I, int H, const float* h_w_ih,
                     const float* h_w_hh, const float* h_b_ih, const float* h_b_hh, int math_mode, float* d_h_out,
                     float* d_c_out, void* hip_stream) {
  return guarded([&] {
    tts::op_lstm_cell(d_x, d_h, d_c, B, I, H, h_w_ih, h_w_hh, h_b_ih, h_b_hh, math_mode, d_h_out, d_c_out,
                      static_cast<hipStream_t>(hip_stream));
  });
}

int tts_op_conv2d_3x3(const float* d_x, int B, int Cin, int F, int T, const float* h_w, int Cout, int ksize,
                      int stride, const float* h_bias, int relu, const float* h_scale, const float* h_shift,
                      int math_mode, float* d_out, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_x && h_w && d_out, 1, "NULL argument");
    TTS_REQUIRE(math_mode >= tts::MATH_FP32 && math_mode <= tts::MATH_LAST, 1, "unknown math_mode");
    const int mode = tts::conv2d_mode(math_mode);
    tts::Conv2dArgs a{};
    a.x = d_x; a.y = d_out;
    a.Cin = Cin; a.Cout = Cout; a.F = F; a.T = T; a.KS = ksize; a.stride = stride; a.relu = relu != 0;
    tts::conv2d_check(a, B);  // every limit, before anything is packed or launched
    const int64_t n16 = tts::packed_conv2d_numel16(mode, Cout, Cin, ksize);
    const size_t nb = (size_t)32 * tts::conv2d_mblocks(Cout);
    std::vector<float> pa((size_t)n16 / 2), bias(nb), scale(nb), shift(nb);
    tts::pack_conv2d(mode, h_w, Cout, Cin, ksize, reinterpret_cast<uint16_t*>(pa.data()));
    tts::pack_conv2d_epilogue(h_bias, h_scale, h_shift, Cout, bias.data(), scale.data(), shift.data());
    const tts::DeviceBuffer da = to_device(pa.data(), pa.size());
    const tts::DeviceBuffer db = to_device(bias.data(), nb), dsc = to_device(scale.data(), nb), dsh = to_device(shift.data(), nb);
    a.a = da.as<>(); a.bias = db.as<>(); a.scale = dsc.as<>(); a.shift = dsh.as<>();
    a.a_bytes = (unsigned)(n16 * 2);
    auto s = static_cast<hipStream_t>(hip_stream);
    tts::launch_conv2d(mode, a, B, s);
    TTS_HIP_CHECK(hipStreamSynchronize(s));
  });
}

int tts_op_conv2d_3x3_tile(void) { return tts::kConv2dTile; }

int tts_speaker_encoder_num_weights(const TtsSpeakerEncoderCfg* cfg) {
  return num_weights(cfg, tts::speaker_encoder_validate, tts::speaker_encoder_weight_shapes);
}

int64_t tts_speaker_encoder_weight_numel(const TtsSpeakerEncoderCfg* cfg, int idx) {
  return weight_numel(cfg, idx, tts::speaker_encoder_validate, tts::speaker_encoder_weight_shapes);
}

int tts_speaker_encoder_create(const TtsSpeakerEncoderCfg* cfg, const float* const* host_weights, int device,
                               void** handle) {
  return create<tts::SpeakerEncoder>(cfg, host_weights, device, handle);
}

int tts_speaker_encoder_destroy(void* handle) { return destroy<tts::SpeakerEncoder>(handle); }

int64_t tts_speaker_encoder_num_frames(const void* handle, int64_t n) {
  int64_t T = -1;
  int st = guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    T = static_cast<const tts::SpeakerEncoder*>(handle)->num_frames(n);
  });
  return st == TTS_OK ? T : -st;
}

int tts_speaker_encoder_forward(void* handle, const float* d_x, int B, int64_t n, int l2_norm, float* d_out,
                                void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::SpeakerEncoder*>(handle)->forward(d_x, B, n, l2_norm, d_out, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_speaker_encoder_forward_profiled(void* handle, const float* d_x, int B, int64_t n, int l2_norm, float* d_out,
                                         void* hip_stream, TtsLaunchRecord* records, int max_records, int* n_records) {
  auto body = [&](tts::SpeakerEncoder& h, hipStream_t s, tts::Profiler* prof) {
    h.forward(d_x, B, n, l2_norm, d_out, s, prof);
  };
  return profiled<tts::SpeakerEncoder>(handle, hip_stream, records, max_records, n_records, body);
}

int tts_speaker_encoder_features(void* handle, const float* d_x, int B, int64_t n, float* d_feat, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::SpeakerEncoder*>(handle)->features(d_x, B, n, d_feat, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_stft_create_centered(const TtsStftCfg* cfg, const float* h_window, int device, void** handle) {
  return guarded([&] {
    TTS_REQUIRE(cfg && h_window && handle, 1, "NULL argument");
    *handle = nullptr;
    *handle = new tts::Stft(*cfg, h_window, device, /*center=*/true);
  });
}

int tts_stft_num_frames_centered(const TtsStftCfg* cfg, int64_t N) {
  int n = -1;
  int st = guarded([&] {
    TTS_REQUIRE(cfg, 1, "NULL cfg");
    n = tts::stft_num_frames(*cfg, N, /*center=*/true);
  });
  return st == TTS_OK ? n : -st;
}

// ----------------------------------------------------------------------------- XTTS GPT
int tts_xtts_gpt_num_weights(const TtsXttsGptCfg* cfg) {
  return num_weights(cfg, tts::xtts_gpt_validate, tts::xtts_gpt_weight_shapes);
}

int64_t tts_xtts_gpt_weight_numel(const TtsXttsGptCfg* cfg, int idx) {
  return weight_numel(cfg, idx, tts::xtts_gpt_validate, tts::xtts_gpt_weight_shapes);
}

int tts_xtts_gpt_create(const TtsXttsGptCfg* cfg, const float* const* host_weights, int device, void** handle) {
  return create<tts::XttsGpt>(cfg, host_weights, device, handle);
}

int tts_xtts_gpt_destroy(void* handle) { return destroy<tts::XttsGpt>(handle); }

int tts_xtts_gpt_prefill(void* handle, const float* d_cond, const int64_t* d_tokens, const int64_t* d_text_lengths,
                         int B, int T_text, int max_new_tokens, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::XttsGpt*>(handle)->prefill(d_cond, d_tokens, d_text_lengths, B, T_text, max_new_tokens,
                                                static_cast<hipStream_t>(hip_stream));
  });
}

int tts_xtts_gpt_prefill_profiled(void* handle, const float* d_cond, const int64_t* d_tokens,
                                  const int64_t* d_text_lengths, int B, int T_text, int max_new_tokens,
                                  void* hip_stream, TtsLaunchRecord* records, int max_records, int* n_records) {
  auto body = [&](tts::XttsGpt& h, hipStream_t s, tts::Profiler* prof) {
    h.prefill(d_cond, d_tokens, d_text_lengths, B, T_text, max_new_tokens, s, prof);
  };
  return profiled<tts::XttsGpt>(handle, hip_stream, records, max_records, n_records, body);
}

int tts_xtts_gpt_generate(void* handle, int max_new_tokens, float repetition_penalty, float temperature, int top_k,
                          float top_p, const float* d_uniforms, int32_t* d_codes, int32_t* d_lengths, float* d_logits,
                          float* d_latents, int* steps_run, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    const int n = static_cast<tts::XttsGpt*>(handle)->generate(
        max_new_tokens, repetition_penalty, temperature, top_k, top_p, d_uniforms, d_codes, d_lengths, d_logits,
        d_latents, static_cast<hipStream_t>(hip_stream));
    if (steps_run) *steps_run = n;
  });
}

int tts_xtts_gpt_generate_profiled(void* handle, int max_new_tokens, float repetition_penalty, float temperature,
                                   int top_k, float top_p, const float* d_uniforms, int32_t* d_codes,
                                   int32_t* d_lengths, float* d_logits, float* d_latents, int* steps_run,
                                   void* hip_stream, TtsLaunchRecord* records, int max_records, int* n_records) {
  auto body = [&](tts::XttsGpt& h, hipStream_t s, tts::Profiler* prof) {
    const int n = h.generate(max_new_tokens, repetition_penalty, temperature, top_k, top_p, d_uniforms, d_codes,
                             d_lengths, d_logits, d_latents, s, prof);
    if (steps_run) *steps_run = n;
  };
  return profiled<tts::XttsGpt>(handle, hip_stream, records, max_records, n_records, body);
}

int tts_xtts_gpt_latents(void* handle, const int32_t* d_codes, const int32_t* d_lengths, int S, int rows,
                         float* d_latents, float* d_logits, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::XttsGpt*>(handle)->latents(d_codes, d_lengths, S, rows, d_latents, d_logits,
                                                static_cast<hipStream_t>(hip_stream));
  });
}

int tts_xtts_gpt_latents_profiled(void* handle, const int32_t* d_codes, const int32_t* d_lengths, int S, int rows,
                                  float* d_latents, float* d_logits, void* hip_stream, TtsLaunchRecord* records,
                                  int max_records, int* n_records) {
  auto body = [&](tts::XttsGpt& h, hipStream_t s, tts::Profiler* prof) {
    h.latents(d_codes, d_lengths, S, rows, d_latents, d_logits, s, prof);
  };
  return profiled<tts::XttsGpt>(handle, hip_stream, records, max_records, n_records, body);
}

int tts_op_gpt_decode_attn(const float* d_q, const float* d_k, const float* d_v, const int32_t* d_lengths, int B,
                           int E, int heads, int cap, float* d_out, void* hip_stream) {
  return guarded([&] {
    tts::op_gpt_decode_attn(d_q, d_k, d_v, d_lengths, B, E, heads, cap, d_out, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_op_gpt_decode_attn_waves(void) { return tts::kGptAttnWaves; }

int tts_op_mha_causal(const float* d_qkv, const int64_t* d_key_lengths, int B, int E, int heads, int T, int math_mode,
                      float* d_out, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_qkv && d_out, 1, "NULL argument");
    TTS_REQUIRE(math_mode >= tts::MATH_FP32 && math_mode <= tts::MATH_LAST, 1, "unknown math_mode");
    const int mode = math_mode == tts::MATH_BF16 ? tts::MATH_BF16 : tts::MATH_FP32_X6;
    tts::launch_mha_causal(mode, d_qkv, d_key_lengths, d_out, B, E, heads, T, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_op_gpt_sample(const float* d_logits, int B, int V, int32_t* d_codes, int n_prev, int start_audio_token,
                      float repetition_penalty, float temperature, int top_k, float top_p, const float* d_uniforms,
                      void* hip_stream) {
  return guarded([&] {
    tts::op_gpt_sample(d_logits, B, V, d_codes, n_prev, start_audio_token, repetition_penalty, temperature, top_k,
                       top_p, d_uniforms, static_cast<hipStream_t>(hip_stream));
  });
}

// ----------------------------------------------------------------------------- XTTS conditioning
int tts_xtts_cond_num_weights(const TtsXttsCondCfg* cfg) {
  return num_weights(cfg, tts::xtts_cond_validate, tts::xtts_cond_weight_shapes);
}

int64_t tts_xtts_cond_weight_numel(const TtsXttsCondCfg* cfg, int idx) {
  return weight_numel(cfg, idx, tts::xtts_cond_validate, tts::xtts_cond_weight_shapes);
}

int tts_xtts_cond_create(const TtsXttsCondCfg* cfg, const float* const* host_weights, int device, void** handle) {
  return create<tts::XttsCond>(cfg, host_weights, device, handle);
}

int tts_xtts_cond_destroy(void* handle) { return destroy<tts::XttsCond>(handle); }

int64_t tts_xtts_cond_num_frames(const void* handle, int64_t N) {
  int64_t T = -1;
  int st = guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    T = static_cast<const tts::XttsCond*>(handle)->num_frames(N);
  });
  return st == TTS_OK ? T : -st;
}

int tts_xtts_cond_mel(void* handle, const float* d_wav, int B, int64_t N, const float* d_mel_norms, float* d_mel,
                      void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::XttsCond*>(handle)->mel(d_wav, B, N, d_mel_norms, d_mel, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_xtts_cond_style_emb(void* handle, const float* d_mel, int B, int T, float* d_out, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::XttsCond*>(handle)->style_emb(d_mel, B, T, d_out, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_xtts_cond_style_emb_profiled(void* handle, const float* d_mel, int B, int T, float* d_out, void* hip_stream,
                                     TtsLaunchRecord* records, int max_records, int* n_records) {
  auto body = [&](tts::XttsCond& h, hipStream_t s, tts::Profiler* prof) { h.style_emb(d_mel, B, T, d_out, s, prof); };
  return profiled<tts::XttsCond>(handle, hip_stream, records, max_records, n_records, body);
}

int tts_resample_create(int orig_freq, int new_freq, int device, void** handle) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL argument");
    *handle = nullptr;
    *handle = new tts::Resampler(orig_freq, new_freq, device);
  });
}

int tts_resample_destroy(void* handle) { return destroy<tts::Resampler>(handle); }

int64_t tts_resample_num_samples(const void* handle, int64_t N) {
  int64_t n = -1;
  int st = guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    n = static_cast<const tts::Resampler*>(handle)->num_samples(N);
  });
  return st == TTS_OK ? n : -st;
}

int tts_resample_forward(void* handle, const float* d_x, int B, int64_t N, float* d_y, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(handle, 1, "NULL handle");
    static_cast<tts::Resampler*>(handle)->forward(d_x, B, N, d_y, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_op_groupnorm(const float* d_x, int B, int C, int T, int groups, const float* d_gamma, const float* d_beta,
                     float eps, float* d_y, void* hip_stream) {
  return guarded([&] {
    tts::launch_cond_groupnorm(d_x, d_gamma, d_beta, B, C, T, groups, eps, d_y, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_op_mha_wide(const float* d_qkv, const int64_t* d_key_lengths, int B, int E, int heads, int T, int math_mode,
                    float* d_out, void* hip_stream) {
  return guarded([&] {
    TTS_REQUIRE(d_qkv && d_out, 1, "NULL argument");
    TTS_REQUIRE(math_mode >= tts::MATH_FP32 && math_mode <= tts::MATH_LAST, 1, "unknown math_mode");
    const int mode = math_mode == tts::MATH_BF16 ? tts::MATH_BF16 : tts::MATH_FP32_X6;
    tts::launch_mha_wide(mode, d_qkv, d_key_lengths, d_out, B, E, heads, T, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_op_cross_attn(const float* d_q, const float* d_kv_lat, const float* d_kv_ctx, int B, int heads, int dim_head,
                      int L, int T, float* d_out, void* hip_stream) {
  return guarded([&] {
    tts::launch_cond_cross_attn(d_q, d_kv_lat, d_kv_ctx, B, heads, dim_head, L, T, d_out,
                                static_cast<hipStream_t>(hip_stream));
  });
}

int tts_op_cond_ff(const float* d_x, int B, int E, int I, int L, const float* h_w0, const float* h_b0,
                   const float* h_w2, const float* h_b2, int math_mode, float* d_out, void* hip_stream) {
  return guarded([&] {
    tts::op_cond_ff(d_x, B, E, I, L, h_w0, h_b0, h_w2, h_b2, math_mode, d_out, static_cast<hipStream_t>(hip_stream));
  });
}

int tts_op_rmsnorm(const float* d_x, int B, int E, int L, const float* d_gamma, float* d_y, void* hip_stream) {
  return guarded([&] {
    tts::launch_cond_rmsnorm(d_x, d_gamma, B, E, L, d_y, static_cast<hipStream_t>(hip_stream));
  });
}

}  // extern "C"
