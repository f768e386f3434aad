// Glow-TTS alignment (TTS/tts/models/glow_tts.py:193-247, TTS/tts/utils/helpers.py maximum_path):
// the [B][T_en][T_de] log-likelihood matrix and Monotonic Alignment Search (kernels_mas.hip).
#pragma once

#include <cstddef>
#include <cstdint>

#include "common.hpp"

namespace tts {

// Limits of maximum_path: T_en <= MAS_MAX_TEN tokens (one wave holds an item's column, up to 16
// tokens per lane); any T_de whose [T_en][T_de] fp32 value plane stays under 2 GiB; B <= 65535.
constexpr int MAS_MAX_TEN = 1024;
// Backtrack decision bits of an item stay in LDS up to this many bytes, else they go to the workspace
constexpr int MAS_BITS_LDS = 96 * 1024;

// tokens per lane (1, 2, 4, 8 or 16) of the MAS kernel for T_en tokens
inline int mas_xpt(int T_en) {
  int x = 1;
  while (64 * x < T_en) x *= 2;
  return x;
}
// decision words per item: one 32-bit word per (32-column chunk, padded token row)
inline size_t mas_bits_words(int T_en, int T_de) { return (size_t)((T_de + 31) / 32) * (size_t)(64 * mas_xpt(T_en)); }
inline bool mas_bits_in_lds(int T_en, int T_de) { return mas_bits_words(T_en, T_de) * 4 <= (size_t)MAS_BITS_LDS; }
// workspace: row starts [B][T_en + 1] int32 (rounded up to 256 B), then the decision words of every
// item when they do not fit in LDS
inline size_t mas_starts_bytes(int B, int T_en) { return (((size_t)B * (size_t)(T_en + 1) * 4) + 255) / 256 * 256; }
inline size_t mas_workspace_bytes(int B, int T_en, int T_de) {
  return mas_starts_bytes(B, T_en) + (mas_bits_in_lds(T_en, T_de) ? 0 : (size_t)B * mas_bits_words(T_en, T_de) * 4);
}

// logp [B][T_en][T_de] from o_mean, o_log_scale [B][C][T_en] (o_log_scale NULL: zeros) and z [B][C][T_de]
void launch_mas_logp(const float* o_mean, const float* o_log_scale, const float* z, int B, int C, int T_en, int T_de,
                     float* logp, hipStream_t s);

// value, mask (may be NULL) [B][T_en][T_de]; t_x, t_y [B] int64; path [B][T_en][T_de], durations,
// log_dur [B][T_en] (each may be NULL); workspace of mas_workspace_bytes(B, T_en, T_de)
void launch_maximum_path(const float* value, const float* mask, const int64_t* t_x, const int64_t* t_y, int B, int T_en,
                         int T_de, void* workspace, float* path, float* durations, float* log_dur, hipStream_t s);

}  // namespace tts
