// w2a_episode_word.h -- which form the lock-step mirror's per-episode word takes on a handle (StateArrays::pk_c,
// w2a_common.hip.h). Decided once, by w2a_create, from the table dims alone.
//
// Plain C++, no HIP (like w2a_bookkeeping.h): libw2a.so compiles it, and tests/test_episode_word_gpu.py compiles the same
// header on the CPU to check the rule for the table sizes the benchmark uses.
#ifndef W2A_EPISODE_WORD_H
#define W2A_EPISODE_WORD_H

#include <stdint.h>

// number of bits that hold every value 0 .. v
static inline int ew_bits(uint64_t v) {
  int b = 0;
  while (v) { ++b; v >>= 1; }
  return b;
}

struct EpisodeWord {
  int narrow;   // 1: one u32 per env, wrow | xrow << kw; 0: the 8-byte word
  int kw, kx;   // bits of the coefficient-row index (col * n_samples + sample) and of the day-row index (county_w * Y + year_i)
};

// Narrow when both row indices of an episode fit one 32-bit word together. (The budget does not travel with them: the
// narrow form keeps the REMAINING budget in pk_hot.x.) force_wide: debug / A-B switch, w2a_set_episode_word.
static inline EpisodeWord ew_choose(int32_t S, int32_t n_samples, int32_t S_w, int32_t Y, bool force_wide) {
  EpisodeWord w;
  w.kw = ew_bits((uint64_t)S * (uint64_t)n_samples - 1u);
  w.kx = ew_bits((uint64_t)S_w * (uint64_t)Y - 1u);
  w.narrow = (!force_wide && w.kw + w.kx <= 32 && w.kw < 32) ? 1 : 0;
  return w;
}

#endif  // W2A_EPISODE_WORD_H
