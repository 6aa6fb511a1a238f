// The handle's options: ONE table behind jcm_set_option / jcm_get_option (jcm_api.hip) and the only place where the library reads the
// environment (jcm_create seeds the rows that name a variable).  include/jcm.h documents the same rows, with the defaults, which are the
// initialisers of the fields in ctx.h; tests/test_gpu_options.py holds the two against each other.
#pragma once
#include <climits>

#include "ctx.h"

namespace jcm {

struct Option {
  enum Kind { BOOL, RANGE, EITHER };      // BOOL: stores value != 0;  RANGE: lo <= value <= hi;  EITHER: value == lo or value == hi
  const char* name;
  int jcm_ctx::*field;
  Kind kind;
  int64_t lo, hi;
  bool before_finalize;                   // JCM_ERR_STATE once the handle is finalized
  const char* env;                        // environment variable that supplies the default (atoi; unset = the field's initialiser), or null
  int (*on_change)(jcm_ctx*, int64_t);    // runs in front of the store (not for the environment default), or null
};

int option_profile(jcm_ctx* c, int64_t value);         // switching it on starts a fresh record: the events go back to the pool
int option_fft_single(jcm_ctx* c, int64_t value);      // the filter spectra have another form: the cache is dropped

inline constexpr Option kOptions[] = {
    // name             field                      kind            lo  hi       before_finalize  env                    on_change
    {"precision",       &jcm_ctx::precision,       Option::RANGE,  0,  1,       true,  nullptr,               nullptr},
    {"n_joints",        &jcm_ctx::K,               Option::RANGE,  1,  9,       true,  nullptr,               nullptr},
    {"f32_conv",        &jcm_ctx::f32_conv,        Option::EITHER, 0,  2,       true,  nullptr,               nullptr},
    {"split_min_wgs",   &jcm_ctx::split_min_wgs,   Option::RANGE,  0,  INT_MAX, false, nullptr,               nullptr},
    {"profile",         &jcm_ctx::profile,         Option::BOOL,   0,  1,       false, nullptr,               option_profile},
    {"conv9_fft",       &jcm_ctx::conv9_fft,       Option::BOOL,   0,  1,       false, nullptr,               nullptr},
    {"call_order",      &jcm_ctx::call_order,      Option::BOOL,   0,  1,       false, nullptr,               nullptr},
    {"fft_single",      &jcm_ctx::fft_single,      Option::BOOL,   0,  1,       false, nullptr,               option_fft_single},
    {"fft_t16",         &jcm_ctx::fft_t16,         Option::BOOL,   0,  1,       false, nullptr,               nullptr},
    {"fft_rows_mfma",   &jcm_ctx::fft_rows_mfma,   Option::BOOL,   0,  1,       false, nullptr,               nullptr},
    {"fft_windows",     &jcm_ctx::fft_win,         Option::BOOL,   0,  1,       false, nullptr,               nullptr},
    {"fft_fuse",        &jcm_ctx::fft_fuse,        Option::RANGE,  0,  7,       false, nullptr,               nullptr},
    {"fft_tiles",       &jcm_ctx::fft_tiles,       Option::BOOL,   0,  1,       false, "JCM_FFT_TILES",       nullptr},
    {"fft_logits_rows", &jcm_ctx::fft_logits_rows, Option::BOOL,   0,  1,       false, "JCM_FFT_LOGITS_ROWS", nullptr},
    {"fft_reg",         &jcm_ctx::fft_reg,         Option::BOOL,   0,  1,       false, "JCM_FFT_REG",         nullptr},
    {"fft_cache_gb",    &jcm_ctx::fft_cache_gb,    Option::RANGE,  0,  1 << 20, false, "JCM_FFT_CACHE_GB",    nullptr},
    {"bf16_hpool",      &jcm_ctx::bf16_hpool,      Option::BOOL,   0,  1,       false, nullptr,               nullptr},
    {"sm_algo",         &jcm_ctx::sm_algo,         Option::EITHER, 1,  3,       false, nullptr,               nullptr},
    {"torso_algo",      &jcm_ctx::torso_algo,      Option::EITHER, 1,  1,       false, nullptr,               nullptr},
    {"sm_chunk",        &jcm_ctx::sm_chunk,        Option::RANGE,  1,  INT_MAX, false, nullptr,               nullptr},
    {"micro_batch",     &jcm_ctx::micro_batch,     Option::RANGE,  0,  INT_MAX, false, nullptr,               nullptr},
    {"debug_skip",      &jcm_ctx::debug_skip,      Option::RANGE,  0,  127,     false, nullptr,               nullptr},
};

}  // namespace jcm
