// The host side the entry points of the sequence library share (sequence.hip, seq_centred.hip, seq_tracks.hip, seq_smooth.hip): ONE copy of the argument rules and
// of the taps upload in front of the launch (on entry.h's scaffold), as seq_scan.h is the one copy of the scans.  Host code only; every message is
// part of the interface.
#pragma once

#include <string>

#include "entry.h"

namespace jcm {

// The argument rules in the order they are tried: sizes, the entry's channel rules, R, rho, the map limit, the index range, null pointers.
// sizes / sizes_ok: what the first rule names and whether it holds beyond S, T, HH, WW >= 1;  channels(): the rules of K, or of M and D;
// max_hw / planes: the map limit and what fills the LDS at it;  per_frame / per_frame_name: the factor of S * T in the largest output index.
template <class Channels>
int seq_check(const std::string& w, const float* hm, int S, int T, int HH, int WW, const double* taps, int R, double rho, const char* sizes, bool sizes_ok,
              Channels&& channels, int max_hw, const char* planes, int per_frame, const char* per_frame_name) {
  if (S < 1 || T < 1 || HH < 1 || WW < 1 || !sizes_ok) return fail(JCM_ERR_ARG, w + ": bad sizes (" + sizes + " >= 1)");
  JCM_TRY(channels());
  if (R < 0 || R > kSeqMaxR) return fail(JCM_ERR_ARG, w + ": R = " + std::to_string(R) + "; 0 <= R <= 16");
  if (!(rho >= 0.0 && rho <= 1.0)) return fail(JCM_ERR_ARG, w + ": rho outside [0, 1]");
  if ((int64_t)HH * WW > max_hw)
    return fail(JCM_ERR_ARG, w + ": a map of " + std::to_string(HH) + " x " + std::to_string(WW) + " cells; HH * WW <= " + std::to_string(max_hw) + " (" +
                                 planes + " in 160 KB of LDS), a larger map is not truncated");
  if ((int64_t)S * T >= ((int64_t)1 << 31) / per_frame) return fail(JCM_ERR_ARG, w + ": bad sizes (S * T * " + per_frame_name + " < 2^31)");
  if (!hm || !taps) return fail(JCM_ERR_ARG, w + ": null pointer (hm and taps are required)");
  return JCM_OK;
}

constexpr const char* kSeqScanPlanes = "two float64 planes and a byte plane";      // what the scans of seq_scan.h keep in LDS, at kSeqMaxHW cells

// ... of the maps [S,T,HH,WW,K] of K joints
inline int seq_check_joints(const std::string& w, const float* hm, int S, int T, int HH, int WW, int K, const double* taps, int R, double rho, int max_hw,
                            const char* planes) {
  return seq_check(w, hm, S, T, HH, WW, taps, R, rho, "S, T, HH, WW, K", K >= 1, [&] {
    if (K > kSeqMaxK) return fail(JCM_ERR_ARG, w + ": K = " + std::to_string(K) + " joints; K <= 16");
    return (int)JCM_OK;
  }, max_hw, planes, K, "K");
}

// Both passes of with_arena: the n_taps device taps come first in the arena, then whatever alloc() takes from it; the real pass uploads the taps and
// runs launch(device taps) between one pair of profile events named `what` (entry.h: arena_launch).
template <class Alloc, class Launch>
int seq_launch(jcm_ctx* c, const std::string& what, const double* taps, int n_taps, Alloc&& alloc, Launch&& launch) {
  double* dtaps = nullptr;
  return arena_launch(c, what, [&] {
    dtaps = arena_alloc<double>(c, (size_t)n_taps);
    alloc();
  }, [&] {
    const hipError_t e = seq_put_taps(taps, n_taps, dtaps, c->stream);
    return e == hipSuccess ? launch(dtaps) : e;
  });
}

}  // namespace jcm
