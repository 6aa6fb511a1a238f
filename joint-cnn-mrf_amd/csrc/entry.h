// The host side the entry points share, whatever file they sit in: ONE copy of the timed launch, of its workspace variant, of the workspace refusal and of
// the argument rules that more than one file states.  DeviceGuard and CallOrder are NOT in here: each entry point takes them itself, where their place among
// its argument checks can be read.  Host code only; every message is part of the interface.
#pragma once

#include <string>

#include "ctx.h"

namespace jcm {

// launch() enqueues on c->stream and returns its hipError_t.  The work lies between one pair of profile events filed under `what` (jcm_profile_read); an
// error is reported under the same name.
template <class Launch>
int timed_launch(jcm_ctx* c, const std::string& what, Launch&& launch) {
  hipEvent_t e0, e1;
  JCM_TRY(prof_begin(c, &e0, &e1));
  const hipError_t e = launch();
  prof_end(c, what, e0, e1, e == hipSuccess);
  if (e != hipSuccess) return fail(JCM_ERR_HIP, what + ": " + hipGetErrorString(e));
  return JCM_OK;
}

// Both passes of with_arena: alloc() takes the call's workspace from the arena (the sizing pass sees the same calls in the same order); the real pass then
// is timed_launch(launch).
template <class Alloc, class Launch>
int arena_launch(jcm_ctx* c, const std::string& what, Alloc&& alloc, Launch&& launch) {
  return with_arena(c, [&] {
    alloc();
    if (c->dry) return (int)JCM_OK;
    return timed_launch(c, what, launch);
  });
}

// The workspace grows to hold need_bytes; a clip whose `noun` ("back-pointers", "beliefs") cannot fit in what the device has left is refused.
inline int workspace_or_refuse(jcm_ctx* c, const std::string& what, double need_bytes, const char* noun, int S, int T) {
  if (need_bytes <= (double)c->arena_cap) return JCM_OK;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (need_bytes > (double)free_b + (double)c->arena_cap)
    return fail(JCM_ERR_STATE, what + ": the " + noun + " of " + std::to_string(S) + " x " + std::to_string(T) + " frames need " +
                                   std::to_string((unsigned long long)need_bytes) + " bytes of workspace, " +
                                   std::to_string((unsigned long long)(free_b + c->arena_cap)) + " bytes are available; split the clip");
  return JCM_OK;
}

// do the byte ranges [a, a + na) and [b, b + nb) share a byte?  (each caller words its own refusal)
inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const char *pa = static_cast<const char*>(a), *pb = static_cast<const char*>(b);
  return pa < pb + nb && pb < pa + na;
}

// the content rectangle (y0, x0, ch, cw) of the H x W frames of a clip (jcm_frame_shift, jcm_frame_flow)
inline int check_rectangle(const std::string& w, int H, int W, int y0, int x0, int ch, int cw) {
  if (y0 < 0 || x0 < 0 || ch < 1 || cw < 1 || y0 > H - ch || x0 > W - cw)
    return fail(JCM_ERR_ARG, w + ": the rectangle (" + std::to_string(y0) + ", " + std::to_string(x0) + ", " + std::to_string(ch) + ", " + std::to_string(cw) +
                                 ") is not inside the frame of " + std::to_string(H) + " x " + std::to_string(W));
  return JCM_OK;
}

// ---- gather.hip: the argument rules of the indexed entries (jcm_gather_batch*, and augment.hip's jcm_augment_train_indexed*) ----
// Ky = heat-map channels; params may be null (gather); xes: bytes per image value of the data set (4, or 1 for a byte data set; the outputs are fp32 either way)
int check_indexed(const char* who, const void* x_all, size_t xes, const float* y_all, int64_t N, const int32_t* idx, const float* params, int B, int H, int W,
                  int hh, int hw, int Ky, int min_side, const float* x_out, const float* y_out);

}  // namespace jcm
