// Byte images.  data.load_image makes every image value as float32(k) / float32(255) for a byte k, so a byte image IS the
// float image: u8_to_f32 below is that conversion, and the ONLY place it is written for the device.  It is a true IEEE division (hipcc
// expands it to v_div_scale / v_rcp / the fma refinement / v_div_fmas / v_div_fixup: correctly rounded), not a multiplication by
// float32(1/255), which differs from numpy for 126 of the 256 bytes.  tests/test_gpu_u8.py runs all 256 bytes through it (by way of the
// gather) and compares with numpy bit for bit -- a build flag that relaxed the division would fail there.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace jcm {

__device__ __forceinline__ float u8_to_f32(unsigned k) { return (float)k / 255.0f; }

// one image value as the float the kernels compute on: floats pass, bytes go through u8_to_f32
__device__ __forceinline__ float px_f32(float v) { return v; }
__device__ __forceinline__ float px_f32(uint8_t v) { return u8_to_f32(v); }

}  // namespace jcm
