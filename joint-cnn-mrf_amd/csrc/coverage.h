// The 16 sub-samples of a pixel (include/jcm.h: jcm_render_poses, jcm_synth_people), shared by render.hip and synth_people.hip: pixel (y, x) has its
// centre at (16 y, 16 x) sixteenths and samples at 16 y - 6 + 4 iy, 16 x - 6 + 4 ix, iy, ix = 0..3.  Both tests run on exact integers -- the
// capsule's in float64 products of integers below 2^21 (exact up to 2^53 in every term that is compared), the quadrilateral's in int64.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace jcm {

// the count of the pixel's 16 sub-samples inside capsule (ay, ax) - (by, bx), radius r, all in sixteenths of a pixel (jcm.h has the test)
__device__ __forceinline__ int render_coverage(int y, int x, int ay, int ax, int by, int bx, int r) {
  const double dy = (double)(by - ay), dx = (double)(bx - ax);
  const double L2 = dy * dy + dx * dx, rr = (double)r * (double)r, rrL2 = rr * L2;
  int c = 0;
#pragma unroll
  for (int iy = 0; iy < 4; ++iy) {
    const int sy = 16 * y - 6 + 4 * iy;
    const double ey = (double)(sy - ay), fy = (double)(sy - by);
    const double eyy = ey * ey, eydy = ey * dy, fyy = fy * fy;
#pragma unroll
    for (int ix = 0; ix < 4; ++ix) {
      const int sx = 16 * x - 6 + 4 * ix;
      const double ex = (double)(sx - ax), fx = (double)(sx - bx);
      const double ee = eyy + ex * ex, t = eydy + ex * dx;
      bool in;
      if (L2 == 0.0 || t <= 0.0) in = ee <= rr;
      else if (t >= L2) in = fyy + fx * fx <= rr;
      else in = ee * L2 - t * t <= rrL2;
      c += in ? 1 : 0;
    }
  }
  return c;
}

// the same count for the quadrilateral q = (y0, x0, y1, x1, y2, x2, y3, x3), vertices in order: a sample is inside when the four edge cross
// products (v[i+1] - v[i]) x (s - v[i]) are all >= 0 or all <= 0 (either winding; a sample on an edge is inside), in 64-bit integers
__device__ __forceinline__ int quad_coverage(int y, int x, const int* q) {
  int64_t ey[4], ex[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ey[i] = (int64_t)q[2 * ((i + 1) & 3)] - q[2 * i];
    ex[i] = (int64_t)q[2 * ((i + 1) & 3) + 1] - q[2 * i + 1];
  }
  int c = 0;
#pragma unroll
  for (int iy = 0; iy < 4; ++iy) {
    const int sy = 16 * y - 6 + 4 * iy;
#pragma unroll
    for (int ix = 0; ix < 4; ++ix) {
      const int sx = 16 * x - 6 + 4 * ix;
      bool ge = true, le = true;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t cr = ey[i] * (int64_t)(sx - q[2 * i + 1]) - ex[i] * (int64_t)(sy - q[2 * i]);
        ge = ge && cr >= 0;
        le = le && cr <= 0;
      }
      c += (ge || le) ? 1 : 0;
    }
  }
  return c;
}

}  // namespace jcm
