// Batch gather from a device-resident data set: x_out[b] = x_all[idx[b]], y_out[b] = y_all[idx[b]], bit for bit.
// A pure copy.  One launch covers both arrays of up to kGatherMax images: grid (kGatherXBlocks + kGatherYBlocks, images), the first
// kGatherXBlocks columns sweep the image, the rest the heat maps, each work group striding over its image in 16-byte pieces (uint4) when
// the image's byte count and both base addresses are multiples of 16 -- every image then starts 16-byte aligned -- and in 4-byte pieces
// otherwise (chosen per array on the host).  The indices travel in the kernel arguments (GatherIdx): no staging buffer, no copy, nothing
// for the host to wait for or to keep alive.  The entry point has checked every index against [0, N) before the launch.
// Byte data sets: the image columns convert instead of copying, x_out = u8_to_f32(x_all[idx]) -- a lane takes one aligned dword
// of four image bytes and writes one float4, so a wave reads 256 contiguous bytes and writes 1 KB of whole lines per instruction (wide path:
// image byte count and source base multiples of 4, destination base a multiple of 16); byte loads and dword stores otherwise.
#include <string>

#include "entry.h"
#include "u8.h"

namespace jcm {

namespace {

constexpr int kGatherThreads = 256;
// 14 images x (120 + 8) work groups = 1 792 = 7 per CU: 259 200 uint4 per 480 x 720 x 3 image / (120 x 256 lanes) = 8.4 pieces per lane in the image columns,
// 13 500 uint4 per 60 x 90 x 10 map / (8 x 256) = 6.6 in the heat-map columns
constexpr int kGatherXBlocks = 120, kGatherYBlocks = 8;

template <class T>
__device__ __forceinline__ void copy_image(const T* __restrict__ src, T* __restrict__ dst, size_t n, int part, int parts) {
  const size_t step = (size_t)parts * kGatherThreads;
  size_t i = (size_t)part * kGatherThreads + threadIdx.x;
  for (; i + 3 * step < n; i += 4 * step) {      // four independent loads in flight per lane
    const T a = src[i], b = src[i + step], c = src[i + 2 * step], d = src[i + 3 * step];
    dst[i] = a;
    dst[i + step] = b;
    dst[i + 2 * step] = c;
    dst[i + 3 * step] = d;
  }
  for (; i < n; i += step) dst[i] = src[i];
}

// dst[i] = u8_to_f32(src[i]), n values.  WIDE: four values per piece (src 4-byte aligned, dst 16-byte aligned, n % 4 == 0)
template <bool WIDE>
__device__ __forceinline__ void convert_image(const uint8_t* __restrict__ src, float* __restrict__ dst, size_t n, int part, int parts) {
  const size_t step = (size_t)parts * kGatherThreads;
  size_t i = (size_t)part * kGatherThreads + threadIdx.x;
  if constexpr (WIDE) {
    const unsigned* s4 = reinterpret_cast<const unsigned*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    const size_t n4 = n / 4;
    auto cvt = [](unsigned w) { return make_float4(u8_to_f32(w & 255u), u8_to_f32((w >> 8) & 255u), u8_to_f32((w >> 16) & 255u), u8_to_f32(w >> 24)); };
    for (; i + 3 * step < n4; i += 4 * step) {      // four independent loads in flight per lane
      const unsigned a = s4[i], b = s4[i + step], c = s4[i + 2 * step], d = s4[i + 3 * step];
      d4[i] = cvt(a);
      d4[i + step] = cvt(b);
      d4[i + 2 * step] = cvt(c);
      d4[i + 3 * step] = cvt(d);
    }
    for (; i < n4; i += step) d4[i] = cvt(s4[i]);
  } else {
    for (; i < n; i += step) dst[i] = u8_to_f32(src[i]);
  }
}

// image columns convert nx bytes -> nx floats, heat-map columns copy ny elements of TY
template <bool WIDE, class TY>
__global__ __launch_bounds__(kGatherThreads) void gather_batch_u8_kernel(const uint8_t* __restrict__ x_all, const TY* __restrict__ y_all, GatherIdx idx,
                                                                         size_t nx, size_t ny, float* __restrict__ x_out, TY* __restrict__ y_out) {
  const int b = blockIdx.y;
  const size_t src = (size_t)idx.v[b];
  const int part = blockIdx.x;
  if (part < kGatherXBlocks)
    convert_image<WIDE>(x_all + src * nx, x_out + (size_t)b * nx, nx, part, kGatherXBlocks);
  else
    copy_image(y_all + src * ny, y_out + (size_t)b * ny, ny, part - kGatherXBlocks, kGatherYBlocks);
}

template <bool WIDE>
__global__ __launch_bounds__(kGatherThreads) void u8_to_f32_kernel(const uint8_t* __restrict__ x, float* __restrict__ out, size_t n) {
  convert_image<WIDE>(x, out, n, blockIdx.x, gridDim.x);
}

// nx / ny: elements of TX / TY per image
template <class TX, class TY>
__global__ __launch_bounds__(kGatherThreads) void gather_batch_kernel(const TX* __restrict__ x_all, const TY* __restrict__ y_all, GatherIdx idx, size_t nx,
                                                                      size_t ny, TX* __restrict__ x_out, TY* __restrict__ y_out) {
  const int b = blockIdx.y;
  const size_t src = (size_t)idx.v[b];
  const int part = blockIdx.x;
  if (part < kGatherXBlocks)
    copy_image(x_all + src * nx, x_out + (size_t)b * nx, nx, part, kGatherXBlocks);
  else
    copy_image(y_all + src * ny, y_out + (size_t)b * ny, ny, part - kGatherXBlocks, kGatherYBlocks);
}

template <class TX, class TY>
void launch(const float* x_all, const float* y_all, const GatherIdx& idx, int B, size_t nx, size_t ny, float* x_out, float* y_out, hipStream_t st) {
  hipLaunchKernelGGL((gather_batch_kernel<TX, TY>), dim3(kGatherXBlocks + kGatherYBlocks, B), dim3(kGatherThreads), 0, st,
                     reinterpret_cast<const TX*>(x_all), reinterpret_cast<const TY*>(y_all), idx, nx * sizeof(float) / sizeof(TX),
                     ny * sizeof(float) / sizeof(TY), reinterpret_cast<TX*>(x_out), reinterpret_cast<TY*>(y_out));
}

bool wide(const void* a, const void* b, size_t floats_per_image) {
  return (floats_per_image * sizeof(float)) % 16 == 0 && reinterpret_cast<uintptr_t>(a) % 16 == 0 && reinterpret_cast<uintptr_t>(b) % 16 == 0;
}

template <bool WIDE, class TY>
void launch_u8(const uint8_t* x_all, const float* y_all, const GatherIdx& idx, int B, size_t nx, size_t ny, float* x_out, float* y_out, hipStream_t st) {
  hipLaunchKernelGGL((gather_batch_u8_kernel<WIDE, TY>), dim3(kGatherXBlocks + kGatherYBlocks, B), dim3(kGatherThreads), 0, st, x_all,
                     reinterpret_cast<const TY*>(y_all), idx, nx, ny * sizeof(float) / sizeof(TY), x_out, reinterpret_cast<TY*>(y_out));
}

// every image of a byte array starts 4-byte aligned and every converted image 16-byte aligned
bool wide_u8(const void* src, const void* dst, size_t bytes_per_image) {
  return bytes_per_image % 4 == 0 && reinterpret_cast<uintptr_t>(src) % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0;
}

}  // namespace

// the same from a byte image array: x_out[b][i] = u8_to_f32(x_all[idx[b]][i]) (u8.h), nx values per image; the heat maps are copied as below
static hipError_t gather_batch_u8(const uint8_t* x_all, const float* y_all, const int* idx, int B, size_t nx, size_t ny, float* x_out, float* y_out,
                                  hipStream_t st) {
  const bool wx = wide_u8(x_all, x_out, nx), wy = wide(y_all, y_out, ny);
  for (int b0 = 0; b0 < B; b0 += kGatherMax) {
    const int nb = B - b0 < kGatherMax ? B - b0 : kGatherMax;
    GatherIdx g;
    for (int i = 0; i < kGatherMax; ++i) g.v[i] = i < nb ? idx[b0 + i] : 0;
    float *xo = x_out + (size_t)b0 * nx, *yo = y_out + (size_t)b0 * ny;
    if (wx && wy) launch_u8<true, uint4>(x_all, y_all, g, nb, nx, ny, xo, yo, st);
    else if (wx) launch_u8<true, float>(x_all, y_all, g, nb, nx, ny, xo, yo, st);
    else if (wy) launch_u8<false, uint4>(x_all, y_all, g, nb, nx, ny, xo, yo, st);
    else launch_u8<false, float>(x_all, y_all, g, nb, nx, ny, xo, yo, st);
  }
  return hipGetLastError();
}

hipError_t u8_to_f32_array(const uint8_t* x, float* x_out, size_t n, hipStream_t st) {
  const size_t pieces = (n + 4 * kGatherThreads - 1) / (4 * kGatherThreads);
  const int grid = (int)(pieces < 2048 ? (pieces ? pieces : 1) : 2048);
  if (wide_u8(x, x_out, n)) hipLaunchKernelGGL(u8_to_f32_kernel<true>, dim3(grid), dim3(kGatherThreads), 0, st, x, x_out, n);
  else hipLaunchKernelGGL(u8_to_f32_kernel<false>, dim3(grid), dim3(kGatherThreads), 0, st, x, x_out, n);
  return hipGetLastError();
}

// x_out[b] = x_all[idx[b]] (nx floats per image), y_out[b] = y_all[idx[b]] (ny floats); idx: HOST, B entries, every one checked by the entry point
static hipError_t gather_batch(const float* x_all, const float* y_all, const int* idx, int B, size_t nx, size_t ny, float* x_out, float* y_out,
                               hipStream_t st) {
  const bool wx = wide(x_all, x_out, nx), wy = wide(y_all, y_out, ny);
  for (int b0 = 0; b0 < B; b0 += kGatherMax) {
    const int nb = B - b0 < kGatherMax ? B - b0 : kGatherMax;
    GatherIdx g;
    for (int i = 0; i < kGatherMax; ++i) g.v[i] = i < nb ? idx[b0 + i] : 0;
    float *xo = x_out + (size_t)b0 * nx, *yo = y_out + (size_t)b0 * ny;      // b0 * nx * 4 bytes keeps the 16-byte alignment when nx * 4 is a multiple of 16
    if (wx && wy) launch<uint4, uint4>(x_all, y_all, g, nb, nx, ny, xo, yo, st);
    else if (wx) launch<uint4, float>(x_all, y_all, g, nb, nx, ny, xo, yo, st);
    else if (wy) launch<float, uint4>(x_all, y_all, g, nb, nx, ny, xo, yo, st);
    else launch<float, float>(x_all, y_all, g, nb, nx, ny, xo, yo, st);
  }
  return hipGetLastError();
}

// (declared in entry.h: augment.hip's indexed entries take the same rules)
int check_indexed(const char* who, const void* x_all, size_t xes, const float* y_all, int64_t N, const int32_t* idx, const float* params, int B, int H, int W,
                  int hh, int hw, int Ky, int min_side, const float* x_out, const float* y_out) {
  const std::string w(who);
  if (!x_all || !y_all || !idx || !x_out || !y_out) return fail(JCM_ERR_ARG, w + ": null pointer");
  if (N < 1 || N > INT32_MAX || B < 1 || B > 65535 || H < min_side || W < min_side || hh < min_side || hw < min_side ||
      (int64_t)H * W * 3 >= (int64_t)1 << 30 || (int64_t)hh * hw * Ky >= (int64_t)1 << 30)
    return fail(JCM_ERR_ARG, w + ": bad sizes (N in [1, 2^31), B in [1, 65535], H, W, h, w >= " + std::to_string(min_side) + ")");
  for (int b = 0; b < B; ++b)
    if (idx[b] < 0 || (int64_t)idx[b] >= N)
      return fail(JCM_ERR_ARG, w + ": idx[" + std::to_string(b) + "] = " + std::to_string(idx[b]) + " is outside [0, " + std::to_string(N) + ")");
  const size_t ix = (size_t)H * W * 3 * sizeof(float), iy = (size_t)hh * hw * Ky * sizeof(float);
  const size_t nxa = (size_t)N * H * W * 3 * xes, nya = (size_t)N * iy, nx = (size_t)B * ix, ny = (size_t)B * iy, np = (size_t)B * 6 * sizeof(float);
  const auto overlap = [](const void* a, size_t na, const void* b, size_t nb) { return b != nullptr && ranges_overlap(a, na, b, nb); };
  if (overlap(x_out, nx, x_all, nxa) || overlap(x_out, nx, y_all, nya) || overlap(x_out, nx, params, np) || overlap(y_out, ny, x_all, nxa) ||
      overlap(y_out, ny, y_all, nya) || overlap(y_out, ny, params, np) || overlap(x_out, nx, y_out, ny))
    return fail(JCM_ERR_ARG, w + ": x_out / y_out overlap the data set, params or each other");
  return JCM_OK;
}

}  // namespace jcm

using namespace jcm;

extern "C" {

int jcm_gather_batch(jcm_handle h, const float* x_all, const float* y_all, int64_t N, const int32_t* idx, int B, int H, int W, int hh,
                     int hw, float* x_out, float* y_out) {
  JCM_TRY(check(h, false));
  const int Ky = h->K + 1;
  JCM_TRY(check_indexed("gather_batch", x_all, sizeof(float), y_all, N, idx, nullptr, B, H, W, hh, hw, Ky, 1, x_out, y_out));
  DeviceGuard g(h->device);
  CallOrder order(h);
  HIP_TRY(gather_batch(x_all, y_all, idx, B, (size_t)H * W * 3, (size_t)hh * hw * Ky, x_out, y_out, h->stream));
  return JCM_OK;
}

int jcm_gather_batch_u8(jcm_handle h, const uint8_t* x_all, const float* y_all, int64_t N, const int32_t* idx, int B, int H, int W, int hh,
                        int hw, float* x_out, float* y_out) {
  JCM_TRY(check(h, false));
  const int Ky = h->K + 1;
  JCM_TRY(check_indexed("gather_batch_u8", x_all, 1, y_all, N, idx, nullptr, B, H, W, hh, hw, Ky, 1, x_out, y_out));
  DeviceGuard g(h->device);
  CallOrder order(h);
  HIP_TRY(gather_batch_u8(x_all, y_all, idx, B, (size_t)H * W * 3, (size_t)hh * hw * Ky, x_out, y_out, h->stream));
  return JCM_OK;
}

}  // extern "C"
