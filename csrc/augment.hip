// Training augmentation of HBM-resident folder data (data/augment.py, data/device_folder.py).
//
//   dpa_batch_augment_u8   the per-step batch of dpa_batch_gather_u8 (data_prep.hip) with a random warp and a tone
//                          curve folded in: gather by index, an inverse affine map per item (bilinear for the image,
//                          nearest for the mask, clamp-to-edge for both), a 256-entry float table per item, float32
//                          (images [B,C,H,W], targets [B,1,H,W]) out.
//
// The arithmetic is integer and is the definition (augment.py: augment_reference implements the same lines), so
// kernel, CPU path and tests agree bit for bit.  With M = mats[b] (int32, Q16) and everything in int64:
//   sx = M0 x + M1 y + M2,  sy = M3 x + M4 y + M5               source pixel-index coordinates, Q16
//   x0 = sx >> 16, fx = (sx & 0xFFFF) >> 8;  y0, fy alike       arithmetic shifts
//   v  = ((256-fx)(256-fy) p00 + fx (256-fy) p01 + (256-fx) fy p10 + fx fy p11 + 32768) >> 16
//   img = lut_b[v],  tgt = float(mask[clamp((sy + 32768) >> 16)][clamp((sx + 32768) >> 16)])
// with every tap index clamped to its plane.  |sx| < 2^31 (2^15 + 2^15 + 1) for H, W < 2^15, so no int32 matrix
// overflows the int64 coordinates, and every value that becomes an address is clamped first: no matrix can make
// the kernel read outside the source planes.  An index outside [0, N) writes nothing, as in the plain gather.
#include "common.h"

#define AUG_THREADS 256
#define AUG_TX 32            // threads across a tile: 32 x 4 = 128 output pixels of a row
#define AUG_TY 8             // rows of a tile
#define AUG_MAX_DIM 32768    // H, W below this: the bound the int64 coordinates are derived for

static __device__ __forceinline__ int aug_clamp(long long v, int hi) {
  return (int)(v < 0 ? 0 : (v > (long long)hi ? (long long)hi : v));
}

// One 256-thread workgroup per (item, 128 x 8 output tile); a thread owns four consecutive x of one row, computes
// their source coordinates once and uses them for the C image planes and the mask.  VEC: one 16-byte store per
// plane (W % 4 == 0 and 16-byte aligned outputs); otherwise scalar stores with the row tail guarded.
template <bool VEC>
__global__ __launch_bounds__(AUG_THREADS) void batch_augment_u8_kernel(
    const unsigned char* __restrict__ images, const unsigned char* __restrict__ masks, const long long* __restrict__ idx,
    const int* __restrict__ mats, const float* __restrict__ luts, const float* __restrict__ unit,
    float* __restrict__ img, float* __restrict__ tgt, long long N, int C, int H, int W, int tiles_x, int tiles_y) {
  __shared__ float slut[256];
  const int per_item = tiles_x * tiles_y;
  const int b = (int)(blockIdx.x / (unsigned)per_item);
  const int t = (int)(blockIdx.x - (unsigned)b * (unsigned)per_item);
  slut[threadIdx.x] = luts != nullptr ? luts[(long)b * 256 + threadIdx.x] : unit[threadIdx.x];
  __syncthreads();
  const long long n = idx[b];
  if (n < 0 || n >= N) return;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int y = ty * AUG_TY + (int)(threadIdx.x / AUG_TX);
  const int x = (tx * AUG_TX + (int)(threadIdx.x % AUG_TX)) * 4;
  if (y >= H || x >= W) return;

  const int* m = mats + (long)b * 6;
  const long long m0 = m[0], m3 = m[3];
  long long sx = m0 * x + (long long)m[1] * y + m[2];
  long long sy = m3 * x + (long long)m[4] * y + m[5];
  int o00[4], o01[4], o10[4], o11[4], om[4];       // offsets inside one H x W plane (H W < 2^30)
  unsigned fx[4], fy[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long xi = sx >> 16, yi = sy >> 16;
    const int x0 = aug_clamp(xi, W - 1), x1 = aug_clamp(xi + 1, W - 1);
    const int y0 = aug_clamp(yi, H - 1) * W, y1 = aug_clamp(yi + 1, H - 1) * W;
    o00[j] = y0 + x0, o01[j] = y0 + x1, o10[j] = y1 + x0, o11[j] = y1 + x1;
    fx[j] = (unsigned)(sx & 0xFFFF) >> 8, fy[j] = (unsigned)(sy & 0xFFFF) >> 8;
    om[j] = aug_clamp((sy + 32768) >> 16, H - 1) * W + aug_clamp((sx + 32768) >> 16, W - 1);
    sx += m0, sy += m3;
  }

  const long plane = (long)H * W;
  const long row = (long)y * W + x;
  const int valid = VEC ? 4 : min(4, W - x);
  for (int c = 0; c <= C; ++c) {
    float o[4];
    float* d;
    if (c < C) {
      const unsigned char* s = images + ((long)n * C + c) * plane;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned wx1 = fx[j], wx0 = 256u - wx1, wy1 = fy[j], wy0 = 256u - wy1;
        const unsigned v = (wx0 * wy0 * s[o00[j]] + wx1 * wy0 * s[o01[j]] + wx0 * wy1 * s[o10[j]] +
                            wx1 * wy1 * s[o11[j]] + 32768u) >> 16;
        o[j] = slut[v > 255u ? 255u : v];            // v <= 255 by construction (the weights sum to 65536)
      }
      d = img + ((long)b * C + c) * plane + row;
    } else {
      const unsigned char* s = masks + (long)n * plane;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (float)s[om[j]];
      d = tgt + (long)b * plane + row;
    }
    if (VEC) {
      *reinterpret_cast<f32x4_t*>(d) = f32x4_t{o[0], o[1], o[2], o[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < valid) d[j] = o[j];
    }
  }
}

// luts: float32 [B][256] or null (every item then uses `unit`, the table of the plain gather)
DPA_API int dpa_batch_augment_u8(const unsigned char* images, const unsigned char* masks, const long long* idx,
                                 const int* mats, const float* luts, const float* unit, float* img, float* tgt,
                                 long long N, int B, int C, int H, int W, hipStream_t st) {
  if (N < 1 || B < 1 || C < 1 || H < 1 || W < 1) return (int)hipErrorInvalidValue;
  if (H >= AUG_MAX_DIM || W >= AUG_MAX_DIM) return (int)hipErrorInvalidValue;
  if (!images || !masks || !idx || !mats || !unit || !img || !tgt) return (int)hipErrorInvalidValue;
  const long tiles_x = ((W + 3) / 4 + AUG_TX - 1) / AUG_TX, tiles_y = (H + AUG_TY - 1) / AUG_TY;
  const long blocks = (long)B * tiles_x * tiles_y;
  if (blocks >= (1l << 31) || (long)B * (C + 1) >= (1l << 31)) return (int)hipErrorInvalidValue;
  const uintptr_t al = (uintptr_t)img | (uintptr_t)tgt;
  const bool vec = (W % 4 == 0) && (al & 15) == 0;
  if (vec)
    hipLaunchKernelGGL((batch_augment_u8_kernel<true>), dim3((unsigned)blocks), dim3(AUG_THREADS), 0, st, images, masks,
                       idx, mats, luts, unit, img, tgt, N, C, H, W, (int)tiles_x, (int)tiles_y);
  else
    hipLaunchKernelGGL((batch_augment_u8_kernel<false>), dim3((unsigned)blocks), dim3(AUG_THREADS), 0, st, images, masks,
                       idx, mats, luts, unit, img, tgt, N, C, H, W, (int)tiles_x, (int)tiles_y);
  return (int)hipGetLastError();
}
