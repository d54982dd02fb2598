// Test-time augmentation and checkpoint ensembling of predict.py (distributedpytorch_amd/predict.py): the mirrored
// views of a batch going into the network, and the average of the probability maps coming out of it.
//
//   dpa_tta_views_f32  uint8 [B][C][h][w] -> float32 [V][B][C][h][w]: view v is table[byte] mirrored by codes[v]
//                      (bit 0: x, the width; bit 1: y, the height).  One launch writes all V views: a source byte is
//                      read once, looked up once and stored to V mirrored positions.
//   dpa_tta_accum      acc float32 [B][h][w] = (first ? nothing : acc) + src mirrored back by `code`, then * scale when
//                      `last`; src is the engine's output, bf16 or float32 [B][h][w].  One launch per member in member
//                      order on one stream, so the sum is ops.kernels.tta_merge_reference's bit for bit: one rounded
//                      float32 add per member, one rounded multiply at the end (a sum times a factor has no
//                      multiply-add to contract into).  The first member is copied, not added to zero, so what `acc`
//                      held before is never read.
//
// Both are element-wise passes bound by memory.  A thread owns four neighbouring pixels of a row where the row
// width is a multiple of 4 and the pointers are aligned for it (16-byte loads and stores of float32, 8-byte loads of
// bf16, a mirrored group reversed in registers), one pixel otherwise.  A mirror is its own inverse, so "mirror" and
// "mirror back" are the same index map.  Indices are 64-bit; every x, y and plane comes from dividing an index
// below the element count, and a mirrored one is (size - 1 - that), so no argument value leads outside the planes.
#include "common.h"

#define TTA_THREADS 256
#define TTA_VMAX 4

struct TtaCodes { int c[TTA_VMAX]; };            // by value in the kernel arguments: no device table, no copy

// n: elements of one view (B * C * h * w).  VEC: a thread owns pixels x4 .. x4 + 3 of one row (w % 4 == 0).
template <bool VEC>
__global__ __launch_bounds__(TTA_THREADS) void tta_views_kernel(const unsigned char* __restrict__ src, long n, int h,
                                                                int w, const float* __restrict__ table, TtaCodes codes,
                                                                int V, float* __restrict__ dst) {
  const long i = (long)blockIdx.x * TTA_THREADS + threadIdx.x;
  if (VEC) {
    const int wg = w >> 2;
    if (i >= (n >> 2)) return;
    const int x4 = (int)(i % wg) * 4;
    const long row = i / wg;                     // plane * h + y
    const int y = (int)(row % h);
    const long top = row - y;                    // plane * h
    const unsigned u = *reinterpret_cast<const unsigned*>(src + i * 4);
    const f32x4_t f = {table[u & 255u], table[(u >> 8) & 255u], table[(u >> 16) & 255u], table[u >> 24]};
    const f32x4_t r = {f[3], f[2], f[1], f[0]};
#pragma unroll
    for (int v = 0; v < TTA_VMAX; ++v)
      if (v < V) {
        const int c = codes.c[v];
        const int yy = (c & 2) ? h - 1 - y : y;
        const int xx = (c & 1) ? w - 4 - x4 : x4;
        *reinterpret_cast<f32x4_t*>(dst + v * n + (top + yy) * w + xx) = (c & 1) ? r : f;
      }
  } else {
    if (i >= n) return;
    const int x = (int)(i % w);
    const long row = i / w;
    const int y = (int)(row % h);
    const long top = row - y;
    const float f = table[src[i]];
#pragma unroll
    for (int v = 0; v < TTA_VMAX; ++v)
      if (v < V) {
        const int c = codes.c[v];
        const int yy = (c & 2) ? h - 1 - y : y;
        const int xx = (c & 1) ? w - 1 - x : x;
        dst[v * n + (top + yy) * w + xx] = f;
      }
  }
}

// n: elements of acc (B * h * w).  A thread owns acc[i] (VEC: acc[4 i .. 4 i + 3]) and reads the mirrored source.
template <bool VEC, bool BF16>
__global__ __launch_bounds__(TTA_THREADS) void tta_accum_kernel(const void* __restrict__ src, int code, long n, int h,
                                                                int w, float* __restrict__ acc, int first, int last,
                                                                float scale) {
  const long i = (long)blockIdx.x * TTA_THREADS + threadIdx.x;
  if (VEC) {
    const int wg = w >> 2;
    if (i >= (n >> 2)) return;
    const int x4 = (int)(i % wg) * 4;
    const long row = i / wg;                     // image * h + y
    const int y = (int)(row % h);
    const int yy = (code & 2) ? h - 1 - y : y;
    const int xx = (code & 1) ? w - 4 - x4 : x4;
    const long s = (row - y + yy) * w + xx;
    f32x4_t q;
    if (BF16) {
      const u32x2_t u = *reinterpret_cast<const u32x2_t*>(static_cast<const bf16_t*>(src) + s);
      q = f32x4_t{lo_bf(u[0]), hi_bf(u[0]), lo_bf(u[1]), hi_bf(u[1])};
    } else {
      q = *reinterpret_cast<const f32x4_t*>(static_cast<const float*>(src) + s);
    }
    if (code & 1) q = f32x4_t{q[3], q[2], q[1], q[0]};
    f32x4_t* out = reinterpret_cast<f32x4_t*>(acc + i * 4);
    f32x4_t a = q;
    if (!first) a = *out + q;
    if (last) a = a * scale;
    *out = a;
  } else {
    if (i >= n) return;
    const int x = (int)(i % w);
    const long row = i / w;
    const int y = (int)(row % h);
    const int yy = (code & 2) ? h - 1 - y : y;
    const int xx = (code & 1) ? w - 1 - x : x;
    const long s = (row - y + yy) * w + xx;
    const float q = BF16 ? bf2f(static_cast<const bf16_t*>(src)[s]) : static_cast<const float*>(src)[s];
    float a = q;
    if (!first) a = acc[i] + q;
    if (last) a = a * scale;
    acc[i] = a;
  }
}

// a * b * c * d for positive ints, or -1 where it reaches 2^31
static long tta_count(int a, int b, int c, int d) {
  long n = a;
  const int rest[3] = {b, c, d};
  for (int k = 0; k < 3; ++k) {
    n *= rest[k];                                // < 2^31 * 2^31
    if (n >= (1l << 31)) return -1;
  }
  return n;
}

// `codes` is a HOST array of V ints: it travels in the kernel arguments.
DPA_API int dpa_tta_views_f32(const unsigned char* src, int B, int C, int h, int w, const float* table,
                              const int* codes, int V, float* dst, hipStream_t st) {
  if (B < 1 || C < 1 || h < 1 || w < 1 || V < 1 || V > TTA_VMAX) return (int)hipErrorInvalidValue;
  if (!src || !table || !codes || !dst) return (int)hipErrorInvalidValue;
  if (((uintptr_t)table & 3) != 0 || ((uintptr_t)dst & 3) != 0) return (int)hipErrorInvalidValue;
  const long n = tta_count(B, C, h, w);
  if (n < 0) return (int)hipErrorInvalidValue;
  TtaCodes cd;
  for (int v = 0; v < TTA_VMAX; ++v) {
    cd.c[v] = v < V ? codes[v] : 0;
    if (cd.c[v] < 0 || cd.c[v] > 3) return (int)hipErrorInvalidValue;
  }
  // n % 4 == 0 with w % 4 == 0, so every view and every group of four starts aligned
  const bool vec = (w & 3) == 0 && ((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 15) == 0;
  const long items = vec ? n >> 2 : n;
  const unsigned grid = (unsigned)((items + TTA_THREADS - 1) / TTA_THREADS);         // < 2^23 + 1
  if (vec)
    hipLaunchKernelGGL((tta_views_kernel<true>), dim3(grid), dim3(TTA_THREADS), 0, st, src, n, h, w, table, cd, V, dst);
  else
    hipLaunchKernelGGL((tta_views_kernel<false>), dim3(grid), dim3(TTA_THREADS), 0, st, src, n, h, w, table, cd, V, dst);
  return (int)hipGetLastError();
}

DPA_API int dpa_tta_accum(const void* src, int src_is_bf16, int code, int B, int h, int w, float* acc, int first,
                          int last, float scale, hipStream_t st) {
  if (B < 1 || h < 1 || w < 1 || code < 0 || code > 3) return (int)hipErrorInvalidValue;
  if (!src || !acc) return (int)hipErrorInvalidValue;
  const bool bf = src_is_bf16 != 0;
  if (((uintptr_t)acc & 3) != 0 || ((uintptr_t)src & (bf ? 1 : 3)) != 0) return (int)hipErrorInvalidValue;
  const long n = tta_count(B, h, w, 1);
  if (n < 0) return (int)hipErrorInvalidValue;
  const bool vec = (w & 3) == 0 && ((uintptr_t)acc & 15) == 0 && ((uintptr_t)src & (bf ? 7 : 15)) == 0;
  const long items = vec ? n >> 2 : n;
  const unsigned grid = (unsigned)((items + TTA_THREADS - 1) / TTA_THREADS);
#define TTA_ACCUM(VEC, BF)                                                                                          \
  hipLaunchKernelGGL((tta_accum_kernel<VEC, BF>), dim3(grid), dim3(TTA_THREADS), 0, st, src, code, n, h, w, acc,   \
                     first != 0, last != 0, scale)
  if (vec) {
    if (bf) TTA_ACCUM(true, true); else TTA_ACCUM(true, false);
  } else {
    if (bf) TTA_ACCUM(false, true); else TTA_ACCUM(false, false);
  }
#undef TTA_ACCUM
  return (int)hipGetLastError();
}
