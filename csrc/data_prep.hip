// Data preparation for HBM-resident folder datasets (data/device_folder.py).
//
//   dpa_resize_bicubic_u8  PIL Image.resize(BICUBIC) for 8-bit L / RGB images, bit for bit: PIL's resampler
//                          (Resample.c) is integer arithmetic on per-axis tables of int32 coefficients with 22
//                          fractional bits; the tables are built on the host in float64 (ops/kernels.py:
//                          bicubic_table) and the kernel does the integer part: per pass
//                          clip8(((1 << 21) + sum pixel * coef) >> 22), horizontal pass first, rounded to uint8,
//                          then the vertical pass.  Both passes in one kernel: a workgroup owns TH x TW output
//                          pixels, runs the horizontal pass for the source rows its tile needs into LDS (uint8)
//                          and the vertical pass out of LDS.  Interleaved [H][W][C] in, planar [C][H][W] out.
//                          An axis whose sizes are equal carries the identity table (one coefficient 1 << 22,
//                          which the pass reproduces exactly), so "pass skipped" needs no second kernel.
//   dpa_resize_nearest_u8  PIL NEAREST for single-channel 8-bit masks from per-axis source-index tables, then
//                          the dataset's mask rule on the resized mask: maximum > 1 -> value > 127.
//   dpa_batch_gather_u8    the per-step batch: gather by index, optional horizontal flip, uint8 -> float32
//                          through a 256-entry table (float32(k / 255.0) is not float32(k) * float32(1/255)).
//
// Every table entry that becomes an address is clamped in the kernel: the launchers cannot see the device
// tables, so a bad table gives wrong pixels, never an access outside the source, the tile or the output.
#include "common.h"

#define DP_PREC 22
#define DP_LDS_BYTES 49152
#define DP_THREADS 256

static __device__ __forceinline__ int dp_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static __device__ __forceinline__ unsigned char dp_clip8(int acc) {
  return (unsigned char)dp_clamp(acc >> DP_PREC, 0, 255);
}

// ------------------------------------------------------------------------------ bicubic resize
// hb / vb: int32 [out][2] = (first source index, tap count); hc / vc: int32 [out][k] coefficients.
__global__ __launch_bounds__(DP_THREADS) void resize_bicubic_u8_kernel(
    const unsigned char* __restrict__ src, int Hs, int Ws, int C, unsigned char* __restrict__ dst, int Ho, int Wo,
    const int* __restrict__ hb, const int* __restrict__ hc, int kh, const int* __restrict__ vb,
    const int* __restrict__ vc, int kv, int TH, int TW, int Rcap) {
  extern __shared__ unsigned char tile[];            // [Rcap][TW * C]: horizontally resized source rows
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int tw = min(TW, Wo - x0), th = min(TH, Ho - y0);
  if (tw <= 0 || th <= 0) return;
  // source rows of the tile: the bounds are monotone in y, so first row of y0 .. last row of y0 + th - 1
  const int r0 = dp_clamp(vb[2 * y0], 0, Hs);
  const int ylast = y0 + th - 1;
  const int rl = dp_clamp(vb[2 * ylast], 0, Hs);
  const int r1 = rl + dp_clamp(vb[2 * ylast + 1], 0, Hs - rl);
  const int R = dp_clamp(r1 - r0, 0, Rcap);
  const int rowb = tw * C, pitch = TW * C;

  for (int i = tid; i < R * rowb; i += DP_THREADS) {
    const int r = i / rowb, j = i - r * rowb;
    const int x = j / C, c = j - x * C;
    const int xo = x0 + x;
    const int xm = dp_clamp(hb[2 * xo], 0, Ws);
    const int n = dp_clamp(hb[2 * xo + 1], 0, min(kh, Ws - xm));
    const unsigned char* p = src + ((long)(r0 + r) * Ws + xm) * C + c;
    const int* k = hc + (long)xo * kh;
    int acc = 1 << (DP_PREC - 1);
    for (int t = 0; t < n; ++t) acc += (int)p[t * C] * k[t];
    tile[r * pitch + j] = dp_clip8(acc);
  }
  __syncthreads();

  const int per = th * tw;
  for (int i = tid; i < C * per; i += DP_THREADS) {
    const int c = i / per, q = i - c * per;
    const int y = q / tw, x = q - y * tw;
    const int yo = y0 + y;
    const int ym = dp_clamp(vb[2 * yo], 0, Hs);
    const int rr = dp_clamp(ym - r0, 0, R);
    const int n = dp_clamp(vb[2 * yo + 1], 0, min(kv, R - rr));
    const unsigned char* p = tile + rr * pitch + x * C + c;
    const int* k = vc + (long)yo * kv;
    int acc = 1 << (DP_PREC - 1);
    for (int t = 0; t < n; ++t) acc += (int)p[t * pitch] * k[t];
    dst[((long)c * Ho + yo) * Wo + x0 + x] = dp_clip8(acc);
  }
}

// PIL's table width for one axis (Resample.c precompute_coeffs); 1 for the identity table of a skipped pass
static int dp_ksize(int in, int out) {
  if (in == out) return 1;
  const double scale = (double)in / (double)out;
  const double support = 2.0 * (scale < 1.0 ? 1.0 : scale);
  return (int)ceil(support) * 2 + 1;
}

// most source rows any TH consecutive output rows read: x_max(y + TH - 1) - x_min(y) <= (TH-1) scale + 2 support + 1
static long dp_rows_bound(int in, int out, int TH) {
  if (in == out) return TH < in ? TH : in;
  const double scale = (double)in / (double)out;
  const double support = 2.0 * (scale < 1.0 ? 1.0 : scale);
  const double r = floor((TH - 1) * scale + 2.0 * support + 1.0) + 1.0;
  return r < (double)in ? (long)r : (long)in;
}

DPA_API int dpa_resize_bicubic_u8(const unsigned char* src, int Hs, int Ws, int C, unsigned char* dst, int Ho, int Wo,
                                  const int* hb, const int* hc, int kh, const int* vb, const int* vc, int kv,
                                  hipStream_t st) {
  if (Hs < 1 || Ws < 1 || Ho < 1 || Wo < 1 || (C != 1 && C != 3)) return (int)hipErrorInvalidValue;
  if (!src || !dst || !hb || !hc || !vb || !vc) return (int)hipErrorInvalidValue;
  if ((long)Hs * Ws * C >= (1l << 31) || (long)Ho * Wo * C >= (1l << 31)) return (int)hipErrorInvalidValue;
  if (kh != dp_ksize(Ws, Wo) || kv != dp_ksize(Hs, Ho)) return (int)hipErrorInvalidValue;
  // tile: the widest, then the tallest, whose horizontally resized source rows fit in LDS
  static const int tws[3] = {64, 32, 16}, ths[6] = {32, 16, 8, 4, 2, 1};
  int TW = 0, TH = 0;
  long R = 0;
  for (int a = 0; a < 3 && !TW; ++a)
    for (int b = 0; b < 6; ++b) {
      const long rows = dp_rows_bound(Hs, Ho, ths[b]);
      if (rows * tws[a] * C <= DP_LDS_BYTES) {
        TW = tws[a], TH = ths[b], R = rows;
        break;
      }
    }
  if (!TW) return (int)hipErrorInvalidValue;       // extreme down-scaling: the caller resizes on the CPU
  const long gx = (Wo + TW - 1) / TW, gy = (Ho + TH - 1) / TH;
  if (gy > 65535 || gx > (1l << 30)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(resize_bicubic_u8_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(DP_THREADS),
                     (size_t)(R * TW * C), st, src, Hs, Ws, C, dst, Ho, Wo, hb, hc, kh, vb, vc, kv, TH, TW, (int)R);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------ nearest resize + mask rule
// xi[Wo] / yi[Ho]: source index per output column / row.  The maximum of the resized mask goes to *vmax.
__global__ __launch_bounds__(DP_THREADS) void resize_nearest_u8_kernel(
    const unsigned char* __restrict__ src, int Hs, int Ws, unsigned char* __restrict__ dst, int Ho, int Wo,
    const int* __restrict__ xi, const int* __restrict__ yi, int* __restrict__ vmax) {
  const long tot = (long)Ho * Wo;
  int m = 0;
  for (long i = (long)blockIdx.x * DP_THREADS + threadIdx.x; i < tot; i += (long)gridDim.x * DP_THREADS) {
    const int y = (int)(i / Wo), x = (int)(i - (long)y * Wo);
    const int sy = dp_clamp(yi[y], 0, Hs - 1), sx = dp_clamp(xi[x], 0, Ws - 1);
    const int v = src[(long)sy * Ws + sx];
    dst[i] = (unsigned char)v;
    m = max(m, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(vmax, m);
}

// BasicDataset.preprocess: a mask whose maximum exceeds 1 (0/255 files) becomes value > 127
__global__ __launch_bounds__(DP_THREADS) void mask_rule_u8_kernel(unsigned char* __restrict__ m, long tot,
                                                                  const int* __restrict__ vmax) {
  if (*vmax <= 1) return;
  for (long i = (long)blockIdx.x * DP_THREADS + threadIdx.x; i < tot; i += (long)gridDim.x * DP_THREADS)
    m[i] = m[i] > 127 ? 1 : 0;
}

// vmax: one int32 of device scratch (zeroed here); rule != 0 applies the mask rule after the resize
DPA_API int dpa_resize_nearest_u8(const unsigned char* src, int Hs, int Ws, unsigned char* dst, int Ho, int Wo,
                                  const int* xi, const int* yi, int* vmax, int rule, hipStream_t st) {
  if (Hs < 1 || Ws < 1 || Ho < 1 || Wo < 1) return (int)hipErrorInvalidValue;
  if (!src || !dst || !xi || !yi || !vmax) return (int)hipErrorInvalidValue;
  if ((long)Hs * Ws >= (1l << 31) || (long)Ho * Wo >= (1l << 31)) return (int)hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(vmax, 0, sizeof(int), st);
  if (e != hipSuccess) return (int)e;
  const long tot = (long)Ho * Wo;
  const int grid = dpa_grid(tot, DP_THREADS, 2048);
  hipLaunchKernelGGL(resize_nearest_u8_kernel, dim3(grid), dim3(DP_THREADS), 0, st, src, Hs, Ws, dst, Ho, Wo, xi, yi, vmax);
  if (rule) hipLaunchKernelGGL(mask_rule_u8_kernel, dim3(grid), dim3(DP_THREADS), 0, st, dst, tot, vmax);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------ batch gather
// Planes: (b, c) for c < C from the images through the table, (b, C) from the masks as float(value).
// VEC: 16 pixels per thread, one 16-byte load and four 16-byte stores; a flipped row reads the mirrored chunk
// and reverses its bytes.  An index outside [0, N) writes nothing.
template <bool VEC>
__global__ __launch_bounds__(DP_THREADS) void batch_gather_u8_kernel(
    const unsigned char* __restrict__ images, const unsigned char* __restrict__ masks, const long long* __restrict__ idx,
    const unsigned char* __restrict__ flip, const float* __restrict__ lut, float* __restrict__ img, float* __restrict__ tgt,
    long long N, int B, int C, int H, int W) {
  __shared__ float slut[256];
  slut[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const int Wc = VEC ? W / 16 : W;
  const long tot = (long)B * (C + 1) * H * Wc;
  for (long i = (long)blockIdx.x * DP_THREADS + threadIdx.x; i < tot; i += (long)gridDim.x * DP_THREADS) {
    const int xc = (int)(i % Wc);
    const long t = i / Wc;
    const int y = (int)(t % H);
    const int pl = (int)(t / H);
    const int b = pl / (C + 1), c = pl - b * (C + 1);
    const long long n = idx[b];
    if (n < 0 || n >= N) continue;
    const bool f = flip != nullptr && flip[b] != 0;
    const bool is_img = c < C;
    const unsigned char* s = is_img ? images + (((long)n * C + c) * H + y) * W : masks + ((long)n * H + y) * W;
    float* d = is_img ? img + (((long)b * C + c) * H + y) * W : tgt + ((long)b * H + y) * W;
    if (VEC) {
      const int sx = f ? W - 16 - xc * 16 : xc * 16;
      const u32x4_t v = *reinterpret_cast<const u32x4_t*>(s + sx);
      float o[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const unsigned k = (v[j >> 2] >> ((j & 3) * 8)) & 255u;
        o[j] = is_img ? slut[k] : (float)k;
      }
      f32x4_t* dv = reinterpret_cast<f32x4_t*>(d + xc * 16);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        dv[q] = f ? f32x4_t{o[15 - 4 * q], o[14 - 4 * q], o[13 - 4 * q], o[12 - 4 * q]}
                  : f32x4_t{o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]};
    } else {
      const unsigned k = s[f ? W - 1 - xc : xc];
      d[xc] = is_img ? slut[k] : (float)k;
    }
  }
}

DPA_API int dpa_batch_gather_u8(const unsigned char* images, const unsigned char* masks, const long long* idx,
                                const unsigned char* flip, const float* lut, float* img, float* tgt, long long N, int B,
                                int C, int H, int W, hipStream_t st) {
  if (N < 1 || B < 1 || C < 1 || H < 1 || W < 1) return (int)hipErrorInvalidValue;
  if (!images || !masks || !idx || !lut || !img || !tgt) return (int)hipErrorInvalidValue;
  if ((long)B * (C + 1) >= (1l << 31) || (long)H * W >= (1l << 31)) return (int)hipErrorInvalidValue;
  const uintptr_t al = (uintptr_t)images | (uintptr_t)masks | (uintptr_t)img | (uintptr_t)tgt;
  const bool vec = (W % 16 == 0) && (al & 15) == 0;
  const long tot = (long)B * (C + 1) * H * (vec ? W / 16 : W);
  const int grid = dpa_grid(tot, DP_THREADS, 16384);
  if (vec)
    hipLaunchKernelGGL((batch_gather_u8_kernel<true>), dim3(grid), dim3(DP_THREADS), 0, st, images, masks, idx, flip, lut,
                       img, tgt, N, B, C, H, W);
  else
    hipLaunchKernelGGL((batch_gather_u8_kernel<false>), dim3(grid), dim3(DP_THREADS), 0, st, images, masks, idx, flip, lut,
                       img, tgt, N, B, C, H, W);
  return (int)hipGetLastError();
}
