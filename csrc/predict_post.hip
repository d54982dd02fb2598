// Post-processing of predict.py (distributedpytorch_amd/predict.py): from the network's probability map to a
// full-size mask and its run-length list, without the full mask leaving the GPU.
//
//   dpa_prob_to_mask_u8  float32 probabilities [B][h][w] -> uint8 mask [B][H][W] = (resized > threshold) ? value : 0,
//                        resized bit-equal to PIL Image.resize((W, H), BILINEAR) of a mode "F" image (Resample.c,
//                        the 32bpc passes): per-axis tables of float64 coefficients built on the host
//                        (ops/kernels.py: bilinear_table), per pass ss = 0.0; ss += double(pixel) * k[j] in tap order,
//                        rounded to float32; horizontal pass first.  Both passes in one kernel: a thread owns one
//                        output column and walks down 16 output rows; it keeps the horizontal sums (float32) of the
//                        source rows its current output row reads in a register window and computes a source row
//                        once, when the window reaches it (2x up-scaling: one new source row per two output rows).
//                        The build contracts a * b + c into an fma and PIL's double sums are a rounded multiply,
//                        then a rounded add: contraction is switched off in the walk (by a pragma, which the build honours
//                        for this file: tools/build_hip.py FILE_FLAGS).  An axis whose sizes are
//                        equal carries the identity table (one coefficient 1.0: 0.0 + p * 1.0 == p), so "pass
//                        skipped" needs no second kernel.
//   dpa_prob_score       the same resize, compared with up to 8 thresholds and with ground-truth bytes [B][H][W]
//                        (a pixel is truth where its byte > cut[b]) and counted instead of stored: int64
//                        [B][1 + 2T] = (truth, pred_0, inter_0, ...), what the Dice coefficient and the IoU of the
//                        full-size masks at every threshold are made of, without a mask being written.
//   dpa_mask_rle         uint8 masks [B][H][W] -> the maximal runs of non-zero bytes of each flattened image as
//                        (start, length), start 1-indexed, ascending; counts[b] is the true number of runs, nothing
//                        is written past cap.  With a zero in front of the first pixel and behind the last, the
//                        positions where "non-zero" changes alternate start, end, start, end: the k-th of them is
//                        element k of the flattened run list.  Four kernels: count the changes per tile of 4096
//                        pixels; exclusive scan over the tiles of an image; recompute and write position + 1 at the
//                        scanned index; length = end - start.  No atomics: the order is the scan's.
//
// Every table entry that becomes an address is clamped in the kernel, as in data_prep.hip.
#include "common.h"

#define PP_THREADS 256
#define PP_KMAX 9                               // taps per axis: down-scaling up to 4x
#define PP_ROWS 16                              // output rows one wave walks down
#define RLE_SPAN 16                             // pixels per thread
#define RLE_TILE (PP_THREADS * RLE_SPAN)        // pixels per workgroup

static __device__ __forceinline__ int pp_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ------------------------------------------------------------------------------ bilinear resize + threshold
// hb / vb: int32 [out][2] = (first source index, tap count); hc / vc: float64 [out][k] coefficients.
// Workgroup: 64 output columns x 4 chunks of PP_ROWS output rows (one wave per chunk), grid.z = image.
// KM: the taps per axis this instantiation holds in registers (3: up-scaling and identity; 9: down-scaling).
// Everything that depends on the output row alone is uniform in a wave; only the column differs between lanes.
//
// pp_walk is the resize itself, shared by the mask kernel and the scoring kernel: output column xc (< W) of image
// `img`, output rows ya .. yb - 1, emit(y, value) per row with value the float32 PIL stores.
template <int KM, class Emit>
static __device__ __forceinline__ void pp_walk(const float* __restrict__ img, int h, int w, int xc, int ya, int yb,
                                               const int* __restrict__ hb, const double* __restrict__ hc, int kh,
                                               const int* __restrict__ vb, const double* __restrict__ vc, int kv,
                                               Emit emit) {
#pragma clang fp contract(off)
  // this column's horizontal taps
  const int xm = pp_clamp(hb[2 * xc], 0, w);
  const int nh = pp_clamp(hb[2 * xc + 1], 0, min(min(kh, KM), w - xm));
  double kx[KM];
#pragma unroll
  for (int t = 0; t < KM; ++t) kx[t] = t < nh ? hc[(long)xc * kh + t] : 0.0;

  // win[r]: the horizontal sum of source row wbase + r, for r < wcount
  float win[KM];
#pragma unroll
  for (int r = 0; r < KM; ++r) win[r] = 0.f;
  int wbase = 0, wcount = 0;
  for (int y = ya; y < yb; ++y) {
    const int ym = pp_clamp(vb[2 * y], 0, h);
    const int nv = pp_clamp(vb[2 * y + 1], 0, min(min(kv, KM), h - ym));
    if (ym < wbase || ym >= wbase + wcount) wbase = ym, wcount = 0;      // nothing to keep (or a table that goes back)
    while (wbase < ym) {                                                 // drop the rows above this output row's first
#pragma unroll
      for (int r = 0; r + 1 < KM; ++r) win[r] = win[r + 1];
      ++wbase, --wcount;
    }
    while (wcount < nv) {                                                // wbase + wcount < ym + nv <= h
      const float* p = img + (long)(wbase + wcount) * w + xm;
      double sh = 0.0;
#pragma unroll
      for (int t = 0; t < KM; ++t)
        if (t < nh) {
          const double m = (double)p[t] * kx[t];
          sh = sh + m;
        }
      const float row = (float)sh;               // the horizontal pass stores float32
#pragma unroll
      for (int r = 0; r < KM; ++r)
        if (r == wcount) win[r] = row;
      ++wcount;
    }
    const double* ky = vc + (long)y * kv;
    double sv = 0.0;
#pragma unroll
    for (int r = 0; r < KM; ++r)
      if (r < nv) {
        const double m = (double)win[r] * ky[r];
        sv = sv + m;
      }
    emit(y, (float)sv);
  }
}

template <int KM>
__global__ __launch_bounds__(PP_THREADS) void prob_to_mask_u8_kernel(
    const float* __restrict__ probs, int h, int w, unsigned char* __restrict__ dst, int H, int W,
    const int* __restrict__ hb, const double* __restrict__ hc, int kh, const int* __restrict__ vb,
    const double* __restrict__ vc, int kv, float threshold, unsigned value) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int chunk = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ya = (blockIdx.y * 4 + chunk) * PP_ROWS;
  if (ya >= H) return;                           // the whole wave; there is no barrier in this kernel
  const int yb = min(ya + PP_ROWS, H);
  const bool live = x < W;
  const int xc = live ? x : W - 1;               // lanes right of the image compute its last column, store nothing
  unsigned char* out = dst + (long)blockIdx.z * H * W;
  pp_walk<KM>(probs + (long)blockIdx.z * h * w, h, w, xc, ya, yb, hb, hc, kh, vb, vc, kv, [&](int y, float v) {
    if (live) out[(long)y * W + x] = (unsigned char)(v > threshold ? value : 0u);
  });
}

// ------------------------------------------------------------------------------ resize + threshold + count
// The mask kernel's grid and walk, but nothing is stored per pixel: a lane compares its 16 values with up to 8
// thresholds and with the ground truth (byte > cut[image]) and counts.  A workgroup covers at most 64 x 64 = 4096
// pixels, so a pair (pred_t, inter_t) is counted in the two halves of one 32-bit register: + 1 for "predicted",
// + 0x10000 more where the pixel is truth as well.  Lanes right of the image and rows below it add nothing.  The
// wave sums by shuffles, the four waves through LDS, and the workgroup writes row (blockIdx.y * gridDim.x +
// blockIdx.x) of work [B][blocks][1 + 2T] = (truth, pred_0, inter_0, ...) with plain stores; score_sum_kernel adds
// an image's rows up.  No atomics, nothing to zero.
struct PPThresholds { float v[8]; };             // by value in the kernel arguments: no device table, no copy

static __device__ __forceinline__ unsigned pp_wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;                                      // lane 0 holds the sum
}

// NT: the thresholds this instantiation counts (1 or 8); thr.v[t] for T <= t < NT is +infinity and counts nothing.
template <int KM, int NT>
__global__ __launch_bounds__(PP_THREADS) void prob_score_kernel(
    const float* __restrict__ probs, int h, int w, const unsigned char* __restrict__ truth,
    const int* __restrict__ cut, int H, int W, const int* __restrict__ hb, const double* __restrict__ hc, int kh,
    const int* __restrict__ vb, const double* __restrict__ vc, int kv, PPThresholds thr, int T,
    unsigned* __restrict__ work) {
  __shared__ unsigned red[4][NT + 1];
  const int lane = threadIdx.x & 63;
  const int x = blockIdx.x * 64 + lane;
  const int chunk = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ya = min((int)(blockIdx.y * 4 + chunk) * PP_ROWS, H);   // a wave below the image walks no row and still
  const int yb = min(ya + PP_ROWS, H);                         // reaches the barrier
  const bool live = x < W;
  const int xc = live ? x : W - 1;
  const unsigned char* tr = truth + (long)blockIdx.z * H * W;
  const int cutv = cut[blockIdx.z];

  // bit r: the pixel of row ya + r is truth.  Loaded up front, so the bytes arrive while the walk computes.
  unsigned tbits = 0;
#pragma unroll
  for (int r = 0; r < PP_ROWS; ++r)
    if (live && ya + r < yb) tbits |= ((int)tr[(long)(ya + r) * W + x] > cutv ? 1u : 0u) << r;

  unsigned acc[NT];                              // low half: pred_t, high half: inter_t
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = 0u;
  pp_walk<KM>(probs + (long)blockIdx.z * h * w, h, w, xc, ya, yb, hb, hc, kh, vb, vc, kv, [&](int y, float v) {
    const unsigned inc = live ? 1u + (((tbits >> (y - ya)) & 1u) << 16) : 0u;
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] += v > thr.v[t] ? inc : 0u;
  });

  const unsigned nt = pp_wave_sum((unsigned)__popc(tbits));
  if (lane == 0) red[chunk][0] = nt;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const unsigned s = pp_wave_sum(acc[t]);      // at most 1024 in either half
    if (lane == 0) red[chunk][1 + t] = s;
  }
  __syncthreads();
  const int n = 1 + 2 * T, k = threadIdx.x;
  if (k < n) {
    const int c = (k + 1) >> 1;                  // red column: 0 truth; 1 + t for pred_t (odd k) and inter_t (even k)
    const unsigned s = red[0][c] + red[1][c] + red[2][c] + red[3][c];
    const long row = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    work[row * n + k] = k == 0 ? s : ((k & 1) ? (s & 0xffffu) : (s >> 16));
  }
}

// one workgroup per image: counts [B][n] = the sums over the image's `blocks` rows of work, in int64
__global__ __launch_bounds__(PP_THREADS) void score_sum_kernel(const unsigned* __restrict__ work, int blocks, int n,
                                                               long long* __restrict__ counts) {
  __shared__ long long red[4][17];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned* wk = work + (long)blockIdx.x * blocks * n;
  long long acc[17];
#pragma unroll
  for (int k = 0; k < 17; ++k) acc[k] = 0;
  for (int r = threadIdx.x; r < blocks; r += PP_THREADS)
#pragma unroll
    for (int k = 0; k < 17; ++k)
      if (k < n) acc[k] += (long long)wk[(long)r * n + k];
#pragma unroll
  for (int k = 0; k < 17; ++k) {
    long long v = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) red[wv][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < n) {
    const int k = threadIdx.x;
    counts[(long)blockIdx.x * n + k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
  }
}

// PIL's table width for one axis with the triangle filter (support 1); 1 for the identity table of a skipped pass
static int pp_ksize(int in, int out) {
  if (in == out) return 1;
  const double scale = (double)in / (double)out;
  const double support = scale < 1.0 ? 1.0 : scale;
  return (int)ceil(support) * 2 + 1;
}

DPA_API int dpa_prob_to_mask_u8(const float* probs, int B, int h, int w, unsigned char* dst, int H, int W,
                                const int* hb, const double* hc, int kh, const int* vb, const double* vc, int kv,
                                float threshold, int value, hipStream_t st) {
  if (B < 1 || h < 1 || w < 1 || H < 1 || W < 1 || value < 0 || value > 255) return (int)hipErrorInvalidValue;
  if (!probs || !dst || !hb || !hc || !vb || !vc) return (int)hipErrorInvalidValue;
  if ((long)h * w >= (1l << 31) || (long)H * W >= (1l << 31)) return (int)hipErrorInvalidValue;
  if (kh != pp_ksize(w, W) || kv != pp_ksize(h, H)) return (int)hipErrorInvalidValue;
  if (kh > PP_KMAX || kv > PP_KMAX) return (int)hipErrorInvalidValue;       // the caller resizes on the host
  const long gx = ((long)W + 63) / 64, gy = ((long)H + 4 * PP_ROWS - 1) / (4 * PP_ROWS);
  if (gy > 65535 || B > 65535) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)B);
  if (kh <= 3 && kv <= 3)
    hipLaunchKernelGGL((prob_to_mask_u8_kernel<3>), grid, dim3(PP_THREADS), 0, st, probs, h, w, dst, H, W, hb, hc, kh,
                       vb, vc, kv, threshold, (unsigned)value);
  else
    hipLaunchKernelGGL((prob_to_mask_u8_kernel<PP_KMAX>), grid, dim3(PP_THREADS), 0, st, probs, h, w, dst, H, W, hb, hc,
                       kh, vb, vc, kv, threshold, (unsigned)value);
  return (int)hipGetLastError();
}

// workgroups (= rows of `work`) per image of dpa_prob_score; 0 for sizes the launcher rejects
DPA_API int dpa_prob_score_blocks(int H, int W) {
  if (H < 1 || W < 1 || (long)H * W >= (1l << 31)) return 0;
  const long gx = ((long)W + 63) / 64, gy = ((long)H + 4 * PP_ROWS - 1) / (4 * PP_ROWS);
  return gy > 65535 ? 0 : (int)(gx * gy);        // H * W < 2^31: gx * gy < 2^20 + gx + gy
}

// counts int64 [B][1 + 2T] = (truth, pred_0, inter_0, ...): truth pixels (byte > cut[b]), pixels whose resized
// probability is > thresholds[t], and those that are both.  `thresholds` is a HOST array: it travels in the
// kernel arguments, so the two launches can be captured in a graph.
DPA_API int dpa_prob_score(const float* probs, int B, int h, int w, const unsigned char* truth, const int* cut, int H,
                           int W, const int* hb, const double* hc, int kh, const int* vb, const double* vc, int kv,
                           const float* thresholds, int T, long long* counts, unsigned* work, long long work_elems,
                           hipStream_t st) {
  if (B < 1 || h < 1 || w < 1 || H < 1 || W < 1 || T < 1 || T > 8) return (int)hipErrorInvalidValue;
  if (!probs || !truth || !cut || !hb || !hc || !vb || !vc || !thresholds || !counts || !work)
    return (int)hipErrorInvalidValue;
  if ((long)h * w >= (1l << 31) || (long)H * W >= (1l << 31)) return (int)hipErrorInvalidValue;
  if (kh != pp_ksize(w, W) || kv != pp_ksize(h, H)) return (int)hipErrorInvalidValue;
  if (kh > PP_KMAX || kv > PP_KMAX) return (int)hipErrorInvalidValue;       // the caller scores on the host
  const int blocks = dpa_prob_score_blocks(H, W);
  if (blocks < 1 || B > 65535) return (int)hipErrorInvalidValue;
  const int n = 1 + 2 * T;
  if (work_elems < (long long)B * blocks * n) return (int)hipErrorInvalidValue;
  PPThresholds thr;
  for (int t = 0; t < 8; ++t) thr.v[t] = t < T ? thresholds[t] : INFINITY;
  const unsigned gx = (unsigned)(((long)W + 63) / 64);
  const dim3 grid(gx, (unsigned)blocks / gx, (unsigned)B);
#define PP_SCORE(KM, NT)                                                                                              \
  hipLaunchKernelGGL((prob_score_kernel<KM, NT>), grid, dim3(PP_THREADS), 0, st, probs, h, w, truth, cut, H, W, hb,  \
                     hc, kh, vb, vc, kv, thr, T, work)
  const bool small = kh <= 3 && kv <= 3;
  if (T == 1) {
    if (small) PP_SCORE(3, 1); else PP_SCORE(PP_KMAX, 1);
  } else {
    if (small) PP_SCORE(3, 8); else PP_SCORE(PP_KMAX, 8);
  }
#undef PP_SCORE
  const int err = (int)hipGetLastError();
  if (err) return err;
  hipLaunchKernelGGL(score_sum_kernel, dim3(B), dim3(PP_THREADS), 0, st, (const unsigned*)work, blocks, n, counts);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------ run-length encoding
// Bit j of the result: "non-zero" changes between pixels p0 + j - 1 and p0 + j of image m [N]; pixels -1 and >= N
// count as zero, so the end of a run that reaches the last pixel shows at position N.
static __device__ __forceinline__ unsigned rle_changes(const unsigned char* __restrict__ m, long N, long p0, bool vec) {
  unsigned nz = 0;
  if (vec && p0 + RLE_SPAN <= N) {
    const u32x4_t v = *reinterpret_cast<const u32x4_t*>(m + p0);
#pragma unroll
    for (int j = 0; j < RLE_SPAN; ++j) nz |= (((v[j >> 2] >> ((j & 3) * 8)) & 255u) != 0u ? 1u : 0u) << j;
  } else {
    for (int j = 0; j < RLE_SPAN; ++j)
      if (p0 + j < N) nz |= (m[p0 + j] != 0 ? 1u : 0u) << j;
  }
  const unsigned prev = (p0 > 0 && p0 - 1 < N && m[p0 - 1] != 0) ? 1u : 0u;
  return (nz ^ ((nz << 1) | prev)) & 0xffffu;
}

// inclusive prefix sum over the workgroup (256 threads, 4 waves); `red` holds 4 ints of LDS.  *total: the sum.
static __device__ __forceinline__ int rle_block_scan(int v, int* red, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  __syncthreads();                               // `red` may still be read from the previous call
  if (lane == 63) red[wv] = v;
  __syncthreads();
  int before = 0;
  for (int i = 0; i < wv; ++i) before += red[i];
  *total = red[0] + red[1] + red[2] + red[3];
  return v + before;
}

// work [B][tiles]: the number of changes in each tile
__global__ __launch_bounds__(PP_THREADS) void rle_count_kernel(const unsigned char* __restrict__ masks, long N,
                                                               unsigned* __restrict__ work, int tiles, int vec) {
  __shared__ int red[4];
  const unsigned char* m = masks + (long)blockIdx.y * N;
  const long p0 = ((long)blockIdx.x * PP_THREADS + threadIdx.x) * RLE_SPAN;
  int total;
  rle_block_scan(__popc(rle_changes(m, N, p0, vec != 0)), red, &total);
  if (threadIdx.x == 0) work[(long)blockIdx.y * tiles + blockIdx.x] = (unsigned)total;
}

// one workgroup per image: work -> its exclusive prefix sum, counts[b] = changes / 2
__global__ __launch_bounds__(PP_THREADS) void rle_scan_kernel(unsigned* __restrict__ work, int tiles, int* __restrict__ counts) {
  __shared__ int red[4];
  unsigned* wk = work + (long)blockIdx.x * tiles;
  unsigned carry = 0;                            // up to N + 1 changes: 2^31 fits
  for (int t0 = 0; t0 < tiles; t0 += PP_THREADS) {
    const int t = t0 + threadIdx.x;
    const int c = t < tiles ? (int)wk[t] : 0;      // one tile: at most 4096
    int total;
    const int inc = rle_block_scan(c, red, &total);
    if (t < tiles) wk[t] = carry + (unsigned)(inc - c);
    carry += (unsigned)total;
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = (int)(carry >> 1);
}

// runs [B][cap][2] flattened: element k = position of the k-th change + 1 (even k: the 1-indexed start; odd k: one
// past the 1-indexed last pixel), for k / 2 < cap
__global__ __launch_bounds__(PP_THREADS) void rle_write_kernel(const unsigned char* __restrict__ masks, long N,
                                                               const unsigned* __restrict__ work, int tiles,
                                                               unsigned* __restrict__ runs, int cap, int vec) {
  __shared__ int red[4];
  const unsigned char* m = masks + (long)blockIdx.y * N;
  const long p0 = ((long)blockIdx.x * PP_THREADS + threadIdx.x) * RLE_SPAN;
  unsigned tr = rle_changes(m, N, p0, vec != 0);
  const int c = __popc(tr);
  int total;
  const int inc = rle_block_scan(c, red, &total);
  if (total == 0) return;
  long k = (long)work[(long)blockIdx.y * tiles + blockIdx.x] + inc - c;
  unsigned* out = runs + (long)blockIdx.y * cap * 2;
  const long lim = 2l * cap;
  while (tr != 0 && k < lim) {
    const int j = __ffs(tr) - 1;
    tr &= tr - 1;
    out[k++] = (unsigned)(p0 + j) + 1u;
  }
}

__global__ __launch_bounds__(PP_THREADS) void rle_length_kernel(unsigned* __restrict__ runs, int cap,
                                                                const int* __restrict__ counts) {
  const int n = pp_clamp(counts[blockIdx.y], 0, cap);
  const int j = blockIdx.x * PP_THREADS + threadIdx.x;
  if (j >= n) return;
  unsigned* r = runs + ((long)blockIdx.y * cap + j) * 2;
  r[1] = r[1] - r[0];
}

// tiles per image: the `work` scratch of dpa_mask_rle is int32 [B][tiles]; 0 for sizes the launcher rejects
DPA_API int dpa_mask_rle_tiles(int H, int W) {
  if (H < 1 || W < 1 || (long)H * W >= (1l << 31)) return 0;
  return (int)(((long)H * W + 1 + RLE_TILE - 1) / RLE_TILE);               // positions 0 .. N inclusive
}

DPA_API int dpa_mask_rle(const unsigned char* masks, int B, int H, int W, int* runs, int cap, int* counts, int* work,
                         long long work_elems, hipStream_t st) {
  if (B < 1 || H < 1 || W < 1 || cap < 1 || B > 65535) return (int)hipErrorInvalidValue;
  if (!masks || !runs || !counts || !work) return (int)hipErrorInvalidValue;
  if ((long)H * W >= (1l << 31) || cap >= (1 << 30)) return (int)hipErrorInvalidValue;
  const long N = (long)H * W;
  const int tiles = dpa_mask_rle_tiles(H, W);
  if (work_elems < (long long)B * tiles) return (int)hipErrorInvalidValue;
  const int vec = ((uintptr_t)masks & 15) == 0 && (N & 15) == 0;             // every image starts 16-byte aligned
  hipLaunchKernelGGL(rle_count_kernel, dim3(tiles, B), dim3(PP_THREADS), 0, st, masks, N, (unsigned*)work, tiles, vec);
  hipLaunchKernelGGL(rle_scan_kernel, dim3(B), dim3(PP_THREADS), 0, st, (unsigned*)work, tiles, counts);
  hipLaunchKernelGGL(rle_write_kernel, dim3(tiles, B), dim3(PP_THREADS), 0, st, masks, N, (const unsigned*)work, tiles,
                     (unsigned*)runs, cap, vec);
  hipLaunchKernelGGL(rle_length_kernel, dim3((cap + PP_THREADS - 1) / PP_THREADS, B), dim3(PP_THREADS), 0, st,
                     (unsigned*)runs, cap, counts);
  return (int)hipGetLastError();
}
