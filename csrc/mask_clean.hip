// Cleaning of a predicted mask on the GPU (distributedpytorch_amd/predict.py --clean): keep the largest 8-connected
// component of the foreground, fill the holes of what is kept, and count a mask against its ground truth.
//
//   dpa_mask_clean   uint8 masks [B][H][W] -> uint8 [B][H][W] of 0 / value and stats int32 [B][3] = (components
//                    before cleaning, foreground pixels removed, pixels filled), as ops/kernels.py: clean_reference
//                    defines them.  Foreground is every non-zero byte.  flags 1: keep the 8-connected component with
//                    the most pixels, on a tie the one whose first pixel in row-major order comes first.  flags 2: a
//                    background pixel of the kept mask that cannot reach the image border through 4-connected
//                    background becomes foreground.
//   dpa_mask_score   counts int64 [B][3] = (truth, pred, inter) of masks != 0 against truth > cut[b]: the counting
//                    half of dpa_prob_score (predict_post.hip) for a mask that exists already.  One slab row per
//                    4096 pixels with plain stores, then an int64 sum per image; no atomics.
//
// Connected-component labelling.  One labeller, templated on the connectivity (8 or 4) and on the set (non-zero bytes
// of the source, or zero bytes of the kept mask), gives every pixel of the set the smallest row-major index of its
// component, which is unique, so two runs are bit-equal:
//   1. mc_tile_kernel     one workgroup per tile of 16 x 64 pixels: a union-find over the tile in LDS (a pixel
//                         starts at the first pixel of its horizontal run, found by a ballot, and is joined to the
//                         row above once per pair of touching runs), then every pixel stores the image index of its
//                         tile-local root, and the root the pixel count of the tile's piece.
//   2. mc_merge_kernel    pixels on the top row and the left and right column of a tile join their component with
//                         that of set neighbours in another tile (west, north-west, north, north-east; west and
//                         north for connectivity 4; a join that others imply is left out): lock-free union-find on
//                         the label plane.
//   3. mc_flatten_kernel  label = root.
//   4. mc_area_kernel     a tile-local root that is not the root of its component adds its count to the root's:
//                         one integer atomic per (tile, piece), never one per pixel.
//   5. mc_roots_kernel    per image the maximum of (area << 32) | (0xffffffff - root) over the roots, which is the
//                         largest area and among equals the smallest root; the number of roots; the pixel total.
//   6. mc_keep_kernel     dst = value where the pixel's label is the winner (or, without flag 1, where it is set).
//   7. the labeller again on the zero bytes of dst with connectivity 4; mc_border_kernel marks the root of every
//      zero pixel on the image border (plain stores of 1); mc_fill_kernel sets the zero pixels whose root is not
//      marked and counts them.
// Every phase is a launch of its own.  Inside a launch no workgroup waits for another: there is no flag, no grid
// barrier and no spinning; every loop runs at most as many times as the tile or the image has pixels.
//
// Why the merge is correct although a load of a label word may return an OLD value of that word (a CU's L1 is not
// refreshed by another CU's atomics; the loads here bypass it, but nothing below relies on that):
//   * Every value a label word lab[a] ever holds is <= a, is a itself only while a is a root, and is a pixel that
//     already belongs to a's component.  Labels only decrease (atomicMin, or the flatten's store of the root).
//     So a walk along any mixture of old and current labels stays inside the component and strictly descends: it
//     ends after at most n steps at a pixel that is or was a root of that component.
//   * The only decision that needs the CURRENT state is "a is a root and I linked it to b".  It rests on the value
//     atomicMin(&lab[a], b) returns, which an agent-scope atomic reads in L2: returned a means a was a root and
//     now points at b < a.  Any other returned value `old` < a means a had a parent already; lab[a] is then
//     min(old, b), both members of what must become one component, and the loop goes on to unite old with b, so no
//     link is lost.  A walk that stopped at a stale root costs one more round, never a wrong link.
//   * Flattening runs after the merge launch has ended, when no label changes but to its component's root.
// Only integer atomics are used.  Every label, and the winner, is range-checked before it becomes an address.
#include "common.h"

#define MC_THREADS 256
#define MC_TW 64                                // tile width: one wave reads 64 consecutive bytes of a row
#define MC_TH 16                                // tile height
#define MC_TP (MC_TW * MC_TH)                   // pixels per tile
#define MC_PER (MC_TP / MC_THREADS)             // pixels per thread in the tile kernel
#define MC_SPAN 16                              // pixels per thread in the flat kernels
#define MC_CHUNK (MC_THREADS * MC_SPAN)         // pixels per workgroup in the flat kernels
#define MC_HDR 8                                // header words per image: key (2), roots, total, filled, 3 spare

static_assert(MC_TW == 64 && (MC_TP & (MC_TP - 1)) == 0, "the tile kernel shifts and masks by these");

// ------------------------------------------------------------------------------ union-find in LDS (one tile)
static __device__ __forceinline__ int mc_lds_load(const int* l, int a) {
  return __hip_atomic_load(l + (a & (MC_TP - 1)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

static __device__ __forceinline__ int mc_lds_find(const int* l, int a) {
  for (int i = 0; i < MC_TP; ++i) {             // strictly descending: at most MC_TP steps
    const int r = mc_lds_load(l, a);
    if (r == a || r < 0) break;
    a = r;
  }
  return a;
}

static __device__ __forceinline__ void mc_lds_union(int* l, int a, int b) {
  for (int i = 0; i < MC_TP; ++i) {             // every round but the last lowers a or b
    a = mc_lds_find(l, a);
    b = mc_lds_find(l, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(l + (a & (MC_TP - 1)), b);
    if (old == a) return;
    a = old;
  }
}

// ------------------------------------------------------------------------------ union-find on the label plane
static __device__ __forceinline__ int mc_load(const int* lab, int a) {
  return __hip_atomic_load(lab + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a: a pixel of the set, 0 <= a < n.  Returns a pixel that is or was a root of a's component.
static __device__ __forceinline__ int mc_find(const int* lab, int n, int a) {
  for (int i = 0; i < n; ++i) {                 // strictly descending: at most n steps
    const int r = mc_load(lab, a);
    if (r >= a || r < 0) break;                 // a root; anything else outside [0, a) is not a label and ends the walk
    a = r;
  }
  return a;
}

static __device__ __forceinline__ void mc_union(int* lab, int n, int a, int b) {
  for (int i = 0; i < n; ++i) {                 // every round but the last lowers a or b
    a = mc_find(lab, n, a);
    b = mc_find(lab, n, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(lab + a, b);      // agent scope: the returned value is current
    if (old == a) return;                       // a was a root and is linked now
    if (old < 0 || old > a) return;             // not a label: never on a plane the tile kernel wrote
    a = old;                                    // a had a parent: unite that parent with b
  }
}

template <bool INV>
static __device__ __forceinline__ bool mc_set(unsigned char v) { return INV ? v == 0 : v != 0; }

// ------------------------------------------------------------------------------ 1. tiles
// m: the bytes that define the set, [B][n].  lab [n] and aux [n] of image blockIdx.z lie at work + z * per + MC_HDR.
// Every word of both planes is written.  AREA: aux = pixels of the tile's piece at its root, 0 elsewhere; else 0.
template <int CONN, bool INV, bool AREA>
__global__ __launch_bounds__(MC_THREADS) void mc_tile_kernel(const unsigned char* __restrict__ m, int H, int W,
                                                             int* __restrict__ work, long per) {
  __shared__ int l[MC_TP];
  __shared__ int cnt[MC_TP];
  const long n = (long)H * W;
  const unsigned char* img = m + (long)blockIdx.z * n;
  int* lab = work + (long)blockIdx.z * per + MC_HDR;
  int* aux = lab + n;
  const int x0 = blockIdx.x * MC_TW, y0 = blockIdx.y * MC_TH;
  const int lane = threadIdx.x & 63;             // = the pixel's column in the tile
  unsigned inside = 0, set = 0;
#pragma unroll
  for (int j = 0; j < MC_PER; ++j) {
    const int li = threadIdx.x + j * MC_THREADS;
    const int y = y0 + (li >> 6), x = x0 + (li & 63);
    const bool in = y < H && x < W;
    const bool s = in && mc_set<INV>(img[in ? (long)y * W + x : 0]);
    inside |= (in ? 1u : 0u) << j;
    set |= (s ? 1u : 0u) << j;
    // a wave holds one row of the tile: a pixel starts out pointing at the first pixel of its horizontal run,
    // the lane above the highest unset lane below it
    const unsigned long long unset_below = ~__ballot(s) & ((1ull << lane) - 1ull);
    const int start = unset_below ? 64 - __clzll((long long)unset_below) : 0;
    l[li] = s ? li - lane + start : -1;
    cnt[li] = 0;
  }
  __syncthreads();
  // Join with the set pixels of the row above (the run joined the western one).  With W, NW, N, NE the western
  // and the three upper neighbours: N is joined unless W and NW are both set, since then W is joined with NW,
  // its upper neighbour, and NW with N, its eastern one.  Connectivity 8, N unset: NW is joined unless W is set
  // (NW is W's upper neighbour), and NE.  With N set, NW and NE are N's neighbours in its row.
#pragma unroll
  for (int j = 0; j < MC_PER; ++j) {
    if (!((set >> j) & 1u)) continue;
    const int li = threadIdx.x + j * MC_THREADS;
    const int ly = li >> 6, lx = li & 63;
    if (ly == 0) continue;
    const bool north = l[li - MC_TW] >= 0;
    const bool west = lx > 0 && l[li - 1] >= 0;
    const bool nw = lx > 0 && l[li - MC_TW - 1] >= 0;
    if (north) {
      if (!(west && nw)) mc_lds_union(l, li, li - MC_TW);
    } else if (CONN == 8) {
      if (!west && nw) mc_lds_union(l, li, li - MC_TW - 1);
      if (lx < MC_TW - 1 && l[li - MC_TW + 1] >= 0) mc_lds_union(l, li, li - MC_TW + 1);
    }
  }
  __syncthreads();
  int root[MC_PER];
#pragma unroll
  for (int j = 0; j < MC_PER; ++j) {
    const int li = threadIdx.x + j * MC_THREADS;
    root[j] = ((set >> j) & 1u) ? mc_lds_find(l, li) & (MC_TP - 1) : -1;
    if (AREA && root[j] >= 0) atomicAdd(&cnt[root[j]], 1);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < MC_PER; ++j) {
    if (!((inside >> j) & 1u)) continue;
    const int li = threadIdx.x + j * MC_THREADS;
    const long p = (long)(y0 + (li >> 6)) * W + x0 + (li & 63);
    // the root lies in this tile and is a pixel of the image: its index is below n
    lab[p] = root[j] < 0 ? -1 : (int)((long)(y0 + (root[j] >> 6)) * W + x0 + (root[j] & 63));
    aux[p] = AREA && root[j] == li ? cnt[li] : 0;
  }
}

// ------------------------------------------------------------------------------ 2. merge across tile borders
template <int CONN, bool INV>
__global__ __launch_bounds__(MC_THREADS) void mc_merge_kernel(const unsigned char* __restrict__ m, int H, int W,
                                                              int* __restrict__ work, long per) {
  const long n = (long)H * W;
  const unsigned char* img = m + (long)blockIdx.z * n;
  int* lab = work + (long)blockIdx.z * per + MC_HDR;
  // one thread per border pixel of the tile: 64 on the top row, 15 below it on the left and on the right column
  const int t = threadIdx.x;
  int ly, lx;
  if (t < MC_TW) ly = 0, lx = t;
  else if (t < MC_TW + MC_TH - 1) ly = t - MC_TW + 1, lx = 0;
  else if (t < MC_TW + 2 * (MC_TH - 1)) ly = t - (MC_TW + MC_TH - 1) + 1, lx = MC_TW - 1;
  else return;
  const int y = blockIdx.y * MC_TH + ly, x = blockIdx.x * MC_TW + lx;
  if (y >= H || x >= W) return;
  const long p = (long)y * W + x;
  if (!mc_set<INV>(img[p])) return;
  // The neighbours behind the pixel that lie in another tile, by the tile kernel's rules on the whole image: N
  // unless W and NW are set; NW and NE only with N unset, NW only with W unset too.  W is joined across the tile's
  // left edge unless N, in this tile, and NW are set: then the pixel is joined with N, N with NW across the edge,
  // and NW with W below it.  That exception needs a row above in the tile, so a tile's corner pixel never relies
  // on W for N and on N for W at once.
  const bool top = ly == 0, left = lx == 0, right = lx == MC_TW - 1;
  const bool west = x > 0 && mc_set<INV>(img[p - 1]);
  const bool north = y > 0 && mc_set<INV>(img[p - W]);
  const bool nw = y > 0 && x > 0 && mc_set<INV>(img[p - W - 1]);
  if (left && west && !(!top && north && nw)) mc_union(lab, (int)n, (int)p, (int)(p - 1));
  if (top && north && !(west && nw)) mc_union(lab, (int)n, (int)p, (int)(p - W));
  if (CONN == 8 && !north) {
    if (!west && nw && (top || left)) mc_union(lab, (int)n, (int)p, (int)(p - W - 1));
    if (y > 0 && x + 1 < W && (top || right) && mc_set<INV>(img[p - W + 1]))
      mc_union(lab, (int)n, (int)p, (int)(p - W + 1));
  }
}

// ------------------------------------------------------------------------------ 3. flatten, 4. areas
__global__ __launch_bounds__(MC_THREADS) void mc_flatten_kernel(int* __restrict__ work, long per, int n) {
  int* lab = work + (long)blockIdx.y * per + MC_HDR;
  const long p0 = (long)blockIdx.x * MC_CHUNK + threadIdx.x;
#pragma unroll 4
  for (int j = 0; j < MC_SPAN; ++j) {
    const long p = p0 + (long)j * MC_THREADS;
    if (p >= n) break;
    const int r = lab[p];
    if (r >= 0 && r < (int)p) lab[p] = mc_find(lab, n, r);
  }
}

__global__ __launch_bounds__(MC_THREADS) void mc_area_kernel(int* __restrict__ work, long per, int n) {
  const int* lab = work + (long)blockIdx.y * per + MC_HDR;
  int* aux = work + (long)blockIdx.y * per + MC_HDR + n;
  const long p0 = (long)blockIdx.x * MC_CHUNK + threadIdx.x;
#pragma unroll 4
  for (int j = 0; j < MC_SPAN; ++j) {
    const long p = p0 + (long)j * MC_THREADS;
    if (p >= n) break;
    const int a = aux[p];                        // only a component's root is added to, and a root adds nothing
    if (a <= 0) continue;
    const int r = lab[p];
    if (r >= 0 && r < (int)p) atomicAdd(aux + r, a);
  }
}

// ------------------------------------------------------------------------------ header and reductions
__global__ void mc_init_kernel(int* __restrict__ work, long per) {
  if (threadIdx.x < MC_HDR) work[(long)blockIdx.x * per + threadIdx.x] = 0;
}

template <class T>
static __device__ __forceinline__ T mc_wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;                                      // lane 0 holds the sum
}

// 5. roots: a pixel is the root of a component where its label is its own index; aux holds the component's area
__global__ __launch_bounds__(MC_THREADS) void mc_roots_kernel(int* __restrict__ work, long per, int n) {
  int* hdr = work + (long)blockIdx.y * per;
  const int* lab = hdr + MC_HDR;
  const int* aux = lab + n;
  const long p0 = (long)blockIdx.x * MC_CHUNK + threadIdx.x;
  unsigned long long key = 0;
  unsigned roots = 0, total = 0;
#pragma unroll 4
  for (int j = 0; j < MC_SPAN; ++j) {
    const long p = p0 + (long)j * MC_THREADS;
    if (p >= n) break;
    if (lab[p] != (int)p) continue;
    const unsigned a = (unsigned)aux[p];
    const unsigned long long k = ((unsigned long long)a << 32) | (0xffffffffu - (unsigned)p);
    key = k > key ? k : key;
    ++roots;
    total += a;                                  // the areas of an image add up to at most n < 2^31
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long k = __shfl_down(key, o, 64);
    key = k > key ? k : key;
  }
  roots = mc_wave_sum(roots);
  total = mc_wave_sum(total);
  if ((threadIdx.x & 63) == 0 && roots != 0) {
    atomicMax(reinterpret_cast<unsigned long long*>(hdr), key);
    atomicAdd(reinterpret_cast<unsigned*>(hdr) + 2, roots);
    atomicAdd(reinterpret_cast<unsigned*>(hdr) + 3, total);
  }
}

// 6. ALL: dst = value where src is set; else where the pixel's label is the winner of its image
template <bool ALL>
__global__ __launch_bounds__(MC_THREADS) void mc_keep_kernel(const unsigned char* __restrict__ src,
                                                             unsigned char* __restrict__ dst,
                                                             const int* __restrict__ work, long per, int n,
                                                             unsigned value) {
  const int* hdr = work + (long)blockIdx.y * per;
  const int* lab = hdr + MC_HDR;
  const unsigned char* s = src + (long)blockIdx.y * n;
  unsigned char* d = dst + (long)blockIdx.y * n;
  int win = -1;                                  // an empty image has no root: the key stays 0
  if (!ALL) {
    const unsigned long long key = *reinterpret_cast<const unsigned long long*>(hdr);
    if (key >> 32) win = (int)(0xffffffffu - (unsigned)key);
  }
  const long p0 = (long)blockIdx.x * MC_CHUNK + threadIdx.x;
#pragma unroll 4
  for (int j = 0; j < MC_SPAN; ++j) {
    const long p = p0 + (long)j * MC_THREADS;
    if (p >= n) break;
    const bool keep = s[p] != 0 && (ALL || lab[p] == win);
    d[p] = (unsigned char)(keep ? value : 0u);
  }
}

// 7. fill: flag (the aux plane, zeroed by the tile kernel) = 1 at the root of every zero pixel on the image border
__global__ __launch_bounds__(MC_THREADS) void mc_border_kernel(const unsigned char* __restrict__ dst,
                                                               int* __restrict__ work, long per, int H, int W) {
  const long n = (long)H * W;
  const int* lab = work + (long)blockIdx.y * per + MC_HDR;
  int* flag = work + (long)blockIdx.y * per + MC_HDR + n;
  const unsigned char* d = dst + (long)blockIdx.y * n;
  const long k = (long)blockIdx.x * MC_THREADS + threadIdx.x;       // 0 .. 2W - 1: top and bottom row; then the columns
  long p;
  if (k < W) p = k;
  else if (k < 2l * W) p = (long)(H - 1) * W + (k - W);
  else if (k < 2l * W + H) p = (k - 2l * W) * W;
  else if (k < 2l * W + 2l * H) p = (k - 2l * W - H) * W + (W - 1);
  else return;
  if (d[p] != 0) return;
  const int r = lab[p];
  if (r >= 0 && r < n) flag[r] = 1;
}

__global__ __launch_bounds__(MC_THREADS) void mc_fill_kernel(unsigned char* __restrict__ dst, int* __restrict__ work,
                                                             long per, int n, unsigned value) {
  int* hdr = work + (long)blockIdx.y * per;
  const int* lab = hdr + MC_HDR;
  const int* flag = lab + n;
  unsigned char* d = dst + (long)blockIdx.y * n;
  const long p0 = (long)blockIdx.x * MC_CHUNK + threadIdx.x;
  unsigned filled = 0;
#pragma unroll 4
  for (int j = 0; j < MC_SPAN; ++j) {
    const long p = p0 + (long)j * MC_THREADS;
    if (p >= n) break;
    if (d[p] != 0) continue;
    const int r = lab[p];
    if (r >= 0 && r < n && flag[r] == 0) {
      d[p] = (unsigned char)value;
      ++filled;
    }
  }
  filled = mc_wave_sum(filled);
  if ((threadIdx.x & 63) == 0 && filled != 0) atomicAdd(reinterpret_cast<unsigned*>(hdr) + 4, filled);
}

__global__ void mc_stats_kernel(const int* __restrict__ work, long per, int B, int* __restrict__ stats) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int* hdr = work + (long)b * per;
  const unsigned long long key = *reinterpret_cast<const unsigned long long*>(hdr);
  stats[3 * b + 0] = hdr[2];
  stats[3 * b + 1] = hdr[3] - (int)(key >> 32);
  stats[3 * b + 2] = hdr[4];
}

// int32 words of workspace per image: the header, the label plane and the area / flag plane.  0 for sizes the
// launcher refuses: no pixels, a word count that does not fit in int32, more tile rows than grid.y takes.
DPA_API int dpa_mask_clean_work(int H, int W) {
  if (H < 1 || W < 1) return 0;
  const long n = (long)H * W, per = 2 * n + MC_HDR;
  if (per >= (1l << 31)) return 0;
  if (((long)H + MC_TH - 1) / MC_TH > 65535) return 0;
  return (int)per;
}

template <int CONN, bool INV, bool AREA>
static void mc_label(const unsigned char* m, int B, int H, int W, int* work, long per, hipStream_t st) {
  const int n = H * W;
  const dim3 tiles((W + MC_TW - 1) / MC_TW, (H + MC_TH - 1) / MC_TH, B);
  const dim3 flat((n + MC_CHUNK - 1) / MC_CHUNK, B);
  hipLaunchKernelGGL((mc_tile_kernel<CONN, INV, AREA>), tiles, dim3(MC_THREADS), 0, st, m, H, W, work, per);
  hipLaunchKernelGGL((mc_merge_kernel<CONN, INV>), tiles, dim3(128), 0, st, m, H, W, work, per);   // 94 border pixels
  hipLaunchKernelGGL(mc_flatten_kernel, flat, dim3(MC_THREADS), 0, st, work, per, n);
}

// flags: 1 keep the largest component, 2 fill holes (after 1).  value: 1 .. 255, the byte of a foreground pixel of
// dst.  work: int32 [B][dpa_mask_clean_work(H, W)], 8-byte aligned, any contents.
DPA_API int dpa_mask_clean(const unsigned char* src, int B, int H, int W, unsigned char* dst, int flags, int value,
                           int* stats, int* work, long long work_elems, hipStream_t st) {
  if (B < 1 || H < 1 || W < 1 || B > 65535 || flags < 1 || flags > 3 || value < 1 || value > 255)
    return (int)hipErrorInvalidValue;
  if (!src || !dst || !stats || !work || src == dst || ((uintptr_t)work & 7)) return (int)hipErrorInvalidValue;
  const long per = dpa_mask_clean_work(H, W);
  if (per < 1 || work_elems < (long long)B * per) return (int)hipErrorInvalidValue;
  const int n = H * W;
  const dim3 flat((n + MC_CHUNK - 1) / MC_CHUNK, B), thr(MC_THREADS);
  hipLaunchKernelGGL(mc_init_kernel, dim3(B), dim3(64), 0, st, work, per);
  if (flags & 1) {
    mc_label<8, false, true>(src, B, H, W, work, per, st);
    hipLaunchKernelGGL(mc_area_kernel, flat, thr, 0, st, work, per, n);
    hipLaunchKernelGGL(mc_roots_kernel, flat, thr, 0, st, work, per, n);
    hipLaunchKernelGGL(mc_keep_kernel<false>, flat, thr, 0, st, src, dst, (const int*)work, per, n, (unsigned)value);
  } else {
    hipLaunchKernelGGL(mc_keep_kernel<true>, flat, thr, 0, st, src, dst, (const int*)work, per, n, (unsigned)value);
  }
  if (flags & 2) {
    mc_label<4, true, false>(dst, B, H, W, work, per, st);
    const long rim = 2l * W + 2l * H;
    hipLaunchKernelGGL(mc_border_kernel, dim3((unsigned)((rim + MC_THREADS - 1) / MC_THREADS), B), thr, 0, st,
                       (const unsigned char*)dst, work, per, H, W);
    hipLaunchKernelGGL(mc_fill_kernel, flat, thr, 0, st, dst, work, per, n, (unsigned)value);
  }
  hipLaunchKernelGGL(mc_stats_kernel, dim3((B + 63) / 64), dim3(64), 0, st, (const int*)work, per, B, stats);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------ counting a mask against its truth
// A workgroup counts MC_CHUNK = 4096 consecutive pixels, a thread 16 of them (one 16-byte load each where the image
// starts are aligned), into row blockIdx.x of work [B][blocks][3] = (truth, pred, inter); mc_score_sum_kernel adds
// an image's rows up in int64.
__global__ __launch_bounds__(MC_THREADS) void mc_score_kernel(const unsigned char* __restrict__ masks,
                                                              const unsigned char* __restrict__ truth,
                                                              const int* __restrict__ cut, long n, int blocks,
                                                              unsigned* __restrict__ work, int vec) {
  __shared__ unsigned red[4][3];
  const unsigned char* m = masks + (long)blockIdx.y * n;
  const unsigned char* t = truth + (long)blockIdx.y * n;
  const int cutv = cut[blockIdx.y];
  const long p0 = ((long)blockIdx.x * MC_THREADS + threadIdx.x) * MC_SPAN;
  unsigned nt = 0, np = 0, ni = 0;
  if (vec && p0 + MC_SPAN <= n) {
    const u32x4_t mv = *reinterpret_cast<const u32x4_t*>(m + p0);
    const u32x4_t tv = *reinterpret_cast<const u32x4_t*>(t + p0);
#pragma unroll
    for (int j = 0; j < MC_SPAN; ++j) {
      const unsigned pm = ((mv[j >> 2] >> ((j & 3) * 8)) & 255u) != 0u ? 1u : 0u;
      const unsigned pt = (int)((tv[j >> 2] >> ((j & 3) * 8)) & 255u) > cutv ? 1u : 0u;
      nt += pt, np += pm, ni += pm & pt;
    }
  } else {
    for (int j = 0; j < MC_SPAN; ++j)
      if (p0 + j < n) {
        const unsigned pm = m[p0 + j] != 0 ? 1u : 0u;
        const unsigned pt = (int)t[p0 + j] > cutv ? 1u : 0u;
        nt += pt, np += pm, ni += pm & pt;
      }
  }
  nt = mc_wave_sum(nt), np = mc_wave_sum(np), ni = mc_wave_sum(ni);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) red[wv][0] = nt, red[wv][1] = np, red[wv][2] = ni;
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    work[((long)blockIdx.y * blocks + blockIdx.x) * 3 + k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
  }
}

// one workgroup per image
__global__ __launch_bounds__(MC_THREADS) void mc_score_sum_kernel(const unsigned* __restrict__ work, int blocks,
                                                                  long long* __restrict__ counts) {
  __shared__ long long red[4][3];
  const unsigned* wk = work + (long)blockIdx.x * blocks * 3;
  long long acc[3] = {0, 0, 0};
  for (int r = threadIdx.x; r < blocks; r += MC_THREADS)
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] += (long long)wk[(long)r * 3 + k];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const long long v = mc_wave_sum(acc[k]);
    if (lane == 0) red[wv][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    counts[(long)blockIdx.x * 3 + k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
  }
}

// workgroups (= rows of `work`) per image of dpa_mask_score; 0 for sizes the launcher rejects
DPA_API int dpa_mask_score_blocks(int H, int W) {
  if (H < 1 || W < 1 || (long)H * W >= (1l << 31)) return 0;
  return (int)(((long)H * W + MC_CHUNK - 1) / MC_CHUNK);
}

DPA_API int dpa_mask_score(const unsigned char* masks, const unsigned char* truth, const int* cut, int B, int H, int W,
                           long long* counts, unsigned* work, long long work_elems, hipStream_t st) {
  if (B < 1 || H < 1 || W < 1 || B > 65535) return (int)hipErrorInvalidValue;
  if (!masks || !truth || !cut || !counts || !work) return (int)hipErrorInvalidValue;
  const int blocks = dpa_mask_score_blocks(H, W);
  if (blocks < 1 || work_elems < (long long)B * blocks * 3) return (int)hipErrorInvalidValue;
  const long n = (long)H * W;
  const int vec = (((uintptr_t)masks | (uintptr_t)truth) & 15) == 0 && (n & 15) == 0;
  hipLaunchKernelGGL(mc_score_kernel, dim3(blocks, B), dim3(MC_THREADS), 0, st, masks, truth, cut, n, blocks, work, vec);
  hipLaunchKernelGGL(mc_score_sum_kernel, dim3(B), dim3(MC_THREADS), 0, st, (const unsigned*)work, blocks, counts);
  return (int)hipGetLastError();
}
