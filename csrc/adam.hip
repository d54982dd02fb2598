// The optimizer step over ONE flat fp32 buffer: fused multi-tensor Adam (L2 weight decay, torch.optim.Adam
// semantics) and, as options of the same kernel, the gradient scaled by torch.nn.utils.clip_grad_norm_'s
// coefficient on the fly (CLIP) and an exponential moving average of the parameters kept in the same pass (EMA);
// plus the global gradient norm (deterministic, fp64) that the coefficient comes from.
// Reference: utils/train_utils.py:45 (Adam(lr, weight_decay=1e-8)), SURVEY K13.
// Memory-bound: 4 streams in (p, g, m, v) + 3 out (+ 1 in and out with EMA) -> float4 per lane, grid-stride, one
// launch per step.  With both options off nothing else is launched and no aux block is needed.
//
// aux block (fp64, DPA_AUX_LEN doubles, device): {sumsq, norm, coef, 1 - ema decay of this step, reserved...}.
// coef and the decay are read from it on the device, never from a host scalar, so the launches are the same
// every step and can be captured in a HIP graph.
#include "common.h"
#include <math.h>

#define DPA_AUX_LEN 8
#define SUMSQ_BLOCK 256
#define SUMSQ_MAX_BLOCKS 1024        // 256 CUs x 4 blocks; a constant, not a device query: same bits on every box

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Blocks of stage 1 (= slab entries): a function of n only.
DPA_API int dpa_grad_sumsq_blocks(long long n) {
  if (n < 0) return 0;
  return dpa_grid((n + 3) / 4, SUMSQ_BLOCK, SUMSQ_MAX_BLOCKS);
}

static __device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Stage 1: each lane sums (double)x * (double)x of its float4s (the product of two fp32 values is exact in fp64),
// the wave butterfly and the four wave partials are added in a fixed order, one fp64 partial per block.
__global__ __launch_bounds__(SUMSQ_BLOCK) void grad_sumsq_kernel(const float* __restrict__ g, long long n,
                                                                  double* __restrict__ slab) {
  __shared__ double red[SUMSQ_BLOCK / 64];
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 x = reinterpret_cast<const float4*>(g)[i];
    acc += (double)x.x * (double)x.x;
    acc += (double)x.y * (double)x.y;
    acc += (double)x.z * (double)x.z;
    acc += (double)x.w * (double)x.w;
  }
  // scalar tail (n % 4)
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const double x = (double)g[(n4 << 2) + threadIdx.x];
    acc += x * x;
  }
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) slab[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// Stage 2 (one block): the slab summed in index order, then {sumsq, norm, coef}.
// coef = min(1, C / (norm + 1e-6)) in fp64 (clip_grad_norm_); C = +inf gives 1; a non-finite sumsq gives NaN.
__global__ __launch_bounds__(SUMSQ_BLOCK) void grad_sumsq_finish_kernel(const double* __restrict__ slab, int nb,
                                                                         double* __restrict__ aux, double max_norm) {
  __shared__ double part[SUMSQ_MAX_BLOCKS];
  for (int i = threadIdx.x; i < nb; i += blockDim.x) part[i] = slab[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int i = 0; i < nb; ++i) s += part[i];
  const double norm = sqrt(s);
  double coef;
  if (!isfinite(s)) {
    coef = __builtin_nan("");
  } else {
    const double r = max_norm / (norm + 1e-6);
    coef = r < 1.0 ? r : 1.0;
  }
  aux[0] = s;
  aux[1] = norm;
  aux[2] = coef;
}

DPA_API int dpa_grad_sumsq(const float* g, long long n, double* slab, long long slab_len, double* aux,
                           double max_norm, hipStream_t stream) {
  if (!g || !slab || !aux || n < 0 || !aligned16(g)) return (int)hipErrorInvalidValue;
  const int nb = dpa_grad_sumsq_blocks(n);
  if (slab_len < nb) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(nb), dim3(SUMSQ_BLOCK), 0, stream, g, n, slab);
  hipLaunchKernelGGL(grad_sumsq_finish_kernel, dim3(1), dim3(SUMSQ_BLOCK), 0, stream, (const double*)slab, nb, aux,
                     max_norm);
  return (int)hipGetLastError();
}

// One element of the update: gs = coef * g (CLIP); gr = gs + wd * p; m = b1 m + (1 - b1) gr;
// v = b2 v + (1 - b2) gr^2; p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps); e += (1 - d) (p - e) (EMA).
//
// Every instantiation must round alike (coef == 1 and EMA off or on: the same p, m, v, pinned by
// tests/golden/adam_plain_bits.npz), so the roundings cannot be left to -ffp-contract=fast: which product of a sum
// of two products gets fused is the compiler's choice, and the extra product coef * g changes it.  This file is
// compiled with -ffp-contract=fast-honor-pragmas (tools/build_hip.py), contraction is off in here, and every fma
// is spelled out -- in the float4 loop, and in the scalar tail (TAIL), which fuses m the other way round and does
// not fuse v.
template <bool CLIP, bool EMA, bool TAIL>
static __device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float& e, float coef,
                                                 float lr, float b1, float b2, float eps, float wd, float inv_bc1,
                                                 float inv_sqrt_bc2, float omd) {
#pragma clang fp contract(off)
  float gs = g;
  if constexpr (CLIP) gs = coef * g;
  const float gr = fmaf(wd, p, gs);                          // gr = gs + wd * p
  if constexpr (TAIL) {
    m = fmaf(1.f - b1, gr, b1 * m);                          // m = b1 * m + (1 - b1) * gr
    v = b2 * v + (1.f - b2) * gr * gr;                       // v = b2 * v + (1 - b2) * gr * gr, every op rounded
  } else {
    m = fmaf(b1, m, (1.f - b1) * gr);
    v = fmaf(b2, v, (1.f - b2) * gr * gr);
  }
  const float denom = fmaf(sqrtf(v), inv_sqrt_bc2, eps);     // sqrt(v) * inv_sqrt_bc2 + eps
  p -= lr * inv_bc1 * m / denom;
  if constexpr (EMA) e = fmaf(omd, p - e, e);                // e = e + (1 - d) * (p_new - e)
}

// DEV: hyper-parameters read from a device state block (HIP-graph replay: the captured launch cannot
// bake host scalars that change every step); state = {step, lr, 1/bc1, 1/sqrt(bc2)} in fp64, 1 - d_t = aux[3].
template <bool CLIP, bool EMA, bool DEV>
__global__ __launch_bounds__(256) void adam_flat_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
    float* __restrict__ e, long long n, float lr, float b1, float b2, float eps, float wd, float inv_bc1,
    float inv_sqrt_bc2, float omd, const double* __restrict__ state, const double* __restrict__ aux) {
  if constexpr (DEV) {
    lr = (float)state[1];
    inv_bc1 = (float)state[2];
    inv_sqrt_bc2 = (float)state[3];
    if constexpr (EMA) omd = (float)aux[3];
  }
  float coef = 1.f;
  if constexpr (CLIP) coef = (float)aux[2];
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float4 ee = {0.f, 0.f, 0.f, 0.f};
    if constexpr (EMA) ee = reinterpret_cast<float4*>(e)[i];
    float* pa = &pp.x; float* ga = &gg.x; float* ma = &mm.x; float* va = &vv.x; float* ea = &ee.x;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      adam_elem<CLIP, EMA, false>(pa[j], ga[j], ma[j], va[j], ea[j], coef, lr, b1, b2, eps, wd, inv_bc1,
                                  inv_sqrt_bc2, omd);
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    if constexpr (EMA) reinterpret_cast<float4*>(e)[i] = ee;
  }
  // scalar tail (n % 4)
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    long long i = (n4 << 2) + threadIdx.x;
    float pi = p[i], mi = m[i], vi = v[i], ei = 0.f;
    if constexpr (EMA) ei = e[i];
    adam_elem<CLIP, EMA, true>(pi, g[i], mi, vi, ei, coef, lr, b1, b2, eps, wd, inv_bc1, inv_sqrt_bc2, omd);
    p[i] = pi; m[i] = mi; v[i] = vi;
    if constexpr (EMA) e[i] = ei;
  }
}

template <bool DEV>
static int launch_adam(bool clip, bool ema, hipStream_t stream, float* p, const float* g, float* m, float* v,
                       float* e, long long n, float lr, float b1, float b2, float eps, float wd, float inv_bc1,
                       float inv_sqrt_bc2, float omd, const double* state, const double* aux) {
  const int grid = dpa_grid((n + 3) / 4, 256, 4096);
#define DPA_ADAM(C, E)                                                                                          \
  hipLaunchKernelGGL((adam_flat_kernel<C, E, DEV>), dim3(grid), dim3(256), 0, stream, p, g, m, v, e, n, lr, b1, \
                     b2, eps, wd, inv_bc1, inv_sqrt_bc2, omd, state, aux)
  if (clip && ema) DPA_ADAM(true, true);
  else if (clip) DPA_ADAM(true, false);
  else if (ema) DPA_ADAM(false, true);
  else DPA_ADAM(false, false);
#undef DPA_ADAM
  return (int)hipGetLastError();
}

static bool adam_args_ok(const float* p, const float* g, const float* m, const float* v, const float* e,
                         long long n) {
  if (!p || !g || !m || !v || n < 0) return false;
  return aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(e);
}

// Host-state form.  e == nullptr: EMA off, else ema_decay is this step's d_t.  clip != 0: g is scaled by aux[2]
// (written by dpa_grad_sumsq earlier on the stream); aux may be null when clip == 0.
DPA_API int dpa_adam_flat(float* p, const float* g, float* m, float* v, float* e, long long n, float lr, float b1,
                          float b2, float eps, float wd, float bc1, float bc2, double ema_decay, const double* aux,
                          int clip, hipStream_t stream) {
  if (!adam_args_ok(p, g, m, v, e, n) || (clip && !aux)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  return launch_adam<false>(clip != 0, e != nullptr, stream, p, g, m, v, e, n, lr, b1, b2, eps, wd, 1.f / bc1,
                            1.f / sqrtf(bc2), (float)(1.0 - ema_decay), nullptr, aux);
}

// state[0] += 1 and the bias corrections of the new step, in fp64 (same rounding as the host path); with an aux
// block also this step's EMA decay d_t = min(D, (1 + t) / (10 + t)), t the step count after the increment:
// 1 - d_t goes to aux[3].
__global__ void adam_tick_kernel(double* state, double* aux, double b1, double b2, double ema_decay) {
  const double t = state[0] + 1.0;
  state[0] = t;
  state[2] = 1.0 / (1.0 - pow(b1, t));
  state[3] = 1.0 / sqrt(1.0 - pow(b2, t));
  if (aux) {
    const double w = (1.0 + t) / (10.0 + t);
    aux[3] = 1.0 - (ema_decay < w ? ema_decay : w);
  }
}

// Device-state / graph-capturable form: tick + update, every per-step scalar from `state` (lr = state[1], set by
// the host) and `aux`; ema_decay is D.  aux may be null when clip == 0 and e == nullptr.
DPA_API int dpa_adam_flat_dev(float* p, const float* g, float* m, float* v, float* e, long long n, double* state,
                              double* aux, double b1, double b2, float eps, float wd, double ema_decay, int clip,
                              hipStream_t stream) {
  if (!adam_args_ok(p, g, m, v, e, n) || !state || (!aux && (clip || e))) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, stream, state, aux, b1, b2, ema_decay);
  return launch_adam<true>(clip != 0, e != nullptr, stream, p, g, m, v, e, n, 0.f, (float)b1, (float)b2, eps, wd,
                           0.f, 0.f, 0.f, (const double*)state, (const double*)aux);
}

DPA_API int dpa_version() { return 1; }
DPA_API const char* dpa_error_string(int e) { return hipGetErrorString((hipError_t)e); }
