// Fused flat-arena Adam (one launch for every parameter of a model).
//
// Reference: torch.optim.Adam as constructed at RCNet/rcnet_main.py:233-238 and train_zju.py:205-211
// (betas (0.9, 0.999), eps 1e-8, weight_decay 0 -> L2-coupled form, no amsgrad).  The arithmetic follows
// torch's single-tensor Adam: m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
// p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps).  28 algorithmic bytes per parameter.
#include "rd_common.h"
#include "rd_kernels.h"

namespace rd {

// fp16 mode (static loss scale): any non-finite scaled gradient raises flag[0]; flag[1] counts the steps that were skipped because of it.
// One pass over the gradient arena (4 bytes per parameter) on top of Adam's 28.
__global__ __launch_bounds__(256) void grad_finite_kernel(const float* __restrict__ g, int64_t n, int* __restrict__ flag) {
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float gg[4];
    ld4(g + (i << 2), gg);
#pragma unroll
    for (int e = 0; e < 4; e++) bad |= !(fabsf(gg[e]) <= 3.4028234e38f);      // false for inf and NaN
  }
  for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) bad |= !(fabsf(g[i]) <= 3.4028234e38f);
  if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicAdd(flag, 1);      // any non-zero value raises the flag
}
__global__ void adam_skip_count_kernel(int* __restrict__ flag) {   // after the guarded Adam launches of a step: count the skip, clear the flag
  if (flag[0]) { flag[1] += 1; flag[0] = 0; }
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps,
                                                   float wd, float bc1, float bc2_sqrt, float gscale, const int* __restrict__ skip) {
  if (skip && *skip) return;      // a non-finite gradient somewhere in the arena: parameters and moments stay untouched (uniform branch)
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const float step = lr / bc1;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float pp[4], gg[4], mm[4], vv[4];
    ld4(p + (i << 2), pp); ld4(g + (i << 2), gg); ld4(m + (i << 2), mm); ld4(v + (i << 2), vv);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      float gr = gg[e] * gscale + wd * pp[e];
      mm[e] = b1 * mm[e] + (1.f - b1) * gr;
      vv[e] = b2 * vv[e] + (1.f - b2) * gr * gr;
      pp[e] -= step * mm[e] / (sqrtf(vv[e]) / bc2_sqrt + eps);
    }
    st4(p + (i << 2), pp); st4(m + (i << 2), mm); st4(v + (i << 2), vv);
  }
  for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float gr = g[i] * gscale + wd * p[i];
    float mi = b1 * m[i] + (1.f - b1) * gr, vi = b2 * v[i] + (1.f - b2) * gr * gr;
    m[i] = mi; v[i] = vi;
    p[i] -= step * mi / (sqrtf(vi) / bc2_sqrt + eps);
  }
}

// ---- parameter groups (torch.optim.Adam's list of group dictionaries, RCNet/rcnet_main.py:233-238) in one launch --------------------------
// The table arrives by value in the kernel arguments and is only ever indexed with compile-time constants (a runtime index would send it to
// scratch): the group of an element is the number of group ends at or below it, a group's constant is an unrolled select.  Both are scalar
// work when the element index is block-uniform, which it is for the first and last element of a block's 1024-element chunk, and both are
// done only when a block's chunk leaves the group its previous chunk was in.
__device__ __forceinline__ int adam_group_of(const AdamGroupTable& t, int64_t e) {
  int g = 0;
#pragma unroll
  for (int k = 0; k < kAdamMaxGroups - 1; k++) g += e >= t.end[k] ? 1 : 0;      // ends past the last group equal n > e
  return g;
}
__device__ __forceinline__ float adam_sel(const float (&a)[kAdamMaxGroups], int g) {
  float r = a[0];
#pragma unroll
  for (int k = 1; k < kAdamMaxGroups; k++) r = g == k ? a[k] : r;
  return r;
}
__device__ __forceinline__ int64_t adam_end(const AdamGroupTable& t, int g) {
  int64_t r = t.end[0];
#pragma unroll
  for (int k = 1; k < kAdamMaxGroups; k++) r = g == k ? t.end[k] : r;
  return r;
}
struct AdamConsts { float step, b1, b2, eps, wd, decay, bc2_sqrt; };
// where a group's two bias-correction constants come from: the table itself (rd_adam_step_groups: formed on the host, selected like every other
// constant) or the block's LDS (rd_adam_step_groups_scaled: formed on the device, LDS takes a runtime index)
struct AdamBiasTable {
  const AdamGroupTable& t;
  __device__ __forceinline__ float step_size(int g) const { return adam_sel(t.step_size, g); }
  __device__ __forceinline__ float bc2_sqrt(int g) const { return adam_sel(t.bc2_sqrt, g); }
};
struct AdamBiasLds {
  const float* sm;      // [0, 8): step sizes, [8, 16): sqrt(bias correction 2)
  __device__ __forceinline__ float step_size(int g) const { return sm[g]; }
  __device__ __forceinline__ float bc2_sqrt(int g) const { return sm[kAdamMaxGroups + g]; }
};
template <class Bias>
__device__ __forceinline__ AdamConsts adam_consts(const AdamGroupTable& t, const Bias& bias, int g) {
  AdamConsts c;
  c.step = bias.step_size(g); c.b1 = adam_sel(t.b1, g); c.b2 = adam_sel(t.b2, g); c.eps = adam_sel(t.eps, g);
  c.wd = adam_sel(t.wd, g); c.decay = adam_sel(t.decay, g); c.bc2_sqrt = bias.bc2_sqrt(g);
  return c;
}
// adam_kernel's arithmetic with one group's constants; decoupled decay scales p first (decay = 1 and p * 1 = p for a coupled group)
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, const AdamConsts& c, float gscale) {
  float pd = p * c.decay;
  float gr = g * gscale + c.wd * pd;
  m = c.b1 * m + (1.f - c.b1) * gr;
  v = c.b2 * v + (1.f - c.b2) * gr * gr;
  p = pd - c.step * m / (sqrtf(v) / c.bc2_sqrt + c.eps);
}
__device__ __forceinline__ void adam_update4(float* p, const float* g, float* m, float* v, int64_t i4, const AdamConsts& c, float gscale) {
  float pp[4], gg[4], mm[4], vv[4];
  ld4(p + (i4 << 2), pp); ld4(g + (i4 << 2), gg); ld4(m + (i4 << 2), mm); ld4(v + (i4 << 2), vv);
#pragma unroll
  for (int e = 0; e < 4; e++) adam_update(pp[e], gg[e], mm[e], vv[e], c, gscale);
  st4(p + (i4 << 2), pp); st4(m + (i4 << 2), mm); st4(v + (i4 << 2), vv);
}

// the one loop of both group kernels (always inlined; Bias is the only thing the two instantiations differ in)
template <class Bias>
__device__ __forceinline__ void adam_groups_body(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n, const AdamGroupTable& t,
    const Bias& bias, float gscale) {
  const int64_t n4 = n >> 2;
  // one chunk = the 256 consecutive 16-byte vectors a block handles per grid-stride iteration.  A block's chunks ascend: the outer loop looks the
  // group of a chunk up, the inner loop is adam_kernel's loop over the block's chunks that lie wholly inside that group (one scalar compare each)
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t c0 = (int64_t)blockIdx.x * blockDim.x;
  while (c0 < n4) {
    const int64_t last = (c0 + blockDim.x < n4 ? c0 + blockDim.x : n4) - 1;
    const int glo = adam_group_of(t, c0 << 2), ghi = adam_group_of(t, last << 2);
    if (glo != ghi) {      // a group boundary inside the chunk: every vector looks its own group up (interior ends are multiples of 4)
      const int64_t i = c0 + threadIdx.x;
      if (i < n4) {
        const int gi = adam_group_of(t, i << 2);
        if (!((t.inactive_mask >> gi) & 1)) adam_update4(p, g, m, v, i, adam_consts(t, bias, gi), gscale);
      }
      c0 += stride;
      continue;
    }
    // chunks starting at or below `bound` lie wholly inside the group (the last group ends with the arena's last, possibly partial, chunk)
    const int64_t lim4 = adam_end(t, glo) >> 2;
    const int64_t bound = lim4 >= n4 ? n4 - 1 : lim4 - (int64_t)blockDim.x;
    if ((t.inactive_mask >> glo) & 1) {      // nothing of an inactive group is read
      do c0 += stride; while (c0 <= bound);
      continue;
    }
    const AdamConsts c = adam_consts(t, bias, glo);
    do {
      const int64_t i = c0 + threadIdx.x;
      if (i < n4) adam_update4(p, g, m, v, i, c, gscale);
      c0 += stride;
    } while (c0 <= bound);
  }
  // the scalar tail belongs to the last group
  const int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const int gt = adam_group_of(t, n4 << 2);
    if (!((t.inactive_mask >> gt) & 1)) adam_update(p[i], g[i], m[i], v[i], adam_consts(t, bias, gt), gscale);
  }
}

__global__ __launch_bounds__(256) void adam_groups_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n, const AdamGroupTable t,
    float gscale, const int* __restrict__ skip) {
  if (skip && *skip) return;
  adam_groups_body(p, g, m, v, n, t, AdamBiasTable{t}, gscale);
}

// ---- dynamic loss scale (torch.amp.GradScaler's semantics, kept on the device) -------------------------------------------------------------
// The scaled launch reads the live state: it writes nothing while found_inf is raised, unscales with gscale * inv_scale, and forms every
// group's bias corrections from the EFFECTIVE step (host step less the skips the host has not yet taken out of its counters), in double as
// rd_api.cpp does for the static launch.  Per block: thread k < 8 forms group k's pair, LDS (64 bytes) hands it to the others.
__device__ __forceinline__ int adam_seli(const int (&a)[kAdamMaxGroups], int g) {
  int r = a[0];
#pragma unroll
  for (int k = 1; k < kAdamMaxGroups; k++) r = g == k ? a[k] : r;
  return r;
}
// every group's bias-correction pair from the effective step, into the block's LDS (both live-state kernels; ends with the block barrier)
__device__ __forceinline__ void adam_dyn_bias(const AdamGroupTable& t, const AdamDynTable& d, float* sm) {
  if (threadIdx.x < kAdamMaxGroups) {
    const int k = threadIdx.x;
    const int late = d.state->skipped - d.skipped_base;
    const int hs = adam_seli(d.step, k);
    const double eff = (double)(hs - late > 1 ? hs - late : 1);
    const float lr = adam_sel(t.step_size, k);
    const double bc1 = 1.0 - pow((double)adam_sel(t.b1, k), eff), bc2 = 1.0 - pow((double)adam_sel(t.b2, k), eff);
    sm[k] = lr / (float)bc1;
    sm[kAdamMaxGroups + k] = (float)sqrt(bc2);
  }
  __syncthreads();
}
__global__ __launch_bounds__(256) void adam_groups_scaled_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n, const AdamGroupTable t,
    const AdamDynTable d, float gscale) {
  if (d.state->found_inf) return;      // uniform: every thread of every block reads the same word
  __shared__ float sm[2 * kAdamMaxGroups];
  adam_dyn_bias(t, d, sm);
  adam_groups_body(p, g, m, v, n, t, AdamBiasLds{sm}, gscale * d.state->inv_scale);
}
__global__ void loss_scale_init_kernel(LossScaleState* __restrict__ s, float scale, int growth_tracker) {
  s->scale = scale; s->inv_scale = (float)(1.0 / (double)scale);
  s->found_inf = 0; s->skipped = 0; s->growth_tracker = growth_tracker; s->backoffs = 0; s->growths = 0; s->reserved = 0;
}
// torch._amp_update_scale_ on one thread; the one departure: a backoff that would leave the normal range is not taken (see the header)
__global__ void loss_scale_update_kernel(LossScaleState* __restrict__ s, float growth, float backoff, int interval) {
  float scale = s->scale;
  if (s->found_inf) {
    const float lower = scale * backoff;
    if (lower >= 1.17549435e-38f) { scale = lower; s->backoffs += 1; }
    s->growth_tracker = 0;
    s->skipped += 1;
  } else {
    int tracker = s->growth_tracker + 1;
    if (tracker == interval) {
      const float higher = scale * growth;
      if (fabsf(higher) <= 3.4028234e38f) { scale = higher; s->growths += 1; }
      tracker = 0;
    }
    s->growth_tracker = tracker;
  }
  s->scale = scale;
  s->inv_scale = (float)(1.0 / (double)scale);
  s->found_inf = 0;
}

// ---- global-norm gradient clipping (torch.nn.utils.clip_grad_norm_, kept on the device) ----------------------------------------------------
// One read of the arena, one tiny launch, then the Adam launch multiplies by one more scalar.  The norm pass multiplies every element by
// `pre` first (grad_scale, times the live 1 / loss scale when a state is given): torch's order -- unscale, then norm -- and the squares of scaled
// fp16 gradients cannot overflow where the unscaled ones would not.  Each block leaves ONE double in its own row of the caller's partial
// buffer (no floating-point atomics: the same bits on every run); accumulate = 1 adds to the row instead, so several launches on one stream
// -- the runs of slots written since zero_grad() -- build one norm.  The flag, when given, is raised as grad_finite_kernel raises it.
// a maximum that keeps a NaN once it has seen one, as torch's amax does (fmaxf would drop it)
template <class T>
__device__ __forceinline__ T nan_max(T a, T b) { return (b > a || b != b) ? b : a; }
template <bool INF>
__device__ __forceinline__ void norm_acc(float& acc, float x) {
  if (INF) acc = nan_max(acc, fabsf(x)); else acc += x * x;
}
template <bool INF>
__global__ __launch_bounds__(256) void grad_norm_kernel(const float* __restrict__ g, int64_t n, float gscale, const LossScaleState* __restrict__ state,
                                                        double* __restrict__ partial, int rows, int accumulate, int* __restrict__ flag) {
  const float pre = state ? gscale * state->inv_scale : gscale;      // the product the scaled Adam launch forms
  const int64_t n4 = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  float acc = 0.f;
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float gg[4];
    ld4(g + (i << 2), gg);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      bad |= !(fabsf(gg[e]) <= 3.4028234e38f);
      norm_acc<INF>(acc, gg[e] * pre);
    }
  }
  for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float x = g[i];
    bad |= !(fabsf(x) <= 3.4028234e38f);
    norm_acc<INF>(acc, x * pre);
  }
  if (flag && __ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicAdd(flag, 1);
  // wave (xor butterfly: every lane ends with the same value), then the block's four waves in a fixed order, in double
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float other = __shfl_xor(acc, o);
    acc = INF ? nan_max(acc, other) : acc + other;
  }
  __shared__ float sm[4];
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = (double)sm[0];
#pragma unroll
    for (int w = 1; w < 4; w++) r = INF ? nan_max(r, (double)sm[w]) : r + (double)sm[w];
    double* row = partial + blockIdx.x;
    if (accumulate) r = INF ? nan_max(*row, r) : *row + r;
    *row = r;
    if (!accumulate)      // rows no block owns hold 0: the finalize reads every row
      for (int k = blockIdx.x + gridDim.x; k < rows; k += gridDim.x) partial[k] = 0.0;
  }
}
// one block: the rows in a fixed order in double (thread t takes rows t, t + 256, ..., then a binary tree over the 256 threads), the norm
// rounded to fp32, and torch's coefficient formed in fp32: min(1, max_norm / (total_norm + 1e-6)); NaN stays NaN, an infinite norm gives 0
__global__ __launch_bounds__(256) void grad_clip_finalize_kernel(const double* __restrict__ partial, int rows, float max_norm, int inf_norm,
                                                                 GradClipState* __restrict__ s) {
  __shared__ double sm[256];
  double r = 0.0;
  for (int k = threadIdx.x; k < rows; k += 256) r = inf_norm ? nan_max(r, partial[k]) : r + partial[k];
  sm[threadIdx.x] = r;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) sm[threadIdx.x] = inf_norm ? nan_max(sm[threadIdx.x], sm[threadIdx.x + h]) : sm[threadIdx.x] + sm[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float total = (float)(inf_norm ? sm[0] : sqrt(sm[0]));
    float coef = max_norm / (total + 1e-6f);
    coef = coef > 1.f ? 1.f : coef;      // torch.clamp(max = 1): a NaN passes through
    s->total_norm = total; s->coef = coef;
    s->passes += 1;
    s->clipped += coef < 1.f ? 1 : 0;
    s->nonfinite += fabsf(total) <= 3.4028234e38f ? 0 : 1;
  }
}
__global__ void grad_clip_init_kernel(GradClipState* __restrict__ s) {
  s->total_norm = 0.f; s->coef = 1.f; s->passes = 0; s->clipped = 0; s->nonfinite = 0; s->reserved[0] = s->reserved[1] = s->reserved[2] = 0;
}
// the two group kernels with the gradient multiplied by (grad_scale [* inv_scale]) * coef: a coefficient of exactly 1 leaves every bit
__global__ __launch_bounds__(256) void adam_groups_clipped_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n, const AdamGroupTable t,
    float gscale, const int* __restrict__ skip, const GradClipState* __restrict__ clip) {
  const float coef = clip->coef;
  if (skip && *skip) return;
  adam_groups_body(p, g, m, v, n, t, AdamBiasTable{t}, gscale * coef);
}
__global__ __launch_bounds__(256) void adam_groups_scaled_clipped_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n, const AdamGroupTable t,
    const AdamDynTable d, float gscale, const GradClipState* __restrict__ clip) {
  const float coef = clip->coef;      // issued with the state's words, ahead of the dependent prologue
  if (d.state->found_inf) return;
  __shared__ float sm[2 * kAdamMaxGroups];
  adam_dyn_bias(t, d, sm);
  adam_groups_body(p, g, m, v, n, t, AdamBiasLds{sm}, gscale * d.state->inv_scale * coef);
}

void launch_grad_norm(const float* g, int64_t n, float gscale, const LossScaleState* state, int inf_norm, double* partial, int rows, int accumulate,
                      int* flag, hipStream_t st) {
  unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, 1024), rows));
  if (inf_norm) hipLaunchKernelGGL(grad_norm_kernel<true>, dim3(grid), dim3(256), 0, st, g, n, gscale, state, partial, rows, accumulate, flag);
  else hipLaunchKernelGGL(grad_norm_kernel<false>, dim3(grid), dim3(256), 0, st, g, n, gscale, state, partial, rows, accumulate, flag);
}
void launch_grad_clip_finalize(const double* partial, int rows, float max_norm, int inf_norm, GradClipState* s, hipStream_t st) {
  hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(256), 0, st, partial, rows, max_norm, inf_norm, s);
}
void launch_grad_clip_init(GradClipState* s, hipStream_t st) { hipLaunchKernelGGL(grad_clip_init_kernel, dim3(1), dim3(1), 0, st, s); }
void launch_adam_groups_clipped(float* p, const float* g, float* m, float* v, int64_t n, const AdamGroupTable& t, const AdamDynTable* d, float gscale,
                                const int* skip, const GradClipState* clip, hipStream_t st) {
  unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, 1024), 2048));
  if (d) hipLaunchKernelGGL(adam_groups_scaled_clipped_kernel, dim3(grid), dim3(256), 0, st, p, g, m, v, n, t, *d, gscale, clip);
  else hipLaunchKernelGGL(adam_groups_clipped_kernel, dim3(grid), dim3(256), 0, st, p, g, m, v, n, t, gscale, skip, clip);
}

void launch_adam_groups(float* p, const float* g, float* m, float* v, int64_t n, const AdamGroupTable& t, float gscale, hipStream_t st,
                        const int* skip) {
  unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, 1024), 2048));
  hipLaunchKernelGGL(adam_groups_kernel, dim3(grid), dim3(256), 0, st, p, g, m, v, n, t, gscale, skip);
}
void launch_adam_groups_scaled(float* p, const float* g, float* m, float* v, int64_t n, const AdamGroupTable& t, const AdamDynTable& d,
                               float gscale, hipStream_t st) {
  unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, 1024), 2048));
  hipLaunchKernelGGL(adam_groups_scaled_kernel, dim3(grid), dim3(256), 0, st, p, g, m, v, n, t, d, gscale);
}
void launch_loss_scale_init(LossScaleState* s, float scale, int growth_tracker, hipStream_t st) {
  hipLaunchKernelGGL(loss_scale_init_kernel, dim3(1), dim3(1), 0, st, s, scale, growth_tracker);
}
void launch_loss_scale_update(LossScaleState* s, float growth, float backoff, int interval, hipStream_t st) {
  hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(1), 0, st, s, growth, backoff, interval);
}

void launch_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, float wd,
                 float bc1, float bc2_sqrt, float gscale, hipStream_t st, const int* skip) {
  unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, 1024), 2048));
  hipLaunchKernelGGL(adam_kernel, dim3(grid), dim3(256), 0, st, p, g, m, v, n, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, skip);
}
void launch_grad_finite(const float* g, int64_t n, int* flag, hipStream_t st) {
  unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, 1024), 2048));
  hipLaunchKernelGGL(grad_finite_kernel, dim3(grid), dim3(256), 0, st, g, n, flag);
}
void launch_adam_skip_count(int* flag, hipStream_t st) { hipLaunchKernelGGL(adam_skip_count_kernel, dim3(1), dim3(1), 0, st, flag); }

}  // namespace rd
