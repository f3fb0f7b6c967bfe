// Masked order statistics on the device and the unsupervised term of the Scale-Map-Learner loss that needs them.
//
// Reference:
//   utils/loss.py:65-70, 83-88, 101-106   loss_unsupervised = phi(output[M] / median(output[M]) - image[M] / median(image[M])), M = invalid_map_gt
//   train_zju.py:361, :464                 invalid_map_gt = batch_gt <= 0 (before outlier removal), "for areas without lidar GT depth"
//
// torch.median over a boolean selection is a sort, a host synchronisation and a variable-size buffer.  Here the lower median (0-based rank
// (n-1)/2 of the n selected values) comes from an exact radix selection on an order-preserving uint32 key: four passes of 8 bits, each one
// streaming the maps once and counting the digit of every selected element whose higher digits match the prefix found so far (per-block LDS
// histogram, one global integer add per non-empty bin per block), and a one-wave kernel between the passes that finds the bin holding the rank
// and leaves the new prefix and the residual rank in DEVICE memory.  The host never learns n, the rank or the prefix, the grids depend on the
// tensor size alone, nothing synchronises: the sequence can be captured in a hipGraph.  The counts are integers, so the result does not
// depend on the order in which blocks arrive: bit-exact and reproducible.  Two selections (prediction and input depth, same mask) ride in the
// same passes.
#include "rd_common.h"
#include "rd_kernels.h"

namespace rd {

// scratch, in 32-bit words: hist[pass 0..3][selection 0..1][256] then the state below
static constexpr int SEL_BINS = 256, SEL_PASSES = 4;
static constexpr int SEL_STATE = SEL_PASSES * 2 * SEL_BINS;
enum { ST_N = 0, ST_NAN0, ST_NAN1, ST_PREFIX0, ST_PREFIX1, ST_K0, ST_K1, ST_PAD, SEL_STATE_WORDS };
static constexpr int SEL_WORDS = SEL_STATE + SEL_STATE_WORDS;
// the unsupervised term appends: float med[4] = [m_o, m_I, n, nan flag], then double partial[rows][3]
static constexpr int64_t UNSUP_MED_OFF = (int64_t)SEL_WORDS * 4, UNSUP_PART_OFF = UNSUP_MED_OFF + 16;

// count passes: every block ends with a flush of up to 512 global adds, and the first two passes are bound by LDS adds on a few bins, not by
// the loads (measured: 1024 blocks make the last pass faster, the first ones slower, the sum no better), so 256 blocks; the term's forward ends with three doubles per block for a one-wave
// finalize (512 rows), its backward with nothing: they only need loads in flight
static unsigned sel_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, 1024), 256)); }
static unsigned unsup_rows(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, 1024), 512)); }
static unsigned unsup_bwd_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, 1024), 2048)); }

// order-preserving key: all bits flipped when negative, the sign bit otherwise (-0 sorts right below +0)
__device__ __forceinline__ unsigned sel_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sel_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// f(i, x0[i], x1[i]) for every selected element: mask_u8[i] != 0 (the memory of a torch bool tensor) or mask_le0[i] <= 0 (exactly one of the two is
// given).  16-byte loads when the pointers allow them; the last n % 4 elements and unaligned inputs take the scalar loop.
template <typename F>
__device__ __forceinline__ void masked_scan(const float* __restrict__ x0, const float* __restrict__ x1, const unsigned char* __restrict__ mu8,
                                            const float* __restrict__ mf, int64_t n, F&& f) {
  const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gstride = (int64_t)gridDim.x * blockDim.x;
  const bool vec = ((reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(x1) | reinterpret_cast<uintptr_t>(mf)) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(mu8) & 3) == 0;
  int64_t done = 0;
  if (vec) {
    const int64_t n4 = n >> 2;
    const float4* a4 = reinterpret_cast<const float4*>(x0);
    const float4* b4 = reinterpret_cast<const float4*>(x1);
    for (int64_t j = gtid; j < n4; j += gstride) {
      const float4 a = a4[j], b = b4[j];
      bool m0, m1, m2, m3;
      if (mu8) {
        const unsigned w = reinterpret_cast<const unsigned*>(mu8)[j];
        m0 = (w & 0xffu) != 0; m1 = (w & 0xff00u) != 0; m2 = (w & 0xff0000u) != 0; m3 = (w & 0xff000000u) != 0;
      } else {
        const float4 g = reinterpret_cast<const float4*>(mf)[j];
        m0 = g.x <= 0.f; m1 = g.y <= 0.f; m2 = g.z <= 0.f; m3 = g.w <= 0.f;
      }
      if (m0) f(4 * j, a.x, b.x);
      if (m1) f(4 * j + 1, a.y, b.y);
      if (m2) f(4 * j + 2, a.z, b.z);
      if (m3) f(4 * j + 3, a.w, b.w);
    }
    done = n4 << 2;
  }
  for (int64_t i = done + gtid; i < n; i += gstride)
    if (mu8 ? mu8[i] != 0 : mf[i] <= 0.f) f(i, x0[i], x1[i]);
}

__global__ __launch_bounds__(256) void select_zero_kernel(unsigned* __restrict__ scratch) {
  for (int i = threadIdx.x; i < SEL_WORDS; i += blockDim.x) scratch[i] = 0u;
}

// one digit pass: histogram of bits [shift, shift + 8) of the keys whose bits above match the prefix
__global__ __launch_bounds__(256) void select_count_kernel(const float* __restrict__ x0, const float* __restrict__ x1,
                                                           const unsigned char* __restrict__ mu8, const float* __restrict__ mf, int64_t n,
                                                           unsigned* __restrict__ scratch, int pass) {
  __shared__ unsigned h[2 * SEL_BINS];
  __shared__ unsigned snan[2];
  const int t = threadIdx.x;
  h[t] = 0u; h[t + SEL_BINS] = 0u;
  if (t < 2) snan[t] = 0u;
  __syncthreads();
  unsigned* state = scratch + SEL_STATE;
  const int shift = 24 - 8 * pass;
  const unsigned hm = pass ? 0xffffffffu << (shift + 8) : 0u;
  const unsigned p0 = pass ? state[ST_PREFIX0] : 0u, p1 = pass ? state[ST_PREFIX1] : 0u;
  // a thread keeps the run of equal digits it is in and adds it once: on near-constant maps (every exponent the same) the LDS adds of a
  // thread collapse into one instead of serialising on a single bin
  unsigned d0 = 0u, c0 = 0u, d1 = 0u, c1 = 0u, nan0 = 0u, nan1 = 0u;
  masked_scan(x0, x1, mu8, mf, n, [&](int64_t, float a, float b) {
    const unsigned ka = sel_key(a), kb = sel_key(b);
    if (((ka ^ p0) & hm) == 0u) {
      const unsigned d = (ka >> shift) & 255u;
      if (d == d0) c0++;
      else { if (c0) atomicAdd(&h[d0], c0); d0 = d; c0 = 1u; }
    }
    if (((kb ^ p1) & hm) == 0u) {
      const unsigned d = (kb >> shift) & 255u;
      if (d == d1) c1++;
      else { if (c1) atomicAdd(&h[SEL_BINS + d1], c1); d1 = d; c1 = 1u; }
    }
    nan0 += a != a ? 1u : 0u; nan1 += b != b ? 1u : 0u;
  });
  if (c0) atomicAdd(&h[d0], c0);
  if (c1) atomicAdd(&h[SEL_BINS + d1], c1);
  if (pass == 0) {
    if (nan0) atomicAdd(&snan[0], nan0);
    if (nan1) atomicAdd(&snan[1], nan1);
  }
  __syncthreads();
  unsigned* hist = scratch + pass * 2 * SEL_BINS;
  if (h[t]) atomicAdd(&hist[t], h[t]);
  if (h[t + SEL_BINS]) atomicAdd(&hist[t + SEL_BINS], h[t + SEL_BINS]);
  if (pass == 0 && t < 2 && snan[t]) atomicAdd(&state[ST_NAN0 + t], snan[t]);
}

// one wave: the bin of this pass that holds the rank -> prefix and residual rank; pass 0 also fixes n and the rank (n-1)/2 of the lower
// median; the last pass writes out[4] = [median 0, median 1, n, nan flag] (NaN for an empty selection or one that holds a NaN, as torch.median)
__global__ __launch_bounds__(64) void select_scan_kernel(unsigned* __restrict__ scratch, int pass, float* __restrict__ out) {
  __shared__ unsigned ssum[2][64];
  const int lane = threadIdx.x;
  unsigned* state = scratch + SEL_STATE;
  const unsigned* hist = scratch + pass * 2 * SEL_BINS;
  const int shift = 24 - 8 * pass;
  unsigned c[2][4], s[2];
  for (int sel = 0; sel < 2; sel++) {
    const uint4 v = reinterpret_cast<const uint4*>(hist + sel * SEL_BINS)[lane];
    c[sel][0] = v.x; c[sel][1] = v.y; c[sel][2] = v.z; c[sel][3] = v.w;
    s[sel] = v.x + v.y + v.z + v.w;
    ssum[sel][lane] = s[sel];
  }
  // everything the winners below overwrite is read before the barrier
  unsigned n = state[ST_N];
  unsigned k[2] = {state[ST_K0], state[ST_K1]}, prefix[2] = {state[ST_PREFIX0], state[ST_PREFIX1]};
  const unsigned nans[2] = {state[ST_NAN0], state[ST_NAN1]};
  __syncthreads();
  if (pass == 0) {
    n = 0u;
    for (int l = 0; l < 64; l++) n += ssum[0][l];
    k[0] = k[1] = n ? (n - 1u) / 2u : 0u;
    prefix[0] = prefix[1] = 0u;
    if (lane == 0) state[ST_N] = n;
  }
  for (int sel = 0; sel < 2; sel++) {
    unsigned before = 0u;
    for (int l = 0; l < lane; l++) before += ssum[sel][l];
    if (n > 0u && k[sel] >= before && k[sel] - before < s[sel]) {      // exactly one lane: the bins of a pass sum to more than its rank
      unsigned cum = before;
      int b = 0;
      while (b < 3 && k[sel] - cum >= c[sel][b]) { cum += c[sel][b]; b++; }
      const unsigned p = prefix[sel] | ((unsigned)(lane * 4 + b) << shift);
      state[ST_PREFIX0 + sel] = p;
      state[ST_K0 + sel] = k[sel] - cum;
      if (pass == SEL_PASSES - 1) out[sel] = nans[sel] ? __uint_as_float(0x7fc00000u) : sel_unkey(p);
    }
  }
  if (pass == SEL_PASSES - 1 && lane == 0) {
    if (n == 0u) { out[0] = __uint_as_float(0x7fc00000u); out[1] = __uint_as_float(0x7fc00000u); }
    out[2] = (float)n;
    out[3] = (nans[0] | nans[1]) ? 1.f : 0.f;
  }
}

// ---- the unsupervised term ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float unsup_sgn(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }
// the supervised term's functions (rd_sml.hip): 'l1' |d|, 'l2' d^2, 'smoothl1' with beta 1
__device__ __forceinline__ float unsup_term(float d, int kind) {
  const float a = fabsf(d);
  return kind == 0 ? a : (kind == 1 ? d * d : (a < 1.f ? 0.5f * d * d : a - 0.5f));
}
__device__ __forceinline__ float unsup_dterm(float d, int kind) {
  return kind == 0 ? unsup_sgn(d) : (kind == 1 ? 2.f * d : (fabsf(d) < 1.f ? d : unsup_sgn(d)));
}
__device__ __forceinline__ double unsup_block_sum(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[wv] = v;
  __syncthreads();
  double r = 0.0;
  for (int w = 0; w < (int)(blockDim.x >> 6); w++) r += sh[w];
  return r;
}

// block partials [blk][3] = sum phi(d), sum phi'(d) * o, count(o == m_o) over the selected pixels; d = o / m_o - I / m_I
__global__ __launch_bounds__(256) void sml_unsup_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ image,
                                                            const unsigned char* __restrict__ mu8, const float* __restrict__ mf, int64_t n,
                                                            int kind, const float* __restrict__ med, double* __restrict__ partial) {
  __shared__ double sh[4];
  const float mo = med[0], mi = med[1];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  masked_scan(pred, image, mu8, mf, n, [&](int64_t, float o, float im) {
    const float d = o / mo - im / mi;
    a0 += (double)unsup_term(d, kind);
    a1 += (double)unsup_dterm(d, kind) * (double)o;
    a2 += o == mo ? 1.0 : 0.0;
  });
  a0 = unsup_block_sum(a0, sh); a1 = unsup_block_sum(a1, sh); a2 = unsup_block_sum(a2, sh);
  if (threadIdx.x == 0) {
    partial[(int64_t)blockIdx.x * 3 + 0] = a0; partial[(int64_t)blockIdx.x * 3 + 1] = a1; partial[(int64_t)blockIdx.x * 3 + 2] = a2;
  }
}
// uinfo[8] = [loss_unsupervised, m_o, m_I, n, c (selected pixels equal to m_o), dL/dm_o, nan flag, 0]; info[0] += w_u * loss_unsupervised
__global__ __launch_bounds__(64) void sml_unsup_finalize_kernel(const double* __restrict__ partial, int rows, const unsigned* __restrict__ scratch,
                                                                const float* __restrict__ med, float w_u, float* __restrict__ uinfo,
                                                                float* __restrict__ info) {
  // one wave: lanes stride over the rows, double-precision xor tree (fixed order)
  const int lane = threadIdx.x;
  double a[3] = {0.0, 0.0, 0.0};
  for (int r = lane; r < rows; r += 64)      // the three loads of a row are independent: one round trip per row, not three
    for (int j = 0; j < 3; j++) a[j] += partial[(int64_t)r * 3 + j];
  for (int j = 0; j < 3; j++) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a[j] += __shfl_xor(a[j], o);
  }
  if (lane) return;
  const double n = (double)scratch[SEL_STATE + ST_N], mo = (double)med[0];
  const double lu = a[0] / n;      // 0 / 0 = NaN for an empty selection, as the reference's mean over nothing
  uinfo[0] = (float)lu; uinfo[1] = med[0]; uinfo[2] = med[1]; uinfo[3] = (float)n; uinfo[4] = (float)a[2];
  uinfo[5] = (float)(-a[1] / (n * mo * mo)); uinfo[6] = med[3]; uinfo[7] = 0.f;
  if (info) info[0] = (float)((double)info[0] + (double)w_u * lu);
}
// dpred_i += dloss * w_u * (phi'(d_i) / (n m_o) + [o_i == m_o] / c * dL/dm_o) on the selected pixels: torch's median backward spreads the
// gradient evenly over the c tied elements, so it does not matter which of them a selection lands on
__global__ __launch_bounds__(256) void sml_unsup_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ image,
                                                            const unsigned char* __restrict__ mu8, const float* __restrict__ mf, int64_t n,
                                                            int kind, float w_u, const float* __restrict__ uinfo, const float* __restrict__ dloss,
                                                            float* __restrict__ dpred) {
  const float mo = uinfo[1], mi = uinfo[2];
  const float gl = dloss[0] * w_u;
  const float c_main = 1.f / (uinfo[3] * mo), c_med = uinfo[5] / uinfo[4];
  masked_scan(pred, image, mu8, mf, n, [&](int64_t i, float o, float im) {
    const float d = o / mo - im / mi;
    float g = c_main * unsup_dterm(d, kind);
    if (o == mo) g += c_med;
    dpred[i] += gl * g;
  });
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------------
int64_t masked_median_bytes(int64_t) { return (int64_t)SEL_WORDS * 4; }
void launch_masked_median(const float* x0, const float* x1, const unsigned char* mu8, const float* mf, int64_t n, void* scratch, float* out,
                          hipStream_t st) {
  unsigned* s = reinterpret_cast<unsigned*>(scratch);
  hipLaunchKernelGGL(select_zero_kernel, dim3(1), dim3(256), 0, st, s);
  const unsigned grid = sel_grid(n);
  for (int pass = 0; pass < SEL_PASSES; pass++) {
    hipLaunchKernelGGL(select_count_kernel, dim3(grid), dim3(256), 0, st, x0, x1, mu8, mf, n, s, pass);
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(64), 0, st, s, pass, out);
  }
}
int64_t sml_unsup_bytes(int64_t n) { return UNSUP_PART_OFF + (int64_t)unsup_rows(n) * 3 * 8; }
void launch_sml_unsup_fwd(const float* pred, const float* image, const unsigned char* mu8, const float* mf, int64_t n, int kind, float w_u,
                          void* scratch, float* uinfo, float* info, hipStream_t st) {
  char* base = reinterpret_cast<char*>(scratch);
  float* med = reinterpret_cast<float*>(base + UNSUP_MED_OFF);
  double* partial = reinterpret_cast<double*>(base + UNSUP_PART_OFF);
  launch_masked_median(pred, image, mu8, mf, n, scratch, med, st);
  const unsigned grid = unsup_rows(n);
  hipLaunchKernelGGL(sml_unsup_fwd_kernel, dim3(grid), dim3(256), 0, st, pred, image, mu8, mf, n, kind, med, partial);
  hipLaunchKernelGGL(sml_unsup_finalize_kernel, dim3(1), dim3(64), 0, st, partial, (int)grid, reinterpret_cast<const unsigned*>(scratch), med, w_u,
                     uinfo, info);
}
void launch_sml_unsup_bwd(const float* pred, const float* image, const unsigned char* mu8, const float* mf, int64_t n, int kind, float w_u,
                          const float* uinfo, const float* dloss, float* dpred, hipStream_t st) {
  hipLaunchKernelGGL(sml_unsup_bwd_kernel, dim3(unsup_bwd_grid(n)), dim3(256), 0, st, pred, image, mu8, mf, n, kind, w_u, uinfo, dloss, dpred);
}

}  // namespace rd
