// Scale-Map-Learner options outside the ZJU default: the direct-regression head of MidasNet_small_depth (model_type 'midas-small-depth',
// modules/midas/midas_net_custom.py:240-257) and the ground-truth dilation (train_zju.py:158-165, :363-364).  Three streaming kernels:
//
//   sml_depth_head_fwd   pred = relu(1 + out); pred > hi -> hi; pred < lo -> lo   (hi = 1/min_pred, lo = 1/max_pred; < 0 disables a clamp)
//   sml_depth_head_bwd   dout = dpred where 1 + out > 0 and neither clamp took the value (strict comparisons), else 0: what autograd gives the
//                        reference's clone() + masked in-place assignment
//   maxpool_dilate       torch.nn.MaxPool2d(k, stride=1, padding=k//2) on (N,1,H,W) fp32 maps: the maximum over the window clipped to the image
//
// The head kernels move one 16-byte vector of `out` per thread and step (4 fp32 or 8 16-bit elements; pred / dpred are fp32, so the 16-bit
// build moves two fp32 vectors next to it) when every pointer is 16-byte aligned, and finish the n % VE elements behind the last whole vector
// one by one; with a misaligned pointer every element takes that scalar form.  The dilation computes four neighbouring outputs of a row per
// thread when W % 4 == 0 (rows then start on 16-byte boundaries): per window row one 16-byte load of the centre and k - 1 scalar loads of the
// halo, every value compared into the outputs whose window holds it.  Other widths take one output per thread.
#include "rd_common.h"
#include "rd_kernels.h"

namespace rd {

// -> pred; pass = the gradient goes through (relu open, value not replaced by a clamp)
__device__ __forceinline__ float depth_head(float o, float hi, float lo, bool& pass) {
  const float s = 1.f + o;
  float p = s > 0.f ? s : 0.f;
  const bool over = hi > 0.f && p > hi, under = lo > 0.f && p < lo;
  pass = s > 0.f && !over && !under;
  if (over) p = hi;
  if (lo > 0.f && p < lo) p = lo;
  return p;
}

// nv whole vectors of VE elements, then the elements [nv * VE, n) one by one
template <typename T>
__global__ __launch_bounds__(256) void sml_depth_head_fwd_kernel(const T* __restrict__ out, float* __restrict__ pred, int64_t n, int64_t nv,
                                                                 float hi, float lo) {
  constexpr int VE = Elem<T>::VE;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = t0; i < nv; i += step) {
    float o[VE];
    ldv(out + i * VE, o);
    bool pass;
#pragma unroll
    for (int q = 0; q < VE; q += 4) {
      float p[4];
#pragma unroll
      for (int j = 0; j < 4; j++) p[j] = depth_head(o[q + j], hi, lo, pass);
      st4(pred + i * VE + q, p);
    }
  }
  for (int64_t i = nv * VE + t0; i < n; i += step) {
    bool pass;
    pred[i] = depth_head(Elem<T>::ld(out + i), hi, lo, pass);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void sml_depth_head_bwd_kernel(const T* __restrict__ out, const float* __restrict__ dpred, T* __restrict__ dout,
                                                                 int64_t n, int64_t nv, float hi, float lo) {
  constexpr int VE = Elem<T>::VE;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = t0; i < nv; i += step) {
    float o[VE], g[VE];
    ldv(out + i * VE, o);
#pragma unroll
    for (int q = 0; q < VE; q += 4) {
      float d[4];
      ld4(dpred + i * VE + q, d);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        bool pass;
        depth_head(o[q + j], hi, lo, pass);
        g[q + j] = pass ? d[j] : 0.f;
      }
    }
    stv(dout + i * VE, g);
  }
  for (int64_t i = nv * VE + t0; i < n; i += step) {
    bool pass;
    depth_head(Elem<T>::ld(out + i), hi, lo, pass);
    Elem<T>::st(dout + i, pass ? dpred[i] : 0.f);
  }
}

// torch's comparison: a larger value or a NaN replaces the running maximum (ties keep the first value met, rows then columns ascending)
__device__ __forceinline__ float dilate_take(float m, float v) { return (v > m || v != v) ? v : m; }

// One item = V neighbouring outputs (y, x .. x + V - 1) of one plane.  V == 4 needs W % 4 == 0 and 16-byte aligned planes.
template <int V>
__global__ __launch_bounds__(256) void maxpool_dilate_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W, int r) {
  const int Wv = W / V;
  const int64_t total = (int64_t)N * H * Wv;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = i / Wv;
    const int c = (int)(i - q * Wv) * V, row = (int)(q % H);
    const float* __restrict__ plane = x + (q - row) * W;      // (q - row) = n * H
    float m[V];
#pragma unroll
    for (int j = 0; j < V; j++) m[j] = -__builtin_huge_valf();
    const int r0 = max(row - r, 0), r1 = min(row + r, H - 1);
    const int c0 = max(c - r, 0), c1 = min(c + V - 1 + r, W - 1);
    for (int rr = r0; rr <= r1; rr++) {
      const float* __restrict__ src = plane + (int64_t)rr * W;
      // left halo: column u belongs to the windows of the outputs j with c + j - r <= u, i.e. j <= u - c + r
      for (int u = c0; u < c; u++) {
        const float v = src[u];
#pragma unroll
        for (int j = 0; j < V; j++)
          if (j <= u - c + r) m[j] = dilate_take(m[j], v);
      }
      float ctr[V];
      if constexpr (V == 4) ld4(src + c, ctr);
      else ctr[0] = src[c];
#pragma unroll
      for (int e = 0; e < V; e++) {
#pragma unroll
        for (int j = 0; j < V; j++)
          if (e - j <= r && j - e <= r) m[j] = dilate_take(m[j], ctr[e]);
      }
      // right halo: column u belongs to the outputs j with u <= c + j + r
      for (int u = c + V; u <= c1; u++) {
        const float v = src[u];
#pragma unroll
        for (int j = 0; j < V; j++)
          if (j >= u - c - r) m[j] = dilate_take(m[j], v);
      }
    }
    float* dst = y + q * W + c;
    if constexpr (V == 4) st4(dst, m);
    else dst[0] = m[0];
  }
}

static unsigned stream_grid(int64_t items) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(items, 256), 4096)); }
static bool aligned16(const void* a, const void* b, const void* c = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

void launch_sml_depth_head_fwd(const void* out, float* pred, int64_t n, float hi, float lo, int dtype, hipStream_t st) {
  const int64_t nv = aligned16(out, pred) ? n / elem_vec(dtype) : 0;
  const unsigned grid = stream_grid(std::max<int64_t>(nv, nv ? 0 : n));
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
    hipLaunchKernelGGL((sml_depth_head_fwd_kernel<T>), dim3(grid), dim3(256), 0, st, (const T*)out, pred, n, nv, hi, lo); });
}
void launch_sml_depth_head_bwd(const void* out, const float* dpred, void* dout, int64_t n, float hi, float lo, int dtype, hipStream_t st) {
  const int64_t nv = aligned16(out, dpred, dout) ? n / elem_vec(dtype) : 0;
  const unsigned grid = stream_grid(std::max<int64_t>(nv, nv ? 0 : n));
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
    hipLaunchKernelGGL((sml_depth_head_bwd_kernel<T>), dim3(grid), dim3(256), 0, st, (const T*)out, dpred, (T*)dout, n, nv, hi, lo); });
}
void launch_maxpool_dilate(const float* x, float* y, int N, int H, int W, int k, hipStream_t st) {
  const bool vec = (W & 3) == 0 && aligned16(x, y);
  const int64_t items = (int64_t)N * H * (vec ? W / 4 : W);
  if (vec) hipLaunchKernelGGL((maxpool_dilate_kernel<4>), dim3(stream_grid(items)), dim3(256), 0, st, x, y, N, H, W, k / 2);
  else hipLaunchKernelGGL((maxpool_dilate_kernel<1>), dim3(stream_grid(items)), dim3(256), 0, st, x, y, N, H, W, k / 2);
}

}  // namespace rd
