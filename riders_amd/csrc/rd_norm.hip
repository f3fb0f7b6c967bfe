// BatchNorm (training/eval), activation, LayerNorm and bias-gradient kernels.  HBM-bound, NHWC.
//
// Reference semantics:
//   utils/net_utils.py:84-91    conv -> torch.nn.BatchNorm2d (train: biased batch var for the
//                               normalisation, unbiased var into running_var, momentum 0.1) -> act
//   utils/net_utils.py:15       LeakyReLU(negative_slope=0.20)
//   utils/net_utils.py:309-323  ResNetBlock: act(conv2 + X)  (residual folded into rd_affine_act)
//   RCNet/linear_attention.py:106-107,125,131  nn.LayerNorm(d_model), eps 1e-5, biased var
//
// BN statistics come from the convolution epilogue as per-block partial (sum, sum^2) rows; they are
// combined here in a fixed order in double precision (deterministic).
#include "rd_common.h"
#include "rd_kernels.h"
#include <type_traits>
#include <stdio.h>

namespace rd {

// pixels per thread of the forward `*_gen` apply kernel's grid (A/B hook: RD_BN_GEN_PPT; SML step 1227-1231 img/s at 2, 1247 at 8, 1243 at 16)
static int gen_ppt() { return rd_opt(OPT_BN_GEN_PPT, 8); }

// ---- BN finalize: partial[rows][C][2] -> mean/rstd + fused scale/shift, running-stat update ----
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ partial, int rows, int C, double count,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float eps, float momentum, int training, float* running_mean,
                                                          float* running_var, float* mean_out, float* rstd_out,
                                                          float* scale, float* shift) {
  __shared__ double s1[4], s2[4];
  const int c = blockIdx.x, t = threadIdx.x;
  float mean, var;
  if (training) {
    // float2 loads, lanes stride over the partial rows; wave shuffle + 4-entry LDS combine (fixed order, double precision)
    const float2* p2 = reinterpret_cast<const float2*>(partial);
    double a = 0.0, b = 0.0;
    bn_rows_sum(p2, rows, C, c, t, a, b);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    if ((t & 63) == 0) { s1[t >> 6] = a; s2[t >> 6] = b; }
    __syncthreads();
    const double sa = (s1[0] + s1[1]) + (s1[2] + s1[3]), sb = (s2[0] + s2[1]) + (s2[2] + s2[3]);
    double m = sa / count;
    double v = sb / count - m * m;
    if (v < 0.0) v = 0.0;
    mean = (float)m; var = (float)v;
    if (t == 0 && running_mean) {
      double unb = count > 1.0 ? v * count / (count - 1.0) : v;
      running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
      running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unb;
    }
  } else {
    mean = running_mean[c]; var = running_var[c];
  }
  if (t == 0) {
    float rstd = 1.0f / sqrtf(var + eps);
    float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    if (mean_out) mean_out[c] = mean;
    if (rstd_out) rstd_out[c] = rstd;
    scale[c] = g * rstd;
    shift[c] = b - mean * g * rstd;
  }
}

// ---- z = act(scale[c]*y + shift[c] + res) ---------------------------------------------------------
template <typename T, bool V4>
__global__ __launch_bounds__(256) void affine_act_kernel(const T* __restrict__ y, const float* __restrict__ scale,
                                                         const float* __restrict__ shift, const T* __restrict__ res,
                                                         T* __restrict__ out, int64_t total, int C, int act, float slope) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (V4) {
    int64_t nv = total >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
      int c = (int)((i << 2) % C);
      float v[4], r[4] = {0.f, 0.f, 0.f, 0.f};
      ld4(y + (i << 2), v);
      if (res) ld4(res + (i << 2), r);
#pragma unroll
      for (int e = 0; e < 4; e++) {
        float s = scale ? scale[c + e] : 1.f, b = shift ? shift[c + e] : 0.f;
        const float u = v[e] * s + b;
        v[e] = act_fwd(res ? u + r[e] : u, act, slope);
      }
      st4(out + (i << 2), v);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
      int c = (int)(i % C);
      float s = scale ? scale[c] : 1.f, b = shift ? shift[c] : 0.f;
      const float u = Elem<T>::ld(y + i) * s + b;
      Elem<T>::st(out + i, act_fwd(res ? u + Elem<T>::ld(res + i) : u, act, slope));
    }
  }
}

// ---- per-channel column reductions over an NHWC [pixels][C] tensor --------------------------------
// thread = (pixel lane pl, channel cl); a block covers BC = min(C,256)-rounded channels x a pixel range
struct RedGeom { int CB, PL, nchunk; };
static RedGeom red_geom(int C) {
  RedGeom g;
  int cb = 1; while (cb < C && cb < 256) cb <<= 1;
  g.CB = cb; g.PL = 256 / cb; g.nchunk = (int)cdiv(C, cb);
  return g;
}
static int red_rows(int64_t pixels, int C) {
  RedGeom g = red_geom(C);
  int64_t per_block = (int64_t)g.PL * 64;  // >= 64 pixels per thread-row
  // wider than 256 channels a block of the vector kernels covers only 256 / (C/8) pixels per iteration (one at C = 1392): 64 pixels per block
  // were 32 dependent round trips on 41 blocks for EfficientNet-Lite3's 9x18 maps (16 us for 7 MB); eight iterations per block instead
  if (C > 256) per_block = 8 * std::max<int64_t>(1, 256 / cdiv(C, 8));
  int64_t r = cdiv(pixels, per_block);
  return (int)std::max<int64_t>(1, std::min<int64_t>(r, 4096));   // short per-block loops: the reduce kernels are load-latency bound
}

// MODE 0: (sum dpre, sum dpre*xhat) for BN backward; MODE 1: column sum of x (bias gradient)
template <typename T, int MODE>
__global__ __launch_bounds__(256) void col_reduce_kernel(const T* __restrict__ dz, const T* __restrict__ z,
                                                         const T* __restrict__ y, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, float* __restrict__ partial,
                                                         int64_t pixels, int C, int CB, int PL, int act, float slope) {
  __shared__ float red[2][256];
  const int t = threadIdx.x;
  const int cl = t % CB, pl = t / CB;
  const int c = blockIdx.y * CB + cl;
  const int nrow = gridDim.x;
  const int64_t per = cdiv(pixels, nrow);
  const int64_t pbeg = (int64_t)blockIdx.x * per, pend = pbeg + per < pixels ? pbeg + per : pixels;
  float a = 0.f, b = 0.f;
  if (c < C) {
    float mu = 0.f, rs = 1.f;
    if (MODE == 0) { mu = mean[c]; rs = rstd[c]; }
    int64_t p = pbeg + pl;
    // four pixels' loads in flight per iteration, accumulated in pixel order (the sums are those of the one-pixel loop below, bit for bit):
    // the 3-channel BatchNorm of the SML's `first` layer walked 2.65 M pixels one dependent 2-byte round trip at a time (85 us for 32 MB)
    for (; p + 3 * (int64_t)PL < pend; p += 4 * (int64_t)PL) {
      float g[4], zz[4] = {0.f, 0.f, 0.f, 0.f}, yy[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int64_t i = (p + q * (int64_t)PL) * C + c;
        g[q] = Elem<T>::ld(dz + i);
        if (MODE == 0) { if (act) zz[q] = Elem<T>::ld(z + i); yy[q] = Elem<T>::ld(y + i); }
      }
#pragma unroll
      for (int q = 0; q < 4; q++) {
        if (MODE == 0) {
          float gq = g[q];
          if (act) gq *= act_grad_from_out(zz[q], act, slope);
          const float xh = (yy[q] - mu) * rs;
          a += gq; b += gq * xh;
        } else a += g[q];
      }
    }
    for (; p < pend; p += PL) {
      int64_t i = p * C + c;
      if (MODE == 0) {
        float g = Elem<T>::ld(dz + i);
        if (act) g *= act_grad_from_out(Elem<T>::ld(z + i), act, slope);
        float xh = (Elem<T>::ld(y + i) - mu) * rs;
        a += g; b += g * xh;
      } else {
        a += Elem<T>::ld(dz + i);
      }
    }
  }
  red[0][t] = a; red[1][t] = b;
  __syncthreads();
  if (pl == 0 && c < C) {
    float sa = 0.f, sb = 0.f;
    for (int q = 0; q < PL; q++) { sa += red[0][q * CB + cl]; sb += red[1][q * CB + cl]; }
    partial[((int64_t)blockIdx.x * C + c) * 2] = sa;
    partial[((int64_t)blockIdx.x * C + c) * 2 + 1] = sb;
  }
}

// one workgroup per channel: threads stride over the partial rows (float2 loads), wave shuffle + 4-entry LDS combine in double
// precision (fixed order).  Four waves keep 4x the loads in flight of the one-wave version: this kernel is pure load latency.
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ partial, int rows, int C, double count,
                                                              float* dgamma, float* dbeta, int accumulate, float* c1, float* c2, int row_pitch) {
  __shared__ double s1[4], s2[4];
  const int c = blockIdx.x, t = threadIdx.x;
  const float2* p2 = reinterpret_cast<const float2*>(partial);
  double a = 0.0, b = 0.0;
  bn_rows_sum(p2, rows, row_pitch, c, t, a, b);      // row_pitch = channels per partial row (> C: the rows of a two-destination data gradient)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
  if ((t & 63) == 0) { s1[t >> 6] = a; s2[t >> 6] = b; }
  __syncthreads();
  if (t == 0) {
    a = (s1[0] + s1[1]) + (s1[2] + s1[3]); b = (s2[0] + s2[1]) + (s2[2] + s2[3]);
    if (dbeta) dbeta[c] = accumulate ? dbeta[c] + (float)a : (float)a;
    if (dgamma) dgamma[c] = accumulate ? dgamma[c] + (float)b : (float)b;
    if (c1) c1[c] = (float)(a / count);
    if (c2) c2[c] = (float)(b / count);
  }
}

__global__ __launch_bounds__(64) void colsum_finalize_kernel(const float* __restrict__ partial, int rows, int C, float* out,
                                                             int accumulate) {
  const int c = blockIdx.x, lane = threadIdx.x;
  double a = 0.0;
  for (int r = lane; r < rows; r += 64) a += partial[((int64_t)r * C + c) * 2];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
  if (lane == 0) out[c] = accumulate ? out[c] + (float)a : (float)a;
}

// dy = scale[c] * (dpre - c1[c] - xhat*c2[c]);  dres = dpre
template <typename T, bool V4>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dz, const T* __restrict__ z,
                                                           const T* __restrict__ y, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ scale,
                                                           const float* __restrict__ c1, const float* __restrict__ c2,
                                                           T* __restrict__ dy, T* __restrict__ dres, int64_t total, int C,
                                                           int act, float slope) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (V4) {
    int64_t nv = total >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
      int c = (int)((i << 2) % C);
      float g[4], zz[4], yy[4], o[4];
      ld4(dz + (i << 2), g);
      if (act) { ld4(z + (i << 2), zz); }
      ld4(y + (i << 2), yy);
#pragma unroll
      for (int e = 0; e < 4; e++) {
        if (act) g[e] *= act_grad_from_out(zz[e], act, slope);
        float xh = (yy[e] - mean[c + e]) * rstd[c + e];
        o[e] = scale[c + e] * (g[e] - c1[c + e] - xh * c2[c + e]);
      }
      st4(dy + (i << 2), o);
      if (dres) st4(dres + (i << 2), g);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
      int c = (int)(i % C);
      float g = Elem<T>::ld(dz + i);
      if (act) g *= act_grad_from_out(Elem<T>::ld(z + i), act, slope);
      float xh = (Elem<T>::ld(y + i) - mean[c]) * rstd[c];
      Elem<T>::st(dy + i, scale[c] * (g - c1[c] - xh * c2[c]));
      if (dres) Elem<T>::st(dres + i, g);
    }
  }
}


// ---- 16-byte-vector forms (C % VE == 0 and C/VE divides 256): a thread keeps the same VE channels for the whole grid-stride loop, so
// the per-channel parameters live in registers and every memory instruction moves 16 bytes per lane.  The scalar forms above issued
// 2-byte loads plus five parameter loads per element and ran 5-17x off the HBM roofline (rocprofv3: col_reduce 116 us/launch). ------------
template <typename T, int ACT, bool HAS_RES>
__global__ __launch_bounds__(256) void affine_act_vec_kernel(const T* __restrict__ y, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, const T* __restrict__ res,
                                                             T* __restrict__ out, int64_t nvec, int C, int act, float slope) {
  constexpr int VE = Elem<T>::VE;
  const int actv = ACT >= 0 ? ACT : act;   // compile-time activation where the launcher knows it
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c0 = (int)((i * VE) % C);
  float sc[VE], sh[VE];
#pragma unroll
  for (int e = 0; e < VE; e++) { sc[e] = scale ? scale[c0 + e] : 1.f; sh[e] = shift ? shift[c0 + e] : 0.f; }
  // four vectors per iteration, all requests in flight before the first is used (ew_grid4 gives a thread at least four): on the 10-45 MB
  // tensors of the encoder stages a thread had ONE vector next to 64 bytes of coefficient loads, on 2048 blocks
  for (; i + 3 * stride < nvec; i += 4 * stride) {
    float v[4][VE], r[HAS_RES ? 4 : 1][VE];
#pragma unroll
    for (int q = 0; q < 4; q++) { ldv(y + (i + q * stride) * VE, v[q]); if (HAS_RES) ldv(res + (i + q * stride) * VE, r[q]); }
#pragma unroll
    for (int q = 0; q < 4; q++) {
#pragma unroll
      for (int e = 0; e < VE; e++) {
        const float u = v[q][e] * sc[e] + sh[e];
        v[q][e] = act_fwd(HAS_RES ? u + r[HAS_RES ? q : 0][e] : u, actv, slope);
      }
      stv(out + (i + q * stride) * VE, v[q]);
    }
  }
  for (; i < nvec; i += stride) {
    float v[VE], r[VE];
    ldv(y + i * VE, v);
    if (HAS_RES) ldv(res + i * VE, r);
#pragma unroll
    for (int e = 0; e < VE; e++) {      // without a residual exactly bn_apply1 (rd_conv_common.h): consumers that apply BatchNorm while staging reproduce z bit for bit
      const float u = v[e] * sc[e] + sh[e];
      v[e] = act_fwd(HAS_RES ? u + r[e] : u, actv, slope);
    }
    stv(out + i * VE, v);
  }
}

// out = act2(round(act1(scale * y + shift)) + res): the BatchNorm apply + activation of a residual block's second convolution
// (utils/net_utils.py:309-321: conv2 is a conv -> BatchNorm -> act module) fused with the block's add + activation (:323).  The inner
// value is rounded to the activation type exactly where rd_affine_act would have stored it, so the result equals the two-pass form.
template <typename T, int ACT1, int ACT2>
__global__ __launch_bounds__(256) void affine_act_add_vec_kernel(const T* __restrict__ y, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, const T* __restrict__ res,
                                                                 T* __restrict__ out, int64_t nvec, int C, int act1, float slope1, int act2, float slope2) {
  constexpr int VE = Elem<T>::VE;
  const int a1 = ACT1 >= 0 ? ACT1 : act1, a2 = ACT2 >= 0 ? ACT2 : act2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c0 = (int)((i * VE) % C);
  float sc[VE], sh[VE];
#pragma unroll
  for (int e = 0; e < VE; e++) { sc[e] = scale[c0 + e]; sh[e] = shift[c0 + e]; }
  for (; i < nvec; i += stride) {
    float v[VE], r[VE];
    ldv(y + i * VE, v);
    ldv(res + i * VE, r);
#pragma unroll
    for (int e = 0; e < VE; e++) {
      const float z = Elem<T>::rnd(act_fwd(v[e] * sc[e] + sh[e], a1, slope1));
      v[e] = act_fwd(z + r[e], a2, slope2);
    }
    stv(out + i * VE, v);
  }
}

template <typename T, bool RC, int ACT>
__global__ __launch_bounds__(256) void bn_bwd_apply_vec_kernel(const T* __restrict__ dz, const T* __restrict__ z,
                                                               const T* __restrict__ y, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, const float* __restrict__ scale,
                                                               const float* __restrict__ c1, const float* __restrict__ c2, const float* __restrict__ shift,
                                                               T* __restrict__ dy, T* __restrict__ dres, int64_t nvec, int C,
                                                               int act, float slope) {
  constexpr int VE = Elem<T>::VE;
  const int actv = ACT >= 0 ? ACT : act;   // compile-time activation where the launcher knows it
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c0 = (int)((i * VE) % C);
  float mu[VE], rs[VE], sc[VE], k1[VE], k2[VE], sh[VE];
#pragma unroll
  for (int e = 0; e < VE; e++) {
    mu[e] = mean[c0 + e]; rs[e] = rstd[c0 + e]; sc[e] = scale[c0 + e]; k1[e] = c1[c0 + e]; k2[e] = c2[c0 + e];
    sh[e] = RC ? shift[c0 + e] : 0.f;
  }
  for (; i + stride < nvec; i += 2 * stride) {      // two vectors per iteration (see affine_act_vec_kernel)
    float g[2][VE], zz[2][VE], yy[2][VE], o[VE];
#pragma unroll
    for (int q = 0; q < 2; q++) {
      ldv(dz + (i + q * stride) * VE, g[q]);
      if (actv && !RC) ldv(z + (i + q * stride) * VE, zz[q]);
      ldv(y + (i + q * stride) * VE, yy[q]);
    }
#pragma unroll
    for (int q = 0; q < 2; q++) {
#pragma unroll
      for (int e = 0; e < VE; e++) {
        if (actv) g[q][e] *= act_grad_from_out(RC ? yy[q][e] * sc[e] + sh[e] : zz[q][e], actv, slope);
        float xh = (yy[q][e] - mu[e]) * rs[e];
        o[e] = sc[e] * (g[q][e] - k1[e] - xh * k2[e]);
      }
      stv(dy + (i + q * stride) * VE, o);
      if (dres) stv(dres + (i + q * stride) * VE, g[q]);
    }
  }
  for (; i < nvec; i += stride) {
    float g[VE], zz[VE], yy[VE], o[VE];
    ldv(dz + i * VE, g);
    if (actv && !RC) ldv(z + i * VE, zz);
    ldv(y + i * VE, yy);
#pragma unroll
    for (int e = 0; e < VE; e++) {
      // shift given: the activation's argument is recomputed from y exactly as the forward computed it (no read of z)
      if (actv) g[e] *= act_grad_from_out(RC ? yy[e] * sc[e] + sh[e] : zz[e], actv, slope);
      float xh = (yy[e] - mu[e]) * rs[e];
      o[e] = sc[e] * (g[e] - k1[e] - xh * k2[e]);
    }
    stv(dy + i * VE, o);
    if (dres) stv(dres + i * VE, g);
  }
}

// MODE 0: (sum dpre, sum dpre*xhat); MODE 1: column sum.  Block b reduces pixels [b*per, (b+1)*per); thread t owns channel group t % VP.
template <typename T, int MODE, bool RC, int ACT>
__global__ __launch_bounds__(256) void col_reduce_vec_kernel(const T* __restrict__ dz, const T* __restrict__ z,
                                                             const T* __restrict__ y, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, float* __restrict__ partial,
                                                             int64_t pixels, int C, int act, float slope, const float* __restrict__ scale,
                                                             const float* __restrict__ shift) {
  constexpr int VE = Elem<T>::VE;
  const int actv = ACT >= 0 ? ACT : act;   // compile-time activation where the launcher knows it
  __shared__ float red[256 * VE * 2];
  const int t = threadIdx.x, lane = t & 63;
  const int VP = C / VE;
  const int64_t per = cdiv(pixels, (int64_t)gridDim.x);
  const int64_t pbeg = (int64_t)blockIdx.x * per, pend = pbeg + per < pixels ? pbeg + per : pixels;
  const int c0 = (t % VP) * VE;
  float mu[VE], rs[VE], a[VE], b[VE], sq[VE], hq[VE];
#pragma unroll
  for (int e = 0; e < VE; e++) {
    a[e] = 0.f; b[e] = 0.f;
    mu[e] = MODE == 0 ? mean[c0 + e] : 0.f; rs[e] = MODE == 0 ? rstd[c0 + e] : 1.f;
    sq[e] = RC ? scale[c0 + e] : 0.f; hq[e] = RC ? shift[c0 + e] : 0.f;
  }
  const int64_t vend = pend * VP;
  auto accum = [&](const float (&g0)[VE], const float (&zz)[VE], const float (&yy)[VE]) RD_INLINE_LAMBDA {
#pragma unroll
    for (int e = 0; e < VE; e++) {
      float gg = g0[e];
      if (MODE == 0) {
        if (actv) gg *= act_grad_from_out(RC ? yy[e] * sq[e] + hq[e] : zz[e], actv, slope);
        a[e] += gg; b[e] += gg * ((yy[e] - mu[e]) * rs[e]);
      } else a[e] += gg;
    }
  };
  int64_t i = pbeg * VP + t;
  for (; i + 256 < vend; i += 512) {   // two independent load sets in flight per iteration
    float g0[VE], z0[VE], y0[VE], g1[VE], z1[VE], y1[VE];
    ldv(dz + i * VE, g0); ldv(dz + (i + 256) * VE, g1);
    if (MODE == 0) {
      if (actv && !RC) { ldv(z + i * VE, z0); ldv(z + (i + 256) * VE, z1); }
      ldv(y + i * VE, y0); ldv(y + (i + 256) * VE, y1);
    }
    accum(g0, z0, y0); accum(g1, z1, y1);
  }
  for (; i < vend; i += 256) {
    float g0[VE], z0[VE], y0[VE];
    ldv(dz + i * VE, g0);
    if (MODE == 0) { if (actv && !RC) ldv(z + i * VE, z0); ldv(y + i * VE, y0); }
    accum(g0, z0, y0);
  }
  // lanes of a wave that share a channel group (lane % VP), fixed xor tree
  for (int o = 32; o >= VP; o >>= 1) {
#pragma unroll
    for (int e = 0; e < VE; e++) { a[e] += __shfl_xor(a[e], o); if (MODE == 0) b[e] += __shfl_xor(b[e], o); }
  }
#pragma unroll
  for (int e = 0; e < VE; e++) { red[(t * VE + e) * 2] = a[e]; red[(t * VE + e) * 2 + 1] = b[e]; }
  __syncthreads();
  for (int c = t; c < C; c += 256) {
    const int g = c / VE, e = c - g * VE;
    float sa = 0.f, sb = 0.f;
    for (int tt = g; tt < 256; tt += VP)
      if ((tt & 63) < VP) { sa += red[(tt * VE + e) * 2]; sb += red[(tt * VE + e) * 2 + 1]; }
    partial[((int64_t)blockIdx.x * C + c) * 2] = sa;
    partial[((int64_t)blockIdx.x * C + c) * 2 + 1] = sb;
  }
}

// ---- 16-byte-vector forms for ANY channel count with C % VE == 0 and C/VE <= 256 (EfficientNet-Lite3's 24..1392-channel maps):
// thread t owns channel group t % VP of pixel slot t / VP; a block covers PPB = 256 / VP consecutive pixels per iteration, so the
// accesses of a block stay one contiguous span and the per-channel parameters still live in registers. ------------------------------
template <typename T, int ACT, bool HAS_RES>
__global__ __launch_bounds__(256) void affine_act_gen_kernel(const T* __restrict__ y, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, const T* __restrict__ res,
                                                             T* __restrict__ out, int64_t pixels, int C, int act, float slope) {
  constexpr int VE = Elem<T>::VE;
  const int actv = ACT >= 0 ? ACT : act;   // compile-time activation where the launcher knows it
  const int VP = C / VE, PPB = 256 / VP;
  const int g = threadIdx.x % VP, pl = threadIdx.x / VP;
  if (pl >= PPB) return;
  float sc[VE], sh[VE];
#pragma unroll
  for (int e = 0; e < VE; e++) { sc[e] = scale ? scale[g * VE + e] : 1.f; sh[e] = shift ? shift[g * VE + e] : 0.f; }
  // two pixels per iteration: both requests are in flight before either is used (the EfficientNet maps are small enough that a wave with one
  // outstanding 16-byte load per lane is latency-bound: waves spent half their cycles waiting, PMC round 2)
  const int64_t step = (int64_t)gridDim.x * PPB;
  int64_t p = (int64_t)blockIdx.x * PPB + pl;
  if (!HAS_RES) {
    // four pixels per iteration (the grid gives a thread eight): the small EfficientNet maps (2.6-41 K pixels x 288-1392 channels) are a
    // few hundred blocks, and a thread's iterations are dependent memory round trips -- 16.8 us for 24 MB with one two-pixel iteration
    // on 1728 blocks (whose per-thread coefficient loads outweighed the data), 10.7 with four on 432, 4-pixel batches below
    for (; p + 3 * step < pixels; p += 4 * step) {
      float v[4][VE];
#pragma unroll
      for (int q = 0; q < 4; q++) ldv(y + (p + q * step) * C + g * VE, v[q]);
#pragma unroll
      for (int q = 0; q < 4; q++) {
#pragma unroll
        for (int e = 0; e < VE; e++) { const float u = v[q][e] * sc[e] + sh[e]; v[q][e] = act_fwd(u, actv, slope); }
        stv(out + (p + q * step) * C + g * VE, v[q]);
      }
    }
  }
  for (; p + step < pixels; p += 2 * step) {
    const int64_t o0 = p * C + g * VE, o1 = (p + step) * C + g * VE;
    float v0[VE], v1[VE], r0[VE], r1[VE];
    ldv(y + o0, v0); ldv(y + o1, v1);
    if (HAS_RES) { ldv(res + o0, r0); ldv(res + o1, r1); }
#pragma unroll
    for (int e = 0; e < VE; e++) {
      { const float u = v0[e] * sc[e] + sh[e]; v0[e] = act_fwd(HAS_RES ? u + r0[e] : u, actv, slope); }
      { const float u = v1[e] * sc[e] + sh[e]; v1[e] = act_fwd(HAS_RES ? u + r1[e] : u, actv, slope); }
    }
    stv(out + o0, v0); stv(out + o1, v1);
  }
  for (; p < pixels; p += step) {
    const int64_t o = p * C + g * VE;
    float v[VE], r[VE];
    ldv(y + o, v);
    if (HAS_RES) ldv(res + o, r);
#pragma unroll
    for (int e = 0; e < VE; e++) { const float u = v[e] * sc[e] + sh[e]; v[e] = act_fwd(HAS_RES ? u + r[e] : u, actv, slope); }
    stv(out + o, v);
  }
}

template <typename T, bool RC, int ACT>
__global__ __launch_bounds__(256) void bn_bwd_apply_gen_kernel(const T* __restrict__ dz, const T* __restrict__ z,
                                                               const T* __restrict__ y, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, const float* __restrict__ scale,
                                                               const float* __restrict__ c1, const float* __restrict__ c2, const float* __restrict__ shift,
                                                               T* __restrict__ dy, T* __restrict__ dres, int64_t pixels, int C,
                                                               int act, float slope) {
  constexpr int VE = Elem<T>::VE;
  const int actv = ACT >= 0 ? ACT : act;   // compile-time activation where the launcher knows it
  const int VP = C / VE, PPB = 256 / VP;
  const int g = threadIdx.x % VP, pl = threadIdx.x / VP;
  if (pl >= PPB) return;
  float mu[VE], rs[VE], sc[VE], k1[VE], k2[VE], sh[VE];
#pragma unroll
  for (int e = 0; e < VE; e++) {
    const int c = g * VE + e;
    mu[e] = mean[c]; rs[e] = rstd[c]; sc[e] = scale[c]; k1[e] = c1[c]; k2[e] = c2[c]; sh[e] = RC ? shift[c] : 0.f;
  }
  auto one = [&](int64_t o, float (&gg)[VE], const float (&zz)[VE], const float (&yy)[VE]) RD_INLINE_LAMBDA {
    float ov[VE];
#pragma unroll
    for (int e = 0; e < VE; e++) {
      if (actv) gg[e] *= act_grad_from_out(RC ? yy[e] * sc[e] + sh[e] : zz[e], actv, slope);
      const float xh = (yy[e] - mu[e]) * rs[e];
      ov[e] = sc[e] * (gg[e] - k1[e] - xh * k2[e]);
    }
    stv(dy + o, ov);
    if (dres) stv(dres + o, gg);
  };
  // two pixels per iteration, all requests issued before the first use (small maps are latency-bound otherwise)
  const int64_t step = (int64_t)gridDim.x * PPB;
  int64_t p = (int64_t)blockIdx.x * PPB + pl;
  for (; p + step < pixels; p += 2 * step) {
    const int64_t o0 = p * C + g * VE, o1 = (p + step) * C + g * VE;
    float g0[VE], z0[VE], y0[VE], g1[VE], z1[VE], y1[VE];
    ldv(dz + o0, g0); ldv(dz + o1, g1);
    if (actv && !RC) { ldv(z + o0, z0); ldv(z + o1, z1); }
    ldv(y + o0, y0); ldv(y + o1, y1);
    one(o0, g0, z0, y0); one(o1, g1, z1, y1);
  }
  for (; p < pixels; p += step) {
    const int64_t o = p * C + g * VE;
    float gg[VE], zz[VE], yy[VE];
    ldv(dz + o, gg);
    if (actv && !RC) ldv(z + o, zz);
    ldv(y + o, yy);
    one(o, gg, zz, yy);
  }
}

template <typename T, int MODE, bool RC, int ACT>
__global__ __launch_bounds__(256) void col_reduce_gen_kernel(const T* __restrict__ dz, const T* __restrict__ z,
                                                             const T* __restrict__ y, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, float* __restrict__ partial,
                                                             int64_t pixels, int C, int act, float slope, const float* __restrict__ scale,
                                                             const float* __restrict__ shift) {
  constexpr int VE = Elem<T>::VE;
  const int actv = ACT >= 0 ? ACT : act;   // compile-time activation where the launcher knows it
  __shared__ float red[256 * VE * 2];
  const int t = threadIdx.x;
  const int VP = C / VE, PPB = 256 / VP;
  const int g = t % VP, pl = t / VP;
  const int64_t per = cdiv(pixels, (int64_t)gridDim.x);
  const int64_t pbeg = (int64_t)blockIdx.x * per, pend = pbeg + per < pixels ? pbeg + per : pixels;
  float mu[VE], rs[VE], a[VE], b[VE], sq[VE], hq[VE];
#pragma unroll
  for (int e = 0; e < VE; e++) {
    a[e] = 0.f; b[e] = 0.f;
    mu[e] = MODE == 0 ? mean[g * VE + e] : 0.f; rs[e] = MODE == 0 ? rstd[g * VE + e] : 1.f;
    sq[e] = RC ? scale[g * VE + e] : 0.f; hq[e] = RC ? shift[g * VE + e] : 0.f;
  }
  auto accum = [&](const float (&g0)[VE], const float (&zz)[VE], const float (&yy)[VE]) RD_INLINE_LAMBDA {
#pragma unroll
    for (int e = 0; e < VE; e++) {
      float gv = g0[e];
      if (MODE == 0) {
        if (actv) gv *= act_grad_from_out(RC ? yy[e] * sq[e] + hq[e] : zz[e], actv, slope);
        a[e] += gv; b[e] += gv * ((yy[e] - mu[e]) * rs[e]);
      } else a[e] += gv;
    }
  };
  if (pl < PPB) {
    int64_t p = pbeg + pl;
    for (; p + PPB < pend; p += 2 * PPB) {   // two independent load sets in flight per iteration
      const int64_t o0 = p * C + g * VE, o1 = (p + PPB) * C + g * VE;
      float g0[VE], z0[VE], y0[VE], g1[VE], z1[VE], y1[VE];
      ldv(dz + o0, g0); ldv(dz + o1, g1);
      if (MODE == 0) {
        if (actv && !RC) { ldv(z + o0, z0); ldv(z + o1, z1); }
        ldv(y + o0, y0); ldv(y + o1, y1);
      }
      accum(g0, z0, y0); accum(g1, z1, y1);
    }
    for (; p < pend; p += PPB) {
      const int64_t o0 = p * C + g * VE;
      float g0[VE], z0[VE], y0[VE];
      ldv(dz + o0, g0);
      if (MODE == 0) { if (actv && !RC) ldv(z + o0, z0); ldv(y + o0, y0); }
      accum(g0, z0, y0);
    }
  }
#pragma unroll
  for (int e = 0; e < VE; e++) { red[(t * VE + e) * 2] = a[e]; red[(t * VE + e) * 2 + 1] = b[e]; }
  __syncthreads();
  for (int c = t; c < C; c += 256) {
    const int gg = c / VE, e = c - gg * VE;
    float sa = 0.f, sb = 0.f;
    for (int q = 0; q < PPB; q++) { sa += red[((q * VP + gg) * VE + e) * 2]; sb += red[((q * VP + gg) * VE + e) * 2 + 1]; }
    partial[((int64_t)blockIdx.x * C + c) * 2] = sa;
    partial[((int64_t)blockIdx.x * C + c) * 2 + 1] = sb;
  }
}
static bool gen_ok(int C, int dtype) {
  const int ve = elem_vec(dtype);
  return (C % ve) == 0 && C / ve <= 256;
}
static bool vec_ok(int C, int dtype) {
  const int ve = elem_vec(dtype);
  if (C % ve) return false;
  const int vp = C / ve;
  return vp <= 256 && (256 % vp) == 0;
}

template <typename T>
__global__ __launch_bounds__(256) void act_bwd_kernel(const T* __restrict__ dz, const T* __restrict__ z, T* __restrict__ dx,
                                                      int64_t n, int act, float slope) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    Elem<T>::st(dx + i, Elem<T>::ld(dz + i) * act_grad_from_out(Elem<T>::ld(z + i), act, slope));
}

// ---- LayerNorm over the last dim (C multiple of 64, <= 512): one wave per row -------------------------
template <typename T>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const T* __restrict__ res,
                                                            T* __restrict__ out, float* __restrict__ mean,
                                                            float* __restrict__ rstd, int64_t rows, int C, float eps) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int epl = C >> 6;  // elements per lane
  for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < rows; r += (int64_t)gridDim.x * 4) {
    float v[8];
    float s = 0.f;
    for (int e = 0; e < epl; e++) { v[e] = Elem<T>::ld(x + r * C + e * 64 + lane); s += v[e]; }
    float mu = wave_sum(s) / (float)C;
    // the sum is C times the size of its terms and carries that rounding into the mean: (x - mu) * rstd was 2e-4 off for rows of mean 100 and
    // spread 0.1.  The first mean, cut to its top 8 significant bits so that x - mu stays exact, plus the mean of the residuals
    mu = __uint_as_float(__float_as_uint(mu) & 0xffff0000u);
    float dm = 0.f;
    for (int e = 0; e < epl; e++) dm += v[e] - mu;
    mu += wave_sum(dm) / (float)C;
    float q = 0.f;
    for (int e = 0; e < epl; e++) { float d = v[e] - mu; q += d * d; }
    float var = wave_sum(q) / (float)C;
    float rs = 1.0f / sqrtf(var + eps);
    for (int e = 0; e < epl; e++) {
      int c = e * 64 + lane;
      float o = (v[e] - mu) * rs * gamma[c] + beta[c];
      if (res) o += Elem<T>::ld(res + r * C + c);
      Elem<T>::st(out + r * C + c, o);
    }
    if (lane == 0) { mean[r] = mu; rstd[r] = rs; }
  }
}

// dx = rstd*(g - mean(g) - xhat*mean(g*xhat)), g = dout*gamma; partial[block][C][2] = (sum dout, sum dout*xhat)
template <typename T>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const T* __restrict__ dout, const T* __restrict__ x,
                                                            const float* __restrict__ gamma, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, T* __restrict__ dx,
                                                            float* __restrict__ partial, int64_t rows, int C) {
  __shared__ float red[4][2][512];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int epl = C >> 6;
  float ag[8], ab[8];
  for (int e = 0; e < 8; e++) { ag[e] = 0.f; ab[e] = 0.f; }
  for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < rows; r += (int64_t)gridDim.x * 4) {
    float mu = mean[r], rs = rstd[r];
    float g[8], xh[8];
    float s1 = 0.f, s2 = 0.f;
    for (int e = 0; e < epl; e++) {
      int c = e * 64 + lane;
      float d = Elem<T>::ld(dout + r * C + c);
      xh[e] = (Elem<T>::ld(x + r * C + c) - mu) * rs;
      g[e] = d * gamma[c];
      s1 += g[e]; s2 += g[e] * xh[e];
      ag[e] += d * xh[e]; ab[e] += d;
    }
    s1 = wave_sum(s1) / (float)C; s2 = wave_sum(s2) / (float)C;
    for (int e = 0; e < epl; e++)
      Elem<T>::st(dx + r * C + e * 64 + lane, rs * (g[e] - s1 - xh[e] * s2));
  }
  for (int e = 0; e < epl; e++) { red[wv][0][e * 64 + lane] = ag[e]; red[wv][1][e * 64 + lane] = ab[e]; }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float a = 0.f, b = 0.f;
    for (int w = 0; w < 4; w++) { a += red[w][0][c]; b += red[w][1][c]; }
    partial[((int64_t)blockIdx.x * C + c) * 2] = b;      // dbeta terms
    partial[((int64_t)blockIdx.x * C + c) * 2 + 1] = a;  // dgamma terms
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------
static unsigned ew_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, 256), 2048)); }
// grid of the apply kernels that take `per` vectors per thread and iteration (A/B hook RD_BN_VEC_PER: 1 = the one-vector grids)
static unsigned ew_grid_per(int64_t n, int per) {
  const int force = rd_opt(OPT_BN_VEC_PER, 0);
  if (force > 0) per = force;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, 256 * (int64_t)per), 2048));
}

void launch_bn_finalize(const float* partial, int rows, int C, double count, const float* gamma, const float* beta,
                        float eps, float momentum, int training, float* running_mean, float* running_var, float* mean,
                        float* rstd, float* scale, float* shift, hipStream_t st) {
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(C), dim3(256), 0, st, partial, rows, C, count, gamma, beta, eps, momentum,
                     training, running_mean, running_var, mean, rstd, scale, shift);
}

void launch_affine_act(const void* y, const float* scale, const float* shift, const void* res, void* out, int64_t pixels,
                       int C, int act, float slope, int dtype, hipStream_t st) {
  int64_t total = pixels * C;
  if (vec_ok(C, dtype)) {
    const int64_t nvec = total / elem_vec(dtype);
    unsigned gv = ew_grid_per(nvec, 4);
    act_dispatch(act, [&](auto ac) {
      constexpr int A = decltype(ac)::value;
      with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
        with_bool(res != nullptr, [&](auto r) {
          hipLaunchKernelGGL((affine_act_vec_kernel<T, A, decltype(r)::value>), dim3(gv), dim3(256), 0, st, (const T*)y, scale, shift, (const T*)res, (T*)out, nvec, C, act, slope); }); });
    });
    return;
  }
  if (gen_ok(C, dtype)) {
    const int ppb = 256 / (C / elem_vec(dtype));
    unsigned gg = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(pixels, gen_ppt() * ppb), 2048));      // >= two pixels per thread (one iteration of the two-pixel loop)
    act_dispatch(act, [&](auto ac) {
      constexpr int A = decltype(ac)::value;
      with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
        with_bool(res != nullptr, [&](auto r) {
          hipLaunchKernelGGL((affine_act_gen_kernel<T, A, decltype(r)::value>), dim3(gg), dim3(256), 0, st, (const T*)y, scale, shift, (const T*)res, (T*)out, pixels, C, act, slope); }); });
    });
    return;
  }
  bool v4 = (C % 4 == 0);
  unsigned g = ew_grid(v4 ? total / 4 : total);
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
    with_bool(v4, [&](auto v) {
      hipLaunchKernelGGL((affine_act_kernel<T, decltype(v)::value>), dim3(g), dim3(256), 0, st, (const T*)y, scale, shift, (const T*)res, (T*)out, total, C, act, slope); }); });
}

bool affine_act_add_ok(int C, int dtype) { return vec_ok(C, dtype); }
// the backward kernels that recompute the activation's argument from y (the vec and gen forms); the scalar fall-back reads z
bool bn_bwd_recomputes(int C, int dtype) { return vec_ok(C, dtype) || gen_ok(C, dtype); }
void launch_affine_act_add(const void* y, const float* scale, const float* shift, int act1, float slope1, const void* res, void* out,
                           int64_t pixels, int C, int act2, float slope2, int dtype, hipStream_t st) {
  const int64_t nvec = pixels * C / elem_vec(dtype);
  const unsigned gv = ew_grid(nvec);
  act_dispatch(act1 == act2 ? act1 : -1, [&](auto ac) {      // (residual blocks use one activation for both)
    constexpr int A = decltype(ac)::value;
    with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
      hipLaunchKernelGGL((affine_act_add_vec_kernel<T, A, A>), dim3(gv), dim3(256), 0, st, (const T*)y, scale, shift, (const T*)res, (T*)out, nvec, C, act1, slope1, act2, slope2); });
  });
}

// instantiation names as rocprofv3's kernel trace prints them (bench.py attributes HIP-event timings to kernels by these names):
// which 0 = rd_affine_act (flag: residual present), 1 = BatchNorm-backward reduce, 2 = BatchNorm-backward apply (flag: recompute form),
// 3 = the frozen (running-statistics) backward
const char* bn_kernel_name(int which, int C, int dtype, int act, int flag) {
  static thread_local char buf[96];
  const char* T = elem_name(dtype);
  const bool v = vec_ok(C, dtype), g = !v && gen_ok(C, dtype);
  const char* form = v ? "vec" : "gen";
  const int A = (act >= 0 && act <= 3) ? act : -1;
  if (which == 3) {      // the frozen backward: flag bit 0 = the sums are wanted, bit 1 = the derivative is read from z (dres given)
    const char* S = (flag & 1) ? "true" : "false"; const char* Z = (flag & 2) ? "true" : "false";
    if (v || g) snprintf(buf, sizeof(buf), "bn_frozen_bwd_%s_kernel<%s, %s, %s, %d>", form, T, S, Z, A);
    else snprintf(buf, sizeof(buf), "bn_frozen_bwd_kernel<%s, %s, %s>", T, S, Z);
    return buf;
  }
  if (!(v || g)) flag = which == 0 ? flag : 0;
  if (which == 0) {
    if (v || g) snprintf(buf, sizeof(buf), "affine_act_%s_kernel<%s, %d, %s>", form, T, A, flag ? "true" : "false");
    else snprintf(buf, sizeof(buf), "affine_act_kernel<%s, %s>", T, (C % 4 == 0) ? "true" : "false");
  } else if (which == 1) {
    if (v || g) { if (flag) snprintf(buf, sizeof(buf), "col_reduce_%s_kernel<%s, 0, true, %d>", form, T, A); else snprintf(buf, sizeof(buf), "col_reduce_%s_kernel<%s, 0, false, -1>", form, T); }
    else snprintf(buf, sizeof(buf), "col_reduce_kernel<%s, 0>", T);
  } else {
    if (v || g) { if (flag) snprintf(buf, sizeof(buf), "bn_bwd_apply_%s_kernel<%s, true, %d>", form, T, A); else snprintf(buf, sizeof(buf), "bn_bwd_apply_%s_kernel<%s, false, -1>", form, T); }
    else snprintf(buf, sizeof(buf), "bn_bwd_apply_kernel<%s, %s>", T, (C % 4 == 0) ? "true" : "false");
  }
  return buf;
}
int bn_bwd_rows(int64_t pixels, int C) { return red_rows(pixels, C); }
int colsum_rows(int64_t rows, int C) { return red_rows(rows, C); }

void launch_bn_bwd_reduce(const void* dz, const void* z, const void* y, const float* mean, const float* rstd,
                          float* partial, int64_t pixels, int C, int act, float slope, int dtype, hipStream_t st,
                          const float* scale, const float* shift) {
  if (!(vec_ok(C, dtype) || gen_ok(C, dtype))) shift = nullptr;   // the scalar fall-back reads z
  RedGeom g = red_geom(C);
  dim3 grid(red_rows(pixels, C), g.nchunk);
  if (vec_ok(C, dtype)) {
    act_dispatch(act, [&](auto ac) {
      constexpr int A = decltype(ac)::value; (void)A;
      with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;      // without shift the activation's argument is not recomputed: one <T, 0, false, -1> form, whatever A
        if (shift) hipLaunchKernelGGL((col_reduce_vec_kernel<T, 0, true, A>), dim3(grid.x), dim3(256), 0, st, (const T*)dz, (const T*)z, (const T*)y, mean, rstd, partial, pixels, C, act, slope, scale, shift);
        else hipLaunchKernelGGL((col_reduce_vec_kernel<T, 0, false, -1>), dim3(grid.x), dim3(256), 0, st, (const T*)dz, (const T*)z, (const T*)y, mean, rstd, partial, pixels, C, act, slope, scale, shift);
      });
    });
    return;
  }
  if (gen_ok(C, dtype)) {
    act_dispatch(act, [&](auto ac) {
      constexpr int A = decltype(ac)::value; (void)A;
      with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;      // without shift the activation's argument is not recomputed: one <T, 0, false, -1> form, whatever A
        if (shift) hipLaunchKernelGGL((col_reduce_gen_kernel<T, 0, true, A>), dim3(grid.x), dim3(256), 0, st, (const T*)dz, (const T*)z, (const T*)y, mean, rstd, partial, pixels, C, act, slope, scale, shift);
        else hipLaunchKernelGGL((col_reduce_gen_kernel<T, 0, false, -1>), dim3(grid.x), dim3(256), 0, st, (const T*)dz, (const T*)z, (const T*)y, mean, rstd, partial, pixels, C, act, slope, scale, shift);
      });
    });
    return;
  }
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
    hipLaunchKernelGGL((col_reduce_kernel<T, 0>), grid, dim3(256), 0, st, (const T*)dz, (const T*)z, (const T*)y, mean, rstd, partial, pixels, C, g.CB, g.PL, act, slope); });
}

void launch_bn_bwd_finalize(const float* partial, int rows, int C, double count, float* dgamma, float* dbeta,
                            int accumulate, float* c1, float* c2, hipStream_t st, int row_pitch) {
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)C), dim3(256), 0, st, partial, rows, C, count, dgamma, dbeta, accumulate, c1, c2,
                     row_pitch > 0 ? row_pitch : C);
}

void launch_bn_bwd_apply(const void* dz, const void* z, const void* y, const float* mean, const float* rstd,
                         const float* scale, const float* c1, const float* c2, void* dy, void* dres, int64_t pixels, int C,
                         int act, float slope, int dtype, hipStream_t st, const float* shift) {
  if (!(vec_ok(C, dtype) || gen_ok(C, dtype))) shift = nullptr;
  int64_t total = pixels * C;
  if (vec_ok(C, dtype)) {
    const int64_t nvec = total / elem_vec(dtype);
    unsigned gv = ew_grid_per(nvec, 2);
    act_dispatch(act, [&](auto ac) {
      constexpr int A = decltype(ac)::value; (void)A;
      with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;      // as in launch_bn_bwd_reduce: one <T, false, -1> form without shift
        if (shift) hipLaunchKernelGGL((bn_bwd_apply_vec_kernel<T, true, A>), dim3(gv), dim3(256), 0, st, (const T*)dz, (const T*)z, (const T*)y, mean, rstd, scale, c1, c2, shift, (T*)dy, (T*)dres, nvec, C, act, slope);
        else hipLaunchKernelGGL((bn_bwd_apply_vec_kernel<T, false, -1>), dim3(gv), dim3(256), 0, st, (const T*)dz, (const T*)z, (const T*)y, mean, rstd, scale, c1, c2, shift, (T*)dy, (T*)dres, nvec, C, act, slope);
      });
    });
    return;
  }
  if (gen_ok(C, dtype)) {
    const int ppb = 256 / (C / elem_vec(dtype));
    unsigned gg = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(pixels, 2 * ppb), 2048));      // two pixels per thread per iteration (4 / 8: 1244 / 1241 vs 1246 img/s on the SML step)
    act_dispatch(act, [&](auto ac) {
      constexpr int A = decltype(ac)::value; (void)A;
      with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;      // as in launch_bn_bwd_reduce: one <T, false, -1> form without shift
        if (shift) hipLaunchKernelGGL((bn_bwd_apply_gen_kernel<T, true, A>), dim3(gg), dim3(256), 0, st, (const T*)dz, (const T*)z, (const T*)y, mean, rstd, scale, c1, c2, shift, (T*)dy, (T*)dres, pixels, C, act, slope);
        else hipLaunchKernelGGL((bn_bwd_apply_gen_kernel<T, false, -1>), dim3(gg), dim3(256), 0, st, (const T*)dz, (const T*)z, (const T*)y, mean, rstd, scale, c1, c2, shift, (T*)dy, (T*)dres, pixels, C, act, slope);
      });
    });
    return;
  }
  bool v4 = (C % 4 == 0);
  unsigned g = ew_grid(v4 ? total / 4 : total);
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
    with_bool(v4, [&](auto v) {
      hipLaunchKernelGGL((bn_bwd_apply_kernel<T, decltype(v)::value>), dim3(g), dim3(256), 0, st, (const T*)dz, (const T*)z, (const T*)y, mean, rstd, scale, c1, c2, (T*)dy, (T*)dres, total, C, act, slope); }); });
}

// ---- backward through a BatchNorm that normalises with its running statistics (frozen / eval mode).  mean and rstd are constants of the
// layer, so dy = scale * g needs neither batch sum: ONE pass reads dz and y and writes dy (three tensor passes; the training-mode backward
// makes five), and where gamma / beta want gradients the same pass leaves the (sum g, sum g * xhat) rows that bn_bwd_finalize_kernel sums.
// g = dz * act'(u).  FROMZ (the layer had a residual, dres is written): u is read from z, as bn_bwd_apply_kernel does; otherwise u is
// recomputed from y with rd_affine_act's own expression scale * y + shift, in all three channel-count forms -- z is never needed.
// SUMS: block b owns the pixels [b * per, (b + 1) * per) (col_reduce's geometry and summation order); otherwise a plain grid-stride loop.
template <typename T, bool SUMS, bool FROMZ, int ACT>
__global__ __launch_bounds__(256) void bn_frozen_bwd_vec_kernel(const T* __restrict__ dz, const T* __restrict__ z, const T* __restrict__ y,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                const float* __restrict__ scale, const float* __restrict__ shift,
                                                                float* __restrict__ partial, T* __restrict__ dy, T* __restrict__ dres,
                                                                int64_t pixels, int C, int act, float slope) {
  constexpr int VE = Elem<T>::VE;
  const int actv = ACT >= 0 ? ACT : act;
  __shared__ float red[SUMS ? 256 * VE * 2 : 2];
  const int t = threadIdx.x;
  const int VP = C / VE;
  int64_t i, vend, step;
  if (SUMS) {
    const int64_t per = cdiv(pixels, (int64_t)gridDim.x);
    const int64_t pbeg = (int64_t)blockIdx.x * per, pend = pbeg + per < pixels ? pbeg + per : pixels;
    i = pbeg * VP + t; vend = pend * VP; step = 256;
  } else {
    i = (int64_t)blockIdx.x * 256 + t; vend = pixels * VP; step = (int64_t)gridDim.x * 256;
  }
  const int c0 = (t % VP) * VE;      // 256 % VP == 0: a thread keeps its channel vector for the whole loop
  float mu[VE], rs[VE], sc[VE], sh[VE], a[VE], b[VE];
#pragma unroll
  for (int e = 0; e < VE; e++) {
    a[e] = 0.f; b[e] = 0.f;
    mu[e] = SUMS ? mean[c0 + e] : 0.f; rs[e] = SUMS ? rstd[c0 + e] : 1.f;
    sc[e] = scale[c0 + e]; sh[e] = FROMZ ? 0.f : shift[c0 + e];
  }
  auto one = [&](int64_t o, float (&gg)[VE], const float (&zz)[VE], const float (&yy)[VE]) RD_INLINE_LAMBDA {
    float ov[VE];
#pragma unroll
    for (int e = 0; e < VE; e++) {
      if (actv) gg[e] *= act_grad_from_out(FROMZ ? zz[e] : yy[e] * sc[e] + sh[e], actv, slope);
      ov[e] = sc[e] * gg[e];
      if (SUMS) { a[e] += gg[e]; b[e] += gg[e] * ((yy[e] - mu[e]) * rs[e]); }
    }
    stv(dy + o, ov);
    if (FROMZ) stv(dres + o, gg);
  };
  for (; i + step < vend; i += 2 * step) {      // two vectors per iteration, every request issued before the first use
    float g0[VE], z0[VE], y0[VE], g1[VE], z1[VE], y1[VE];
    ldv(dz + i * VE, g0); ldv(dz + (i + step) * VE, g1);
    if (FROMZ && actv) { ldv(z + i * VE, z0); ldv(z + (i + step) * VE, z1); }
    ldv(y + i * VE, y0); ldv(y + (i + step) * VE, y1);
    one(i * VE, g0, z0, y0); one((i + step) * VE, g1, z1, y1);
  }
  for (; i < vend; i += step) {
    float g0[VE], z0[VE], y0[VE];
    ldv(dz + i * VE, g0);
    if (FROMZ && actv) ldv(z + i * VE, z0);
    ldv(y + i * VE, y0);
    one(i * VE, g0, z0, y0);
  }
  if (SUMS) {      // col_reduce_vec_kernel's combine: lanes of a wave that share a channel group, fixed xor tree, then the waves in order
    for (int o = 32; o >= VP; o >>= 1) {
#pragma unroll
      for (int e = 0; e < VE; e++) { a[e] += __shfl_xor(a[e], o); b[e] += __shfl_xor(b[e], o); }
    }
#pragma unroll
    for (int e = 0; e < VE; e++) { red[(t * VE + e) * 2] = a[e]; red[(t * VE + e) * 2 + 1] = b[e]; }
    __syncthreads();
    for (int c = t; c < C; c += 256) {
      const int g = c / VE, e = c - g * VE;
      float sa = 0.f, sb = 0.f;
      for (int tt = g; tt < 256; tt += VP)
        if ((tt & 63) < VP) { sa += red[(tt * VE + e) * 2]; sb += red[(tt * VE + e) * 2 + 1]; }
      partial[((int64_t)blockIdx.x * C + c) * 2] = sa;
      partial[((int64_t)blockIdx.x * C + c) * 2 + 1] = sb;
    }
  }
}

// any channel count with whole vectors, at most 256 of them: thread t owns channel group t % VP of pixel slot t / VP (affine_act_gen_kernel)
template <typename T, bool SUMS, bool FROMZ, int ACT>
__global__ __launch_bounds__(256) void bn_frozen_bwd_gen_kernel(const T* __restrict__ dz, const T* __restrict__ z, const T* __restrict__ y,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                const float* __restrict__ scale, const float* __restrict__ shift,
                                                                float* __restrict__ partial, T* __restrict__ dy, T* __restrict__ dres,
                                                                int64_t pixels, int C, int act, float slope) {
  constexpr int VE = Elem<T>::VE;
  const int actv = ACT >= 0 ? ACT : act;
  __shared__ float red[SUMS ? 256 * VE * 2 : 2];
  const int t = threadIdx.x;
  const int VP = C / VE, PPB = 256 / VP;
  const int g = t % VP, pl = t / VP;
  int64_t p, pend, step;
  if (SUMS) {
    const int64_t per = cdiv(pixels, (int64_t)gridDim.x);
    const int64_t pbeg = (int64_t)blockIdx.x * per;
    pend = pbeg + per < pixels ? pbeg + per : pixels;
    p = pbeg + pl; step = PPB;
  } else {
    p = (int64_t)blockIdx.x * PPB + pl; pend = pixels; step = (int64_t)gridDim.x * PPB;
  }
  float mu[VE], rs[VE], sc[VE], sh[VE], a[VE], b[VE];
#pragma unroll
  for (int e = 0; e < VE; e++) {
    const int c = g * VE + e;
    a[e] = 0.f; b[e] = 0.f;
    mu[e] = SUMS ? mean[c] : 0.f; rs[e] = SUMS ? rstd[c] : 1.f;
    sc[e] = scale[c]; sh[e] = FROMZ ? 0.f : shift[c];
  }
  auto one = [&](int64_t o, float (&gg)[VE], const float (&zz)[VE], const float (&yy)[VE]) RD_INLINE_LAMBDA {
    float ov[VE];
#pragma unroll
    for (int e = 0; e < VE; e++) {
      if (actv) gg[e] *= act_grad_from_out(FROMZ ? zz[e] : yy[e] * sc[e] + sh[e], actv, slope);
      ov[e] = sc[e] * gg[e];
      if (SUMS) { a[e] += gg[e]; b[e] += gg[e] * ((yy[e] - mu[e]) * rs[e]); }
    }
    stv(dy + o, ov);
    if (FROMZ) stv(dres + o, gg);
  };
  if (pl < PPB) {
    for (; p + step < pend; p += 2 * step) {      // two pixels per iteration (small maps are latency-bound otherwise)
      const int64_t o0 = p * C + g * VE, o1 = (p + step) * C + g * VE;
      float g0[VE], z0[VE], y0[VE], g1[VE], z1[VE], y1[VE];
      ldv(dz + o0, g0); ldv(dz + o1, g1);
      if (FROMZ && actv) { ldv(z + o0, z0); ldv(z + o1, z1); }
      ldv(y + o0, y0); ldv(y + o1, y1);
      one(o0, g0, z0, y0); one(o1, g1, z1, y1);
    }
    for (; p < pend; p += step) {
      const int64_t o0 = p * C + g * VE;
      float g0[VE], z0[VE], y0[VE];
      ldv(dz + o0, g0);
      if (FROMZ && actv) ldv(z + o0, z0);
      ldv(y + o0, y0);
      one(o0, g0, z0, y0);
    }
  }
  if (SUMS) {      // col_reduce_gen_kernel's combine: the pixel slots of a channel in slot order
#pragma unroll
    for (int e = 0; e < VE; e++) { red[(t * VE + e) * 2] = a[e]; red[(t * VE + e) * 2 + 1] = b[e]; }
    __syncthreads();
    for (int c = t; c < C; c += 256) {
      const int gg = c / VE, e = c - gg * VE;
      float sa = 0.f, sb = 0.f;
      for (int q = 0; q < PPB; q++) { sa += red[((q * VP + gg) * VE + e) * 2]; sb += red[((q * VP + gg) * VE + e) * 2 + 1]; }
      partial[((int64_t)blockIdx.x * C + c) * 2] = sa;
      partial[((int64_t)blockIdx.x * C + c) * 2 + 1] = sb;
    }
  }
}

// every other channel count: col_reduce_kernel's geometry (thread = pixel lane x channel, grid = pixel ranges x channel chunks), with and
// without the sums; four pixels' loads in flight per iteration, accumulated in pixel order
template <typename T, bool SUMS, bool FROMZ>
__global__ __launch_bounds__(256) void bn_frozen_bwd_kernel(const T* __restrict__ dz, const T* __restrict__ z, const T* __restrict__ y,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            float* __restrict__ partial, T* __restrict__ dy, T* __restrict__ dres,
                                                            int64_t pixels, int C, int CB, int PL, int act, float slope) {
  __shared__ float red[SUMS ? 2 : 1][SUMS ? 256 : 1];
  const int t = threadIdx.x;
  const int cl = t % CB, pl = t / CB;
  const int c = blockIdx.y * CB + cl;
  const int64_t per = cdiv(pixels, (int64_t)gridDim.x);
  const int64_t pbeg = (int64_t)blockIdx.x * per, pend = pbeg + per < pixels ? pbeg + per : pixels;
  float a = 0.f, b = 0.f;
  if (c < C) {
    const float mu = SUMS ? mean[c] : 0.f, rs = SUMS ? rstd[c] : 1.f, sc = scale[c], sh = FROMZ ? 0.f : shift[c];
    int64_t p = pbeg + pl;
    for (; p + 3 * (int64_t)PL < pend; p += 4 * (int64_t)PL) {
      float g[4], zz[4] = {0.f, 0.f, 0.f, 0.f}, yy[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int64_t i = (p + q * (int64_t)PL) * C + c;
        g[q] = Elem<T>::ld(dz + i);
        if (FROMZ && act) zz[q] = Elem<T>::ld(z + i);
        yy[q] = Elem<T>::ld(y + i);
      }
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int64_t i = (p + q * (int64_t)PL) * C + c;
        float gq = g[q];
        if (act) gq *= act_grad_from_out(FROMZ ? zz[q] : yy[q] * sc + sh, act, slope);
        Elem<T>::st(dy + i, sc * gq);
        if (FROMZ) Elem<T>::st(dres + i, gq);
        if (SUMS) { a += gq; b += gq * ((yy[q] - mu) * rs); }
      }
    }
    for (; p < pend; p += PL) {
      const int64_t i = p * C + c;
      float gq = Elem<T>::ld(dz + i);
      const float yv = Elem<T>::ld(y + i);
      if (act) gq *= act_grad_from_out(FROMZ ? Elem<T>::ld(z + i) : yv * sc + sh, act, slope);
      Elem<T>::st(dy + i, sc * gq);
      if (FROMZ) Elem<T>::st(dres + i, gq);
      if (SUMS) { a += gq; b += gq * ((yv - mu) * rs); }
    }
  }
  if (SUMS) {
    red[0][t] = a; red[1][t] = b;
    __syncthreads();
    if (pl == 0 && c < C) {
      float sa = 0.f, sb = 0.f;
      for (int q = 0; q < PL; q++) { sa += red[0][q * CB + cl]; sb += red[1][q * CB + cl]; }
      partial[((int64_t)blockIdx.x * C + c) * 2] = sa;
      partial[((int64_t)blockIdx.x * C + c) * 2 + 1] = sb;
    }
  }
}

// partial != nullptr: the pass also writes bn_bwd_rows(pixels, C) rows of (sum g, sum g * xhat); dres != nullptr: the derivative is read from z
void launch_bn_frozen_bwd(const void* dz, const void* z, const void* y, const float* mean, const float* rstd, const float* scale,
                          const float* shift, float* partial, void* dy, void* dres, int64_t pixels, int C, int act, float slope, int dtype,
                          hipStream_t st) {
  const bool sums = partial != nullptr, fromz = dres != nullptr;
  const int ve = elem_vec(dtype);
  const int rows = red_rows(pixels, C);
  // both macros are used inside with_elem: T is the element type there
#define RD_FZ(K, S, Z, GRID, ...) hipLaunchKernelGGL((K<T, S, Z, ##__VA_ARGS__>), GRID, dim3(256), 0, st, (const T*)dz, (const T*)z, (const T*)y, mean, rstd, scale, shift, partial, (T*)dy, (T*)dres, pixels, C, RD_FZ_TAIL)
#define RD_FZ4(K, GRID, ...) do { if (sums) { if (fromz) RD_FZ(K, true, true, GRID, ##__VA_ARGS__); else RD_FZ(K, true, false, GRID, ##__VA_ARGS__); } \
                                  else { if (fromz) RD_FZ(K, false, true, GRID, ##__VA_ARGS__); else RD_FZ(K, false, false, GRID, ##__VA_ARGS__); } } while (0)
  if (vec_ok(C, dtype) || gen_ok(C, dtype)) {
    const bool v = vec_ok(C, dtype);
    const int ppb = 256 / (C / ve);
    // no sums: two vectors / two pixels per thread and iteration, as the training-mode apply kernels' grids
    const unsigned gx = sums ? (unsigned)rows : v ? ew_grid_per(pixels * (C / ve), 2) : (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(pixels, 2 * ppb), 2048));
    const dim3 grid(gx);
#define RD_FZ_TAIL act, slope
    act_dispatch(act, [&](auto ac) {
      constexpr int A = decltype(ac)::value;
      if (v) with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type; RD_FZ4(bn_frozen_bwd_vec_kernel, grid, A); });
      else with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type; RD_FZ4(bn_frozen_bwd_gen_kernel, grid, A); });
    });
#undef RD_FZ_TAIL
    return;
  }
  RedGeom g = red_geom(C);
  const dim3 grid(rows, g.nchunk);
#define RD_FZ_TAIL g.CB, g.PL, act, slope
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type; RD_FZ4(bn_frozen_bwd_kernel, grid); });
#undef RD_FZ_TAIL
#undef RD_FZ4
#undef RD_FZ
}

void launch_act_bwd(const void* dz, const void* z, void* dx, int64_t n, int act, float slope, int dtype, hipStream_t st) {
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
    hipLaunchKernelGGL((act_bwd_kernel<T>), dim3(ew_grid(n)), dim3(256), 0, st, (const T*)dz, (const T*)z, (T*)dx, n, act, slope); });
}

// LayerNorm parameter gradients of MANY layer applications in one launch.  An item is one (gamma, beta) pair with the partial buffers of
// all its applications since the last flush; they are added in order, each summed over its rows exactly as bn_bwd_finalize_kernel does
// (RC-Net: 12 fused LoFTR backward launches per step, two finalize launches of 5 us behind each).
struct LnGradBatch { LnGradItem it[LN_GRAD_BATCH_MAX]; };
__global__ __launch_bounds__(256) void ln_grad_batch_kernel(LnGradBatch b) {
  __shared__ double s1[4], s2[4];
  const LnGradItem& it = b.it[blockIdx.y];
  const int c = blockIdx.x, t = threadIdx.x;
  if (c >= it.C) return;
  float ga = 0.f, be = 0.f;
  if (it.accumulate) { ga = it.dgamma[c]; be = it.dbeta[c]; }
  for (int p = 0; p < it.nparts; p++) {
    double a = 0.0, g = 0.0;
    bn_rows_sum(reinterpret_cast<const float2*>(it.partial[p]), it.rows[p], it.C, c, t, a, g);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); g += __shfl_xor(g, o); }
    __syncthreads();
    if ((t & 63) == 0) { s1[t >> 6] = a; s2[t >> 6] = g; }
    __syncthreads();
    a = (s1[0] + s1[1]) + (s1[2] + s1[3]); g = (s2[0] + s2[1]) + (s2[2] + s2[3]);
    const bool first = p == 0 && !it.accumulate;
    be = first ? (float)a : be + (float)a;
    ga = first ? (float)g : ga + (float)g;
  }
  if (t == 0) { it.dbeta[c] = be; it.dgamma[c] = ga; }
}
void launch_ln_grad_batch(const LnGradItem* items, int n, hipStream_t st) {
  for (int base = 0; base < n; base += LN_GRAD_BATCH_MAX) {
    const int m = std::min(LN_GRAD_BATCH_MAX, n - base);
    LnGradBatch b;
    int maxc = 1;
    for (int i = 0; i < m; i++) { b.it[i] = items[base + i]; maxc = std::max(maxc, b.it[i].C); }
    for (int i = m; i < LN_GRAD_BATCH_MAX; i++) b.it[i] = b.it[0];
    hipLaunchKernelGGL(ln_grad_batch_kernel, dim3((unsigned)maxc, (unsigned)m), dim3(256), 0, st, b);
  }
}
// many bias gradients finished by ONE launch: item i sums its partial rows exactly as colsum_finalize_kernel does (lanes stride the rows,
// double precision, xor tree).  SML's decoder has 22 biased convolutions per step: 22 finalize launches of 6 us each for a few KB of sums.
struct ColsumBatch { ColsumItem it[COLSUM_BATCH_MAX]; };
__global__ __launch_bounds__(64) void colsum_finalize_batch_kernel(ColsumBatch b) {
  const ColsumItem it = b.it[blockIdx.y];
  const int lane = threadIdx.x;
  for (int c = blockIdx.x; c < it.C; c += gridDim.x) {
    double a = 0.0;
    // eight rows' loads in flight per iteration (unconditional: a row past the end reads row 0 and adds zero), added in row order as the
    // one-row loop did: that loop was one dependent round trip per 64 rows -- 48 us for the SML step's 21 bias gradients
    for (int r = lane; r < it.rows; r += 512) {
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; q++) { const int rq = r + 64 * q; const float x = it.partial[((int64_t)(rq < it.rows ? rq : 0) * it.C + c) * 2]; v[q] = rq < it.rows ? x : 0.f; }
#pragma unroll
      for (int q = 0; q < 8; q++) a += v[q];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if (lane == 0) it.out[c] = it.accumulate ? it.out[c] + (float)a : (float)a;
  }
}
void launch_colsum_finalize_batch(const ColsumItem* items, int n, hipStream_t st) {
  for (int base = 0; base < n; base += COLSUM_BATCH_MAX) {
    const int m = std::min(COLSUM_BATCH_MAX, n - base);
    ColsumBatch b;
    int maxc = 1;
    for (int i = 0; i < m; i++) { b.it[i] = items[base + i]; maxc = std::max(maxc, b.it[i].C); }
    for (int i = m; i < COLSUM_BATCH_MAX; i++) b.it[i] = b.it[0];
    hipLaunchKernelGGL(colsum_finalize_batch_kernel, dim3((unsigned)std::min(maxc, 512), (unsigned)m), dim3(64), 0, st, b);
  }
}
void launch_colsum(const void* x, float* partial, float* out, int accumulate, int64_t rows, int C, int dtype, hipStream_t st) {
  RedGeom g = red_geom(C);
  int nr = red_rows(rows, C);
  dim3 grid(nr, g.nchunk);
  if (vec_ok(C, dtype)) {
    with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
      hipLaunchKernelGGL((col_reduce_vec_kernel<T, 1, false, -1>), dim3(nr), dim3(256), 0, st, (const T*)x, (const T*)nullptr, (const T*)nullptr, (const float*)nullptr, (const float*)nullptr, partial, rows, C, 0, 0.f, (const float*)nullptr, (const float*)nullptr); });
  } else if (gen_ok(C, dtype)) {
    with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
      hipLaunchKernelGGL((col_reduce_gen_kernel<T, 1, false, -1>), dim3(nr), dim3(256), 0, st, (const T*)x, (const T*)nullptr, (const T*)nullptr, (const float*)nullptr, (const float*)nullptr, partial, rows, C, 0, 0.f, (const float*)nullptr, (const float*)nullptr); });
  } else {
    with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
      hipLaunchKernelGGL((col_reduce_kernel<T, 1>), grid, dim3(256), 0, st, (const T*)x, (const T*)nullptr, (const T*)nullptr, (const float*)nullptr, (const float*)nullptr, partial, rows, C, g.CB, g.PL, 0, 0.f); });
  }
  if (out) hipLaunchKernelGGL(colsum_finalize_kernel, dim3((unsigned)C), dim3(64), 0, st, partial, nr, C, out, accumulate);      // out == nullptr: partial rows only
}

void launch_layernorm_fwd(const void* x, const float* gamma, const float* beta, const void* res, void* out, float* mean,
                          float* rstd, int64_t rows, int C, float eps, int dtype, hipStream_t st) {
  unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(rows, 4), 2048));
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
    hipLaunchKernelGGL((layernorm_fwd_kernel<T>), dim3(g), dim3(256), 0, st, (const T*)x, gamma, beta, (const T*)res, (T*)out, mean, rstd, rows, C, eps); });
}

int layernorm_bwd_rows(int64_t rows) { return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(rows, 16), 512)); }

void launch_layernorm_bwd(const void* dout, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx,
                          float* partial, float* dgamma, float* dbeta, int accumulate, int64_t rows, int C, int dtype,
                          hipStream_t st) {
  int nb = layernorm_bwd_rows(rows);
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
    hipLaunchKernelGGL((layernorm_bwd_kernel<T>), dim3(nb), dim3(256), 0, st, (const T*)dout, (const T*)x, gamma, mean, rstd, (T*)dx, partial, rows, C); });
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)C), dim3(256), 0, st, partial, nb, C, 1.0, dgamma, dbeta, accumulate, (float*)nullptr, (float*)nullptr, C);
}

}  // namespace rd
