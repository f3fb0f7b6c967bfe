// RC-Net label build, masked weighted BCE, sigmoid and the inference crop scatter.
//
// Reference:
//   RCNet/rcnet_main.py:308-332  label = (|gt - z| < thr) & (gt > 0); validity = gt > 0
//   RCNet/rcnet_model.py:152-160 binary_cross_entropy_with_logits(pos_weight) * validity, sum / sum(validity)
//   RCNet/rcnet_main.py:460-485  forward_output: threshold, paste each crop at integer offsets, confidence-
//                                weighted mean depth, 0 where no crop responds (gather-by-pixel here, so the
//                                non-zero index set is exact and no N full-size canvases are allocated)
#include "rd_common.h"
#include "rd_kernels.h"

namespace rd {

static unsigned ew_grid(int64_t n, int cap = 2048) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, 256), cap)); }

__global__ __launch_bounds__(256) void rcnet_labels_kernel(const float* __restrict__ gt, const float* __restrict__ points,
                                                           float* __restrict__ label, float* __restrict__ valid, int R, int HW,
                                                           float thr, int all_valid) {
  const int64_t total = (int64_t)R * HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int r = (int)(i / HW);
    float z = points[(int64_t)r * 3 + 2];
    float g = gt[i];
    float lab = (fabsf(g - z) < thr) ? 1.f : 0.f;
    label[i] = (g > 0.f) ? lab : 0.f;
    valid[i] = all_valid ? 1.f : ((g <= 0.f) ? 0.f : 1.f);
  }
}

__device__ __forceinline__ float bce_logits(float x, float y, float pw) {
  // (1-y)*x + (1+(pw-1)*y) * (log1p(exp(-|x|)) + max(-x,0))
  float sp = log1pf(__expf(-fabsf(x))) + fmaxf(-x, 0.f);
  return (1.f - y) * x + (1.f + (pw - 1.f) * y) * sp;
}

template <typename T>
__global__ __launch_bounds__(256) void bce_fwd_kernel(const T* __restrict__ logits, const float* __restrict__ label,
                                                      const float* __restrict__ valid, float pw, float* __restrict__ partial,
                                                      int64_t n) {
  __shared__ float red[2][4];
  float a = 0.f, b = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float vm = valid[i];
    a += vm * bce_logits(Elem<T>::ld(logits + i), label[i], pw);
    b += vm;
  }
  a = wave_sum(a); b = wave_sum(b);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { red[0][wv] = a; red[1][wv] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[blockIdx.x * 2] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    partial[blockIdx.x * 2 + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

// one wave: lanes stride over the partial rows, double-precision xor tree (fixed order -> deterministic)
__global__ void bce_finalize_kernel(const float* __restrict__ partial, int rows, float* loss, float* sums) {
  const int lane = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int r = lane; r < rows; r += 64) { a += partial[r * 2]; b += partial[r * 2 + 1]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
  if (lane == 0) {
    sums[0] = (float)a; sums[1] = (float)b;
    loss[0] = (float)(a / b);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void bce_bwd_kernel(const T* __restrict__ logits, const float* __restrict__ label,
                                                      const float* __restrict__ valid, float pw, const float* __restrict__ sums,
                                                      const float* __restrict__ dloss, T* __restrict__ dlogits, int64_t n) {
  const float gs = dloss[0] / sums[1];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float x = Elem<T>::ld(logits + i), y = label[i];
    float sg = 1.f / (1.f + __expf(-x));
    float d = (1.f - y) - (1.f + (pw - 1.f) * y) * (1.f - sg);
    Elem<T>::st(dlogits + i, valid[i] * d * gs);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void sigmoid_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    Elem<T>::st(y + i, 1.f / (1.f + __expf(-Elem<T>::ld(x + i))));
}

// crops [Ncrop][PH][PW] (responses), points [Ncrop][3] = (x, y, z) in PADDED image coordinates,
// outputs are the un-padded H x W depth and response maps.
template <typename T>
__global__ __launch_bounds__(256) void scatter_crops_kernel(const T* __restrict__ crops, const float* __restrict__ points,
                                                            float* __restrict__ depth, float* __restrict__ response, int Ncrop,
                                                            int PH, int PW, int H, int W, float thr) {
  const int pad_y = PH / 2, pad_x = PW / 2;
  const int total = H * W;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    int u = i / W, v = i - u * W;
    int pr = u + pad_y, pc = v + pad_x;  // padded coordinates of this pixel
    float wsum = 0.f, zsum = 0.f, wmax = 0.f;
    for (int c = 0; c < Ncrop; c++) {
      int y0 = (int)points[c * 3 + 1] - pad_y, x0 = (int)points[c * 3 + 0] - pad_x;
      int cr = pr - y0, cc = pc - x0;
      if ((unsigned)cr >= (unsigned)(2 * pad_y) || (unsigned)cc >= (unsigned)(2 * pad_x)) continue;
      float w = Elem<T>::ld(crops + ((int64_t)c * PH + cr) * PW + cc);
      if (w < thr) w = 0.f;
      wsum += w; zsum += w * points[c * 3 + 2];
      wmax = fmaxf(wmax, w);
    }
    response[i] = wmax;
    depth[i] = (wmax == 0.f) ? 0.f : zsum / wsum;
  }
}

// ---- inference driver pieces (RCNet/run_rcnet_zju.py:204-271) ------------------------------------------------------------------------
// :221-234: every radar point is moved to padded-image coordinates (+ half patch) and gets the box (x - px, y - py, x + px, y + py);
// rows of `rois` are torchvision's (batch index, x1, y1, x2, y2) (convert_boxes_to_roi_format), so no concatenation is needed later.
__global__ void points_to_rois_kernel(const float* __restrict__ pin, float* __restrict__ pout, float* __restrict__ rois, int N, float pad_x,
                                      float pad_y, float batch_index) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const float x = pin[i * 3] + pad_x, y = pin[i * 3 + 1] + pad_y;
  pout[i * 3] = x; pout[i * 3 + 1] = y; pout[i * 3 + 2] = pin[i * 3 + 2];
  float* r = rois + (int64_t)i * 5;
  r[0] = batch_index; r[1] = x - pad_x; r[2] = y - pad_y; r[3] = x + pad_x; r[4] = y + pad_y;
}
// boxes (B, K, 4) -> rois (B*K, 5), image-major (the order torchvision.ops.roi_pool gives a list of per-image box tensors)
__global__ void boxes_to_rois_kernel(const float* __restrict__ boxes, float* __restrict__ rois, int total, int K, int first_image) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const float* b = boxes + (int64_t)i * 4;
  float* r = rois + (int64_t)i * 5;
  r[0] = (float)(first_image + i / K); r[1] = b[0]; r[2] = b[1]; r[3] = b[2]; r[4] = b[3];
}
// data/data_utils.py:128-143 save_depth: np.uint32(z * multiplier) stored as a 16-bit PNG.  float32 product, truncation toward zero, and
// the clamp to 0..65535 PIL applies when it packs mode 'I' into I;16 (negative -> 0, > 65535 -> 65535).
__global__ void depth_quantize_u16_kernel(const float* __restrict__ z, unsigned short* __restrict__ out, int64_t n, float multiplier) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = z[i] * multiplier;
    out[i] = (unsigned short)(v >= 65536.f ? 65535.f : (v > 0.f ? truncf(v) : 0.f));
  }
}
// :253 `np.sum(output_depth) == 0` (retry with a lower threshold): one block, double accumulation
__global__ __launch_bounds__(256) void sum_f32_kernel(const float* __restrict__ x, int64_t n, double* __restrict__ out) {
  __shared__ double sh[4];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) s += (double)x[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = sh[0] + sh[1] + sh[2] + sh[3];
}
void launch_points_to_rois(const float* pin, float* pout, float* rois, int N, float pad_x, float pad_y, int batch_index, hipStream_t st) {
  if (N > 0) hipLaunchKernelGGL(points_to_rois_kernel, dim3((N + 255) / 256), dim3(256), 0, st, pin, pout, rois, N, pad_x, pad_y, (float)batch_index);
}
void launch_boxes_to_rois(const float* boxes, float* rois, int B, int K, int first_image, hipStream_t st) {
  const int total = B * K;
  if (total > 0) hipLaunchKernelGGL(boxes_to_rois_kernel, dim3((total + 255) / 256), dim3(256), 0, st, boxes, rois, total, K, first_image);
}
void launch_depth_quantize_u16(const float* z, unsigned short* out, int64_t n, float multiplier, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(depth_quantize_u16_kernel, dim3(ew_grid(n)), dim3(256), 0, st, z, out, n, multiplier);
}
void launch_sum_f32(const float* x, int64_t n, double* out, hipStream_t st) {
  hipLaunchKernelGGL(sum_f32_kernel, dim3(1), dim3(256), 0, st, x, n, out);
}

void launch_rcnet_labels(const float* gt, const float* points, float* label, float* valid, int R, int HW, float thr,
                         int all_valid, hipStream_t st) {
  hipLaunchKernelGGL(rcnet_labels_kernel, dim3(ew_grid((int64_t)R * HW)), dim3(256), 0, st, gt, points, label, valid, R, HW, thr, all_valid);
}
int bce_rows(int64_t n) { return (int)ew_grid(n, 1024); }
void launch_bce_fwd(const void* logits, const float* label, const float* valid, float pw, float* partial, float* loss,
                    float* sums, int64_t n, int dtype, hipStream_t st) {
  int rows = bce_rows(n);
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
    hipLaunchKernelGGL((bce_fwd_kernel<T>), dim3(rows), dim3(256), 0, st, (const T*)logits, label, valid, pw, partial, n); });
  hipLaunchKernelGGL(bce_finalize_kernel, dim3(1), dim3(64), 0, st, partial, rows, loss, sums);
}
void launch_bce_bwd(const void* logits, const float* label, const float* valid, float pw, const float* sums, const float* dloss,
                    void* dlogits, int64_t n, int dtype, hipStream_t st) {
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
    hipLaunchKernelGGL((bce_bwd_kernel<T>), dim3(ew_grid(n)), dim3(256), 0, st, (const T*)logits, label, valid, pw, sums, dloss, (T*)dlogits, n); });
}
void launch_sigmoid(const void* x, void* y, int64_t n, int dtype, hipStream_t st) {
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
    hipLaunchKernelGGL((sigmoid_kernel<T>), dim3(ew_grid(n)), dim3(256), 0, st, (const T*)x, (T*)y, n); });
}
void launch_scatter_crops(const void* crops, const float* points, float* depth, float* response, int Ncrop, int PH, int PW, int H,
                          int W, float thr, int dtype, hipStream_t st) {
  unsigned g = ew_grid((int64_t)H * W);
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
    hipLaunchKernelGGL((scatter_crops_kernel<T>), dim3(g), dim3(256), 0, st, (const T*)crops, points, depth, response, Ncrop, PH, PW, H, W, thr); });
}

}  // namespace rd
