// RC-Net inference over frame batches: the fusion side of RCNet/run_rcnet_zju.py:204-271 for F frames with ragged point counts.
//
// Reference:
//   RCNet/rcnet_main.py:460-485     forward_output: threshold, paste each crop at integer offsets, confidence-weighted mean depth
//   RCNet/run_rcnet_zju.py:250-264  while the fused depth sums to zero, lower the response threshold by 0.05 and fuse again
//
// All index rules are scatter_crops_kernel's (rd_loss.hip): y0 = (int)py - PH/2, x0 = (int)px - PW/2, points in PADDED coordinates, outputs the
// un-padded H x W maps.  Crop c belongs to frame f iff frame_start[f] <= c < frame_start[f + 1].
//
// The retry loop needs no host: the fused map at threshold t is non-zero iff some response w pasted inside the un-padded image has
// w >= (float)t and w > 0 (radar depths are positive), so the loop's answer is the first t_k = t_{k-1} - step (in double, as Python
// computes it) with (float)t_k <= M, M the largest in-image response of the frame.  frame_rmax_kernel finds the per-crop-slice maxima,
// frame_thresholds_kernel reduces them per frame and walks the sequence, scatter_frames_kernel fuses every frame at its own threshold.
#include "rd_common.h"
#include "rd_kernels.h"

namespace rd {

// ---- in-image maximum ------------------------------------------------------------------------------------------------------------------
// grid (R, S): block (c, s) reads slice s of the rows of crop c that land inside the image -- whole rows, 16 bytes per lane where the
// crops pointer allows (a 240 x 100 bf16 crop has rows of 200 bytes: the flat range is cut at 16-byte boundaries instead of per row) -- and
// writes max(w) over the pixels whose column lands inside the image too to partial[c * S + s]; NaN and w <= 0 never win, 0 if nothing does.
// A maximum has no summation order: the result does not depend on S.
template <typename T>
__global__ __launch_bounds__(256) void frame_rmax_kernel(const T* __restrict__ crops, const float* __restrict__ points,
                                                         float* __restrict__ partial, int PH, int PW, int H, int W, int vec_ok) {
  constexpr int VE = Elem<T>::VE;
  __shared__ float red[4];
  const int c = blockIdx.x, s = blockIdx.y, S = gridDim.y, t = threadIdx.x;
  const int pad_y = PH / 2, pad_x = PW / 2;
  const int y0 = (int)points[c * 3 + 1] - pad_y, x0 = (int)points[c * 3 + 0] - pad_x;
  // crop pixel (cr, cc) lands on image pixel (y0 + cr - pad_y, x0 + cc - pad_x)
  const int64_t ra = max((int64_t)pad_y - y0, (int64_t)0), rb = min((int64_t)H + pad_y - y0, (int64_t)PH);
  const int64_t ca = max((int64_t)pad_x - x0, (int64_t)0), cb = min((int64_t)W + pad_x - x0, (int64_t)PW);
  float m = 0.f;
  if (ra < rb && ca < cb) {
    const int64_t nr = rb - ra;
    const int64_t r_lo = ra + nr * s / S, r_hi = ra + nr * (s + 1) / S;
    const int64_t base = (int64_t)c * PH * PW;
    const int64_t g0 = base + r_lo * PW, g1 = base + r_hi * PW;      // flat element range of this block (all rows land inside the image)
    const int64_t v0 = (g0 + VE - 1) / VE, v1 = g1 / VE;             // whole 16-byte vectors inside it
    const int64_t head_end = (vec_ok && v0 < v1) ? v0 * VE : g1;
    for (int64_t i = g0 + t; i < head_end; i += 256) {
      const int cc = (int)((i - base) % PW);
      const float w = Elem<T>::ld(crops + i);
      if (cc >= ca && cc < cb && w > m) m = w;
    }
    if (head_end < g1) {
      for (int64_t v = v0 + t; v < v1; v += 256) {
        const uint4 raw = *reinterpret_cast<const uint4*>(crops + v * VE);
        float w[VE];
        raw16_to_f32(reinterpret_cast<const T*>(0), raw, w);
        int cc = (int)((v * VE - base) % PW);
#pragma unroll
        for (int e = 0; e < VE; e++) {
          if (cc >= ca && cc < cb && w[e] > m) m = w[e];
          cc = (cc + 1 == PW) ? 0 : cc + 1;
        }
      }
      for (int64_t i = v1 * VE + t; i < g1; i += 256) {
        const int cc = (int)((i - base) % PW);
        const float w = Elem<T>::ld(crops + i);
        if (cc >= ca && cc < cb && w > m) m = w;
      }
    }
  }
  m = wave_max(m);
  if ((t & 63) == 0) red[t >> 6] = m;
  __syncthreads();
  if (t == 0) partial[c * S + s] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// ---- threshold per frame: one wave per frame ---------------------------------------------------------------------------------------------
// rmax[f] = max over the frame's partials; the retry loop of run_rcnet_zju.py:250-264 restated on rmax (see the head of this file).  A frame
// without a positive in-image response is where the reference never ends: thr = (float)start, retries = -1, the sticky flag word becomes 1.
__global__ __launch_bounds__(64) void frame_thresholds_kernel(const float* __restrict__ partial, const int* __restrict__ frame_start, int S,
                                                              double start, double step, float* __restrict__ rmax, float* __restrict__ thr,
                                                              int* __restrict__ retries, int* __restrict__ flag) {
  const int f = blockIdx.x, lane = threadIdx.x;
  const int64_t p0 = (int64_t)frame_start[f] * S, p1 = (int64_t)frame_start[f + 1] * S;
  float m = 0.f;
  for (int64_t i = p0 + lane; i < p1; i += 64) m = fmaxf(m, partial[i]);
  m = wave_max(m);
  if (lane != 0) return;
  rmax[f] = m;
  if (m > 0.f) {
    double tcur = start;
    int n = 0;
    while ((float)tcur > m) { tcur -= step; ++n; }      // bounded: the entry point refuses start / step > 4096, and (float)t <= 0 < m ends it
    thr[f] = (float)tcur;
    retries[f] = n;
  } else {
    thr[f] = (float)start;
    retries[f] = -1;
    atomicMax(flag, 1);
  }
}

// ---- scatter over frames -------------------------------------------------------------------------------------------------------------------
// A block owns a SF_TW x SF_TH tile of one frame's pixels (wide: crop reads are contiguous along x) and walks the frame's points in chunks of
// SF_CHUNK: lane i of the block tests point i's patch rectangle against the tile, the survivors are compacted IN ORDER into LDS (ballot, popcount
// of the lower lanes, per-wave bases in ascending wave order), and every thread then walks that list only -- a 240 x 100 patch covers under a
// fifth of a 256 x 512 frame, so the per-pixel loop over all N points of scatter_crops_kernel mostly rejected.  wsum / zsum / wmax carry across
// chunks in registers, so N_f is unlimited and the accumulation order is ascending crop index: bit-identical to scatter_crops_kernel on the
// frame's slice (the arithmetic per covering crop is that kernel's, statement by statement).
constexpr int SF_TW = 64, SF_TH = 4, SF_CHUNK = 256;
static_assert(SF_TW * SF_TH == 256 && SF_CHUNK == 256, "one pixel and one candidate point per thread");

template <typename T>
__global__ __launch_bounds__(256) void scatter_frames_kernel(const T* __restrict__ crops, const float* __restrict__ points,
                                                             const int* __restrict__ frame_start, const float* __restrict__ thr_f,
                                                             float* __restrict__ depth, float* __restrict__ response, int PH, int PW, int H, int W) {
  __shared__ int4 list[SF_CHUNK];      // (x0, y0, z bits, crop index) of the chunk's surviving points, ascending crop index
  __shared__ int wcount[4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int f = blockIdx.z;
  const int pad_y = PH / 2, pad_x = PW / 2;
  const int tu0 = blockIdx.y * SF_TH, tv0 = blockIdx.x * SF_TW;
  const int u = tu0 + (t / SF_TW), v = tv0 + (t % SF_TW);
  const bool live = u < H && v < W;
  const int pr = u + pad_y, pc = v + pad_x;      // padded coordinates of this pixel
  // the tile's rectangle in padded coordinates, clipped to the image
  const int tr0 = tu0 + pad_y, tr1 = min(tu0 + SF_TH, H) + pad_y, tc0 = tv0 + pad_x, tc1 = min(tv0 + SF_TW, W) + pad_x;
  const int p0 = frame_start[f], p1 = frame_start[f + 1];
  const float thr = thr_f[f];
  float wsum = 0.f, zsum = 0.f, wmax = 0.f;

  auto take = [&](const int4& e, float w) RD_INLINE_LAMBDA {      // scatter_crops_kernel's statements for one covering crop
    if (w < thr) w = 0.f;
    wsum += w; zsum += w * __int_as_float(e.z);
    wmax = fmaxf(wmax, w);
  };
  for (int cbase = p0; cbase < p1; cbase += SF_CHUNK) {
    const int c = cbase + t;
    bool hit = false;
    int4 me = make_int4(0, 0, 0, 0);
    if (c < p1) {
      const float px = points[(int64_t)c * 3 + 0], py = points[(int64_t)c * 3 + 1], pz = points[(int64_t)c * 3 + 2];
      me.x = (int)px - pad_x; me.y = (int)py - pad_y; me.z = __float_as_int(pz); me.w = c;
      hit = (int64_t)me.y < tr1 && (int64_t)me.y + PH > tr0 && (int64_t)me.x < tc1 && (int64_t)me.x + PW > tc0;
    }
    const unsigned long long mask = __ballot(hit);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wcount[wv] = __popcll(mask);
    __syncthreads();
    int woff = 0;
    for (int q = 0; q < wv; q++) woff += wcount[q];
    const int total = wcount[0] + wcount[1] + wcount[2] + wcount[3];
    if (hit) list[woff + before] = me;
    __syncthreads();
    // four survivors per step: their loads are requested together (an address outside the patch is clamped to the crop's first element and the
    // value dropped), the accumulation stays in list order
    int li = 0;
    for (; li + 4 <= total; li += 4) {
      int4 e[4]; bool in[4]; float w[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        e[k] = list[li + k];
        const int cr = pr - e[k].y, cc = pc - e[k].x;
        in[k] = live && (unsigned)cr < (unsigned)PH && (unsigned)cc < (unsigned)PW;
        w[k] = Elem<T>::ld(crops + ((int64_t)e[k].w * PH + (in[k] ? cr : 0)) * PW + (in[k] ? cc : 0));
      }
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (in[k]) take(e[k], w[k]);
    }
    for (; li < total; li++) {
      const int4 e = list[li];
      const int cr = pr - e.y, cc = pc - e.x;
      if (live && (unsigned)cr < (unsigned)PH && (unsigned)cc < (unsigned)PW) take(e, Elem<T>::ld(crops + ((int64_t)e.w * PH + cr) * PW + cc));
    }
    // the next chunk's writes to wcount / list come after every wave has passed the second barrier / reached the next first barrier
  }
  if (live) {
    const int64_t o = ((int64_t)f * H + u) * W + v;
    response[o] = wmax;
    depth[o] = (wmax == 0.f) ? 0.f : zsum / wsum;
  }
}

int scatter_frames_chunk() { return SF_CHUNK; }
int frame_rmax_splits(int R) { return R >= 512 ? 1 : (R >= 128 ? 4 : 8); }
int64_t frame_thresholds_ws_bytes(int R) { return (int64_t)std::max(R, 1) * 8 * sizeof(float); }

void launch_frame_thresholds(const void* crops, const float* points, const int* frame_start, int R, int F, int PH, int PW, int H, int W,
                             double start, double step, float* ws, float* rmax, float* thr, int* retries, int* flag, int dtype, hipStream_t st) {
  const int S = frame_rmax_splits(R);
  const int vec_ok = ((uintptr_t)crops & 15) == 0;
  if (R > 0) {
    with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
      hipLaunchKernelGGL((frame_rmax_kernel<T>), dim3(R, S), dim3(256), 0, st, (const T*)crops, points, ws, PH, PW, H, W, vec_ok); });
  }
  hipLaunchKernelGGL(frame_thresholds_kernel, dim3(F), dim3(64), 0, st, ws, frame_start, S, start, step, rmax, thr, retries, flag);
}

void launch_scatter_crops_frames(const void* crops, const float* points, const int* frame_start, const float* thr, float* depth, float* response,
                                 int F, int PH, int PW, int H, int W, int dtype, hipStream_t st) {
  const dim3 grid((unsigned)cdiv(W, SF_TW), (unsigned)cdiv(H, SF_TH), (unsigned)F);
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
    hipLaunchKernelGGL((scatter_frames_kernel<T>), grid, dim3(256), 0, st, (const T*)crops, points, frame_start, thr, depth, response, PH, PW, H, W); });
}

}  // namespace rd
