// Softmax ('full') attention  softmax(scale * Q K^T) V  with token masks, on MFMA with LDS-staged per-head tiles (fp32 accumulate).
//
// Reference: RCNet/linear_attention.py:49-80 (FullAttention.forward, use_dropout = False)
//   QK[n,l,s,h] = q[n,l,h,:] . k[n,s,h,:]                       (D = 16)
//   QK = -inf where not (q_mask[n,l] and kv_mask[n,s])
//   A  = softmax(scale * QK, dim = s),  scale = 1 / sqrt(D)
//   out[n,l,h,:] = sum_s A[n,l,s,h] v[n,s,h,:]
// Geometry as rd_attention.hip: one wave owns one (n, h) pair, four waves per block, 1 <= L, S <= 32, token matrices with explicit pitches,
// 16-byte staging loads where pointers and pitches allow.  Phases of a wave (ordered by wave_sync()):
//   1. stage raw q, k, v (and dout) into the wave's private LDS, rows beyond L / S zero; token validity (masks and lengths) as 0 / 1 floats
//   2. scores on v_mfma_f32_16x16x4_f32 as up to 2 x 2 tiles of 16 x 16 over K = 16 (the k tile is walked with pitch 17), times scale;
//      into the LDS tile [32][33]; one query row per lane: row maximum over the admissible keys (without it exp() overflows once a score
//      passes 88) and the sum of exp(x - max), keys ascending; A = exp(x - max) / sum (0 where inadmissible) back into the tile
//   3. forward: out = A V on the MFMA (contracting over all 32 padded rows adds exact zeros)
//      backward (saves nothing but q, k, v: A is recomputed):  dV = A^T dO,  dA = dO V^T,  dS = scale * A * (dA - rowsum(dA * A)),
//      dS replaces A in LDS,  dQ = dS K,  dK = dS^T Q
// Masks: uint8 [N][L] / [N][S], nonzero = valid (the storage of a torch.bool tensor), either pointer may be NULL = all valid; a pair (l, s) is
// admissible iff both tokens are valid.
// ZERO-ROW RULE (a deliberate difference from the reference, whose softmax over a row of -inf is NaN): a query row with no admissible key
// has A = 0 -- its output row is exactly 0, its dq row is exactly 0, and it contributes nothing to dk / dv.  dk and dv rows of masked keys are
// exact zeros (their column of A and of dS is 0).  Every row of every output is written on every call.
// LDS: 4 tiles [32][17] + 1 tile [32][33] + 4 x 32 floats (validity, row maximum, 1 / row sum) = 13440 bytes per wave, 53760 per block: three
// blocks per CU (161280 of the 163840 bytes).
#include "rd_attention_head.h"

namespace rd {

static constexpr int LDA = 33;   // row pitch (floats) of the [32][32] attention tile

struct FullSmem {
  float q[MAXR * LD], k[MAXR * LD], v[MAXR * LD], d[MAXR * LD];
  float a[MAXR * LDA];
  float qok[MAXR], kok[MAXR], rmax[MAXR], rinv[MAXR];
};

// rows x 16 head slice -> dst[MAXR][LD], raw values, rows beyond `rows` (and everything of an inactive wave) zero; element-wise path
template <typename T>
__device__ __forceinline__ void stage_raw(const T* __restrict__ src, int64_t row0, int ld, int col0, int rows, float* dst, bool active) {
  const int lane = threadIdx.x & 63;
  for (int idx = lane; idx < MAXR * 16; idx += 64) {
    const int r = idx >> 4, c = idx & 15;
    float x = 0.f;
    if (active && r < rows) x = Elem<T>::ld(src + (row0 + r) * ld + col0 + c);
    dst[r * LD + c] = x;
  }
}

template <typename T, bool BWD>
__global__ __launch_bounds__(256) void full_attention_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
                                                             const T* __restrict__ dout, T* __restrict__ out, T* __restrict__ dq,
                                                             T* __restrict__ dk, T* __restrict__ dv, const uint8_t* __restrict__ q_mask,
                                                             const uint8_t* __restrict__ kv_mask, int N, int L, int S, int H, int ldq,
                                                             int ldk, int ldv, int ldo, float scale) {
  __shared__ FullSmem sm[4];
  const int wv = threadIdx.x >> 6;
  const int pair = blockIdx.x * 4 + wv;
  const bool active = pair < N * H;
  const int n = active ? pair / H : 0, h = active ? pair % H : 0;   // inactive waves walk sequence 0 / head 0 and store nothing
  FullSmem& s = sm[wv];
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int col0 = h * 16;
  const int lt = (L + 15) >> 4, stl = (S + 15) >> 4;  // 16-row tiles

  // ---- 1. staging ----------------------------------------------------------------------------------------
  // token validity, one token per lane: lanes 0..31 the queries, lanes 32..63 the keys (indices clamped into the mask, the result discarded
  // beyond the length)
  {
    const int tkn = lane & 31;
    const bool isq = lane < 32;
    const uint8_t* mp = isq ? q_mask : kv_mask;
    const int len = isq ? L : S;
    bool ok = active && tkn < len;
    if (mp != nullptr) ok = ok && mp[(int64_t)n * len + min(tkn, len - 1)] != 0;
    (isq ? s.qok : s.kok)[tkn] = ok ? 1.f : 0.f;
  }
  constexpr int VE = Elem<T>::VE;
  const bool vec = (ldq % VE == 0) && (ldk % VE == 0) && (ldv % VE == 0) && (!BWD || ldo % VE == 0) &&
                   (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (BWD ? (uintptr_t)dout : (uintptr_t)0)) & 15) == 0;
  if (vec) {
    // 16-byte loads, all tensors' requests in flight together; rows are clamped into the sequence and zeroed afterwards (no branch around a load)
    constexpr int SPR = 16 / VE, NIT = MAXR * SPR / 64;   // slots per row, slots per lane (1 for 16-bit, 2 for fp32)
    float xq[NIT][VE], xk[NIT][VE], xv[NIT][VE], xd[BWD ? NIT : 1][VE];
#pragma unroll
    for (int i = 0; i < NIT; i++) {
      const int idx = lane + 64 * i, rr = idx / SPR, c = (idx - rr * SPR) * VE;
      const int rl = min(rr, L - 1), rs = min(rr, S - 1);
      rd::ldv(q + ((int64_t)n * L + rl) * ldq + col0 + c, xq[i]);
      rd::ldv(k + ((int64_t)n * S + rs) * ldk + col0 + c, xk[i]);
      rd::ldv(v + ((int64_t)n * S + rs) * ldv + col0 + c, xv[i]);
      if (BWD) rd::ldv(dout + ((int64_t)n * L + rl) * ldo + col0 + c, xd[i]);
    }
#pragma unroll
    for (int i = 0; i < NIT; i++) {
      const int idx = lane + 64 * i, rr = idx / SPR, c = (idx - rr * SPR) * VE;
      const bool okq = active && rr < L, okk = active && rr < S;
#pragma unroll
      for (int e = 0; e < VE; e++) {
        s.q[rr * LD + c + e] = okq ? xq[i][e] : 0.f;
        s.k[rr * LD + c + e] = okk ? xk[i][e] : 0.f;
        s.v[rr * LD + c + e] = okk ? xv[i][e] : 0.f;
        if (BWD) s.d[rr * LD + c + e] = okq ? xd[i][e] : 0.f;
      }
    }
  } else {
    stage_raw<T>(q, (int64_t)n * L, ldq, col0, L, s.q, active);
    stage_raw<T>(k, (int64_t)n * S, ldk, col0, S, s.k, active);
    stage_raw<T>(v, (int64_t)n * S, ldv, col0, S, s.v, active);
    if (BWD) stage_raw<T>(dout, (int64_t)n * L, ldo, col0, L, s.d, active);
  }
  wave_sync();

  // ---- 2. A = softmax over the admissible keys; lane (r, g) holds A[tI * 16 + g * 4 + e][tJ * 16 + r] ----------
  // 2a. x = scale * (q . k) into the attention tile, NOADM where the pair is inadmissible (every element of the [32][32] tile is written)
  constexpr float NOADM = -3.0e38f;
  float A[2][2][4];
  {
    float kok[2];
#pragma unroll
    for (int tJ = 0; tJ < 2; tJ++) kok[tJ] = s.kok[tJ * 16 + r];
#pragma unroll
    for (int tI = 0; tI < 2; tI++) {
#pragma unroll
      for (int tJ = 0; tJ < 2; tJ++) {
        f32x4 sc = f32x4{0, 0, 0, 0};
        if (tI < lt && tJ < stl) sc = wave_mm_k<16>(s.q + tI * 16 * LD, LD, 1, s.k + tJ * 16 * LD, 1, LD, sc);
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const bool adm = s.qok[tI * 16 + g * 4 + e] != 0.f && kok[tJ] != 0.f;
          A[tI][tJ][e] = adm ? sc[e] * scale : NOADM;
          s.a[(tI * 16 + g * 4 + e) * LDA + tJ * 16 + r] = A[tI][tJ][e];
        }
      }
    }
  }
  wave_sync();
  // 2b. one query row per lane: the maximum over the admissible keys (without it exp() overflows once a score passes 88) and the sum of
  // exp(x - max), keys ascending; a row with an admissible key has sum >= 1 (the maximum's own term), a row without one gets 1 / sum := 0,
  // which is the zero-row rule.  (Unrolled: the 32 reads are in flight together.)
  if (lane < MAXR) {
    float x[MAXR];
#pragma unroll
    for (int ss = 0; ss < MAXR; ss++) x[ss] = s.a[lane * LDA + ss];
    float m = NOADM;
#pragma unroll
    for (int ss = 0; ss < MAXR; ss++) m = fmaxf(m, x[ss]);
    float sum = 0.f;
#pragma unroll
    for (int ss = 0; ss < MAXR; ss++) sum += x[ss] > NOADM ? __expf(x[ss] - m) : 0.f;
    s.rmax[lane] = m;
    s.rinv[lane] = sum > 0.f ? 1.f / sum : 0.f;
  }
  wave_sync();
  // 2c. A = exp(x - max) / sum (the same exp() of the same operands as in the sum), 0 where inadmissible
#pragma unroll
  for (int tI = 0; tI < 2; tI++)
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int l = tI * 16 + g * 4 + e;
      const float m = s.rmax[l], inv = s.rinv[l];
#pragma unroll
      for (int tJ = 0; tJ < 2; tJ++) {
        const float x = A[tI][tJ][e];
        A[tI][tJ][e] = x > NOADM ? __expf(x - m) * inv : 0.f;
        s.a[l * LDA + tJ * 16 + r] = A[tI][tJ][e];
      }
    }
  wave_sync();

  if (!BWD) {
    // ---- 3. out = A V ------------------------------------------------------------------------------------
#pragma unroll
    for (int tI = 0; tI < 2; tI++) {
      if (tI < lt) {
        f32x4 o = f32x4{0, 0, 0, 0};
        o = wave_mm_k<MAXR>(s.a + tI * 16 * LDA, LDA, 1, s.v, LD, 1, o);
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int l = tI * 16 + g * 4 + e;
          if (active && l < L) Elem<T>::st(out + ((int64_t)n * L + l) * ldo + col0 + r, o[e]);
        }
      }
    }
    return;
  }

  // ---- backward --------------------------------------------------------------------------------------------
  // dV = A^T dO
#pragma unroll
  for (int tJ = 0; tJ < 2; tJ++) {
    if (tJ < stl) {
      f32x4 a = f32x4{0, 0, 0, 0};
      a = wave_mm_k<MAXR>(s.a + tJ * 16, 1, LDA, s.d, LD, 1, a);
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int ss = tJ * 16 + g * 4 + e;
        if (active && ss < S) Elem<T>::st(dv + ((int64_t)n * S + ss) * ldv + col0 + r, a[e]);
      }
    }
  }
  // dA = dO V^T, dS = scale * A * (dA - rowsum(dA * A)) in the layout of A
  float dS[2][2][4];
#pragma unroll
  for (int tI = 0; tI < 2; tI++) {
    f32x4 da[2];
#pragma unroll
    for (int tJ = 0; tJ < 2; tJ++) {
      da[tJ] = f32x4{0, 0, 0, 0};
      if (tI < lt && tJ < stl) da[tJ] = wave_mm_k<16>(s.d + tI * 16 * LD, LD, 1, s.v + tJ * 16 * LD, 1, LD, da[tJ]);
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const float rs = row16_sum(da[0][e] * A[tI][0][e] + da[1][e] * A[tI][1][e]);
      dS[tI][0][e] = scale * A[tI][0][e] * (da[0][e] - rs);
      dS[tI][1][e] = scale * A[tI][1][e] * (da[1][e] - rs);
    }
  }
  wave_sync();      // dV's reads of A are complete before dS replaces it
#pragma unroll
  for (int tI = 0; tI < 2; tI++)
#pragma unroll
    for (int e = 0; e < 4; e++) {
      s.a[(tI * 16 + g * 4 + e) * LDA + r] = dS[tI][0][e];
      s.a[(tI * 16 + g * 4 + e) * LDA + 16 + r] = dS[tI][1][e];
    }
  wave_sync();
  // dQ = dS K
#pragma unroll
  for (int tI = 0; tI < 2; tI++) {
    if (tI < lt) {
      f32x4 a = f32x4{0, 0, 0, 0};
      a = wave_mm_k<MAXR>(s.a + tI * 16 * LDA, LDA, 1, s.k, LD, 1, a);
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int l = tI * 16 + g * 4 + e;
        if (active && l < L) Elem<T>::st(dq + ((int64_t)n * L + l) * ldq + col0 + r, a[e]);
      }
    }
  }
  // dK = dS^T Q
#pragma unroll
  for (int tJ = 0; tJ < 2; tJ++) {
    if (tJ < stl) {
      f32x4 a = f32x4{0, 0, 0, 0};
      a = wave_mm_k<MAXR>(s.a + tJ * 16, 1, LDA, s.q, LD, 1, a);
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const int ss = tJ * 16 + g * 4 + e;
        if (active && ss < S) Elem<T>::st(dk + ((int64_t)n * S + ss) * ldk + col0 + r, a[e]);
      }
    }
  }
}

template <typename T>
static void launch_full(const void* q, const void* k, const void* v, const void* dout, void* out, void* dq, void* dk, void* dv,
                        const uint8_t* q_mask, const uint8_t* kv_mask, int N, int L, int S, int H, int ldq, int ldk, int ldv, int ldo,
                        float scale, bool bwd, hipStream_t st) {
  unsigned grid = (unsigned)cdiv((int64_t)N * H, 4);
  if (grid == 0) return;
  if (bwd)
    hipLaunchKernelGGL((full_attention_kernel<T, true>), dim3(grid), dim3(256), 0, st, (const T*)q, (const T*)k, (const T*)v, (const T*)dout, (T*)nullptr, (T*)dq, (T*)dk, (T*)dv, q_mask, kv_mask, N, L, S, H, ldq, ldk, ldv, ldo, scale);
  else
    hipLaunchKernelGGL((full_attention_kernel<T, false>), dim3(grid), dim3(256), 0, st, (const T*)q, (const T*)k, (const T*)v, (const T*)nullptr, (T*)out, (T*)nullptr, (T*)nullptr, (T*)nullptr, q_mask, kv_mask, N, L, S, H, ldq, ldk, ldv, ldo, scale);
}

void launch_full_attention_fwd(const void* q, const void* k, const void* v, void* out, const uint8_t* q_mask, const uint8_t* kv_mask, int N,
                               int L, int S, int H, int ldq, int ldk, int ldv, int ldo, float scale, int dtype, hipStream_t st) {
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
    launch_full<T>(q, k, v, nullptr, out, nullptr, nullptr, nullptr, q_mask, kv_mask, N, L, S, H, ldq, ldk, ldv, ldo, scale, false, st); });
}
void launch_full_attention_bwd(const void* q, const void* k, const void* v, const void* dout, void* dq, void* dk, void* dv,
                               const uint8_t* q_mask, const uint8_t* kv_mask, int N, int L, int S, int H, int ldq, int ldk, int ldv, int ldo,
                               float scale, int dtype, hipStream_t st) {
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
    launch_full<T>(q, k, v, dout, nullptr, dq, dk, dv, q_mask, kv_mask, N, L, S, H, ldq, ldk, ldv, ldo, scale, true, st); });
}

}  // namespace rd
