// Linear attention  phi(Q) (phi(K)^T V)  on MFMA with LDS-staged per-head tiles (fp32 accumulate).
//
// Reference: RCNet/linear_attention.py:18-45 (LinearAttention.forward; linear_attention_kernel: masks None, linear_attention_masked_kernel: with masks)
//   Q = elu(q)+1, K = elu(k)+1, V = v / S
//   KV[n,h]   = sum_s K[n,s,h,:]^T V[n,s,h,:]            (D x D,  D = 16)
//   Z[n,l,h]  = 1 / (Q[n,l,h,:] . sum_s K[n,s,h,:] + eps)
//   out       = (Q KV) * Z * S
// One wave owns one (n, h) pair: the three 21x16 head slices are staged in LDS (rows padded to 32 with zeros),
// the two contractions K^T V (16x16x32) and Q KV (32x16x16) run on v_mfma_f32_16x16x4_f32 (exact fp32),
// the normaliser on the VALU.  The backward recomputes KV / P from q,k,v (nothing but q,k,v is saved).
#include "rd_attention_head.h"

namespace rd {

template <typename T, bool BWD>
__global__ __launch_bounds__(256) void linear_attention_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                               const T* __restrict__ v, const T* __restrict__ dout,
                                                               T* __restrict__ out, T* __restrict__ dq, T* __restrict__ dk,
                                                               T* __restrict__ dv, int N, int L, int S, int H, int ldq,
                                                               int ldk, int ldv, int ldo, float eps) {
  __shared__ AttnSmem sm[4];
  const int wv = threadIdx.x >> 6;
  const int pair = blockIdx.x * 4 + wv;
  const bool active = pair < N * H;
  const int n = active ? pair / H : 0, h = active ? pair % H : 0;
  attn_head<T, BWD>(sm[wv], q, k, v, dout, out, dq, dk, dv, n, h, active, L, S, ldq, ldk, ldv, ldo, eps, []() {});
}

// The same with token masks (attn_head's MASK flag; reference :33-37): q_mask [N][L], kv_mask [N][S], uint8, nonzero = valid, either may be NULL.
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void linear_attention_masked_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                      const T* __restrict__ v, const T* __restrict__ dout,
                                                                      T* __restrict__ out, T* __restrict__ dq, T* __restrict__ dk,
                                                                      T* __restrict__ dv, const uint8_t* __restrict__ q_mask,
                                                                      const uint8_t* __restrict__ kv_mask, int N, int L, int S, int H,
                                                                      int ldq, int ldk, int ldv, int ldo, float eps) {
  __shared__ AttnSmem sm[4];
  const int wv = threadIdx.x >> 6;
  const int pair = blockIdx.x * 4 + wv;
  const bool active = pair < N * H;
  const int n = active ? pair / H : 0, h = active ? pair % H : 0;
  auto none = []() {};
  attn_head<T, BWD, decltype(none), false, false, true>(sm[wv], q, k, v, dout, out, dq, dk, dv, n, h, active, L, S, ldq, ldk, ldv, ldo, eps,
                                                        none, nullptr, 0, q_mask, kv_mask);
}

template <typename T>
static void launch_masked(const void* q, const void* k, const void* v, const void* dout, void* out, void* dq, void* dk, void* dv,
                          const uint8_t* q_mask, const uint8_t* kv_mask, int N, int L, int S, int H, int ldq, int ldk, int ldv, int ldo,
                          float eps, bool bwd, hipStream_t st) {
  unsigned grid = (unsigned)cdiv((int64_t)N * H, 4);
  if (grid == 0) return;
  if (bwd)
    hipLaunchKernelGGL((linear_attention_masked_kernel<T, true>), dim3(grid), dim3(256), 0, st, (const T*)q, (const T*)k, (const T*)v, (const T*)dout, (T*)nullptr, (T*)dq, (T*)dk, (T*)dv, q_mask, kv_mask, N, L, S, H, ldq, ldk, ldv, ldo, eps);
  else
    hipLaunchKernelGGL((linear_attention_masked_kernel<T, false>), dim3(grid), dim3(256), 0, st, (const T*)q, (const T*)k, (const T*)v, (const T*)nullptr, (T*)out, (T*)nullptr, (T*)nullptr, (T*)nullptr, q_mask, kv_mask, N, L, S, H, ldq, ldk, ldv, ldo, eps);
}
void launch_linear_attention_masked_fwd(const void* q, const void* k, const void* v, void* out, const uint8_t* q_mask, const uint8_t* kv_mask,
                                        int N, int L, int S, int H, int ldq, int ldk, int ldv, int ldo, float eps, int dtype, hipStream_t st) {
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
    launch_masked<T>(q, k, v, nullptr, out, nullptr, nullptr, nullptr, q_mask, kv_mask, N, L, S, H, ldq, ldk, ldv, ldo, eps, false, st); });
}
void launch_linear_attention_masked_bwd(const void* q, const void* k, const void* v, const void* dout, void* dq, void* dk, void* dv,
                                        const uint8_t* q_mask, const uint8_t* kv_mask, int N, int L, int S, int H, int ldq, int ldk, int ldv,
                                        int ldo, float eps, int dtype, hipStream_t st) {
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
    launch_masked<T>(q, k, v, dout, nullptr, dq, dk, dv, q_mask, kv_mask, N, L, S, H, ldq, ldk, ldv, ldo, eps, true, st); });
}

void launch_linear_attention_fwd(const void* q, const void* k, const void* v, void* out, int N, int L, int S, int H, int ldq,
                                 int ldk, int ldv, int ldo, float eps, int dtype, hipStream_t st) {
  unsigned grid = (unsigned)cdiv((int64_t)N * H, 4);
  if (grid == 0) return;
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
    hipLaunchKernelGGL((linear_attention_kernel<T, false>), dim3(grid), dim3(256), 0, st, (const T*)q, (const T*)k, (const T*)v, (const T*)nullptr, (T*)out, (T*)nullptr, (T*)nullptr, (T*)nullptr, N, L, S, H, ldq, ldk, ldv, ldo, eps); });
}
void launch_linear_attention_bwd(const void* q, const void* k, const void* v, const void* dout, void* dq, void* dk, void* dv,
                                 int N, int L, int S, int H, int ldq, int ldk, int ldv, int ldo, float eps, int dtype,
                                 hipStream_t st) {
  unsigned grid = (unsigned)cdiv((int64_t)N * H, 4);
  if (grid == 0) return;
  with_elem(dtype, [&](auto e) { using T = typename decltype(e)::type;
    hipLaunchKernelGGL((linear_attention_kernel<T, true>), dim3(grid), dim3(256), 0, st, (const T*)q, (const T*)k, (const T*)v, (const T*)dout, (T*)nullptr, (T*)dq, (T*)dk, (T*)dv, N, L, S, H, ldq, ldk, ldv, ldo, eps); });
}

}  // namespace rd
