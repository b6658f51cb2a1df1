// Entity-sharded 1-vs-all training (include/coper_hip.h "Entity-sharded training"): the kernels that only the sharded step
// launches.  Deterministic by construction: no float atomics, one writer per element, every sum in one order that does not depend on
// the route (16-byte or scalar) that loads its addends.  The score phase itself is Step::score_csr over the handle's own rows, or
// (sampled labels) the sampled scorer (Step::fwd_score_loss + bwd_scorer) on a plan that names the own rows: the SHARD forms
// of the sampled-scorer kernels in train_kernels.h and k_ord_reduce over the own rows' range.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace coper {
namespace {

// ids[b] = b: the "e1" of a forward pass whose input image is row b of the gathered [B, d] rows
__global__ __launch_bounds__(256) void k_shard_iota(int64_t* __restrict__ ids, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) ids[i] = i;
}

// dh[i] = parts[0][i], then += parts[1][i], ... in ascending g (parts: [G][n]); the loss shares the same way in double, by thread 0
// of workgroup 0.  vec: n % 4 == 0 and both arrays 16-byte aligned -- 16-byte loads, the same additions per element.
__global__ __launch_bounds__(256) void k_shard_fold_parts(const float* __restrict__ parts, int G, int64_t n, int vec, float* __restrict__ dh,
                                                          const double* __restrict__ loss_parts, double* __restrict__ loss) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (vec) {
    const int64_t n4 = n >> 2;
    for (; i < n4; i += stride) {
      float4 a = reinterpret_cast<const float4*>(parts)[i];
      for (int g = 1; g < G; ++g) {
        const float4 p = reinterpret_cast<const float4*>(parts + (size_t)g * n)[i];
        a.x += p.x; a.y += p.y; a.z += p.z; a.w += p.w;
      }
      reinterpret_cast<float4*>(dh)[i] = a;
    }
  } else {
    for (; i < n; i += stride) {
      float a = parts[i];
      for (int g = 1; g < G; ++g) a += parts[(size_t)g * n + i];
      dh[i] = a;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double l = loss_parts[0];
    for (int g = 1; g < G; ++g) l += loss_parts[g];
    loss[0] = l;
  }
}

// k_tr_rows_by_key_det for a shard of the destination: dst holds rows [lo, lo + n_local) of a table of K rows, and only the keys in
// that range have a writer -- the workgroup of the key's first sample, its addends in ascending b onto what dst[key - lo] holds.  A
// key of another shard is dropped without a store; keys outside [0, K) count as 0, as everywhere in the step.
// vec: n, stride and col0 multiples of 4, src and dst 16-byte aligned: a thread carries four columns; per element the same chain.
__global__ __launch_bounds__(256) void k_shard_rows_by_key(const float* __restrict__ src, int64_t stride, int64_t col0, int n,
                                                           const int64_t* __restrict__ keys, int64_t K, int64_t B, int64_t lo, int64_t n_local,
                                                           int vec, float* __restrict__ dst) {
  __shared__ int64_t kc[256];
  const int64_t b = blockIdx.x;
  auto key = [&](int64_t i) { const int64_t k = keys[i]; return (k < 0 || k >= K) ? (int64_t)0 : k; };
  const int64_t k = key(b);
  if (k < lo || k >= lo + n_local) return;      // (uniform: another shard's row)
  int earlier = 0;
  for (int64_t i = threadIdx.x; i < b; i += 256) earlier |= key(i) == k ? 1 : 0;
  if (__syncthreads_or(earlier)) return;      // (uniform)
  float* const drow = dst + (k - lo) * n;
  const int per = vec ? 4 : 1;
  for (int t0 = 0; t0 < n; t0 += 256 * per) {
    const int t = t0 + (int)threadIdx.x * per;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < n) {
      if (vec) a = *reinterpret_cast<const float4*>(drow + t);
      else a.x = drow[t];
    }
    for (int64_t i0 = b; i0 < B; i0 += 256) {
      __syncthreads();
      kc[threadIdx.x] = i0 + threadIdx.x < B ? key(i0 + threadIdx.x) : (int64_t)-1;
      __syncthreads();
      const int m = (int)(B - i0 < 256 ? B - i0 : 256);
      if (t < n)
        for (int u = 0; u < m; ++u)
          if (kc[u] == k) {
            const float* const sp = src + (i0 + u) * stride + col0 + t;
            if (vec) {
              const float4 v = *reinterpret_cast<const float4*>(sp);
              a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
            } else
              a.x += sp[0];
          }
    }
    if (t < n) {
      if (vec) *reinterpret_cast<float4*>(drow + t) = a;
      else drow[t] = a.x;
    }
  }
}

// the squared-norm slots of the update: slot 0 holds the small leaves' share (k_tr_sumsq<true> + k_tr_fold_det), slots 1 .. G take
// the shards' table shares in rank order -- k_tr_amsgrad adds the slots in index order (the rest are zero), on every rank alike
__global__ void k_shard_place_sumsq(const double* __restrict__ parts, int G, double* __restrict__ slots) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < G) slots[1 + g] = parts[g];
}

}  // namespace
}  // namespace coper
