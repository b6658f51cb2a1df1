// Entity-sharded 1-vs-all training (include/coper_hip.h "Entity-sharded training"): the kernels that only the sharded step
// launches.  Deterministic by construction: no float atomics, one writer per element, every sum in one order that does not depend on
// the route (16-byte or scalar) that loads its addends.  The score phase itself is Step::score_csr over the handle's own rows, or
// (sampled labels) the sampled scorer (Step::fwd_score_loss + bwd_scorer) on a plan that names the own rows: the SHARD forms
// of the sampled-scorer kernels in train_kernels.h and k_ord_reduce over the own rows' range.  Deferred rows on a shard:
// the gather that returns a row as of the current update, and the owned run of the step's ordered list -- at the end of this file.
// The forward-only calls launch nothing of this file: their kernels are the SHARD / CURRENT forms in train_kernels.h
// (k_tr_scores_out_shard among them) over the row helpers of train_rows.h (rows_wave_C, rows_current4).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "train_rows.h"

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

// ---- deferred rows on a shard
// coper_train_shard_gather in the mode: out[b] = the owned row e1[b] AS OF THE CURRENT UPDATE, although the table may hold it several
// updates behind -- a wave per b loads p, m, v, v_hat and the row's word, forms the gap's scalars (rows_gap_scalars) and applies
// rows_elem_catch_up to its registers: the value k_rows_catch_up would store, bit for bit.  Only `out` is written: e1 has duplicates,
// and two waves catching the same row up in place would race.  Gap 0: the row as it stands.  A row of another shard: a zero row.
// t: the handle's own rows (t.E of them, the first is entity `lo`).  vec: t.vec and out 16-byte aligned.
__global__ __launch_bounds__(256) void k_shard_gather_current(RowTables t, RowCatchUp cu, const int64_t* __restrict__ e1, int64_t B, int64_t lo,
                                                              int vec, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < B; b += (int64_t)gridDim.x * 4) {
    const int64_t row = e1[b] - lo;      // (wave-uniform)
    float* const dst = out + b * t.d;
    if (row < 0 || row >= t.E) {
      for (int q = lane; q < t.d; q += 64) dst[q] = 0.f;
      continue;
    }
    const int k = cu.now - t.word[row];
    const int64_t o = row * t.d;
    if (k <= 0) {
      for (int q = lane; q < t.d; q += 64) dst[q] = t.p[o + q];
      continue;
    }
    double Cs, b1k, b2k;
    rows_gap_scalars(cu, k, lane, Cs, b1k, b2k);
    const float b1kf = (float)b1k, b2kf = (float)b2k;
    if (vec) {
      const float4 *p4 = (const float4*)(t.p + o), *m4 = (const float4*)(t.m + o), *v4 = (const float4*)(t.v + o), *h4 = (const float4*)(t.vh + o);
      for (int q = lane; q < (t.d >> 2); q += 64) {
        float4 p = p4[q], m = m4[q], v = v4[q], h = h4[q];
        rows_elem_catch_up(p.x, m.x, v.x, h.x, Cs, b1kf, b2kf, cu.b2f, cu.eps);
        rows_elem_catch_up(p.y, m.y, v.y, h.y, Cs, b1kf, b2kf, cu.b2f, cu.eps);
        rows_elem_catch_up(p.z, m.z, v.z, h.z, Cs, b1kf, b2kf, cu.b2f, cu.eps);
        rows_elem_catch_up(p.w, m.w, v.w, h.w, Cs, b1kf, b2kf, cu.b2f, cu.eps);
        ((float4*)dst)[q] = p;
      }
    } else {
      for (int q = lane; q < t.d; q += 64) {
        float p = t.p[o + q], m = t.m[o + q], v = t.v[o + q], h = t.vh[o + q];
        rows_elem_catch_up(p, m, v, h, Cs, b1kf, b2kf, cu.b2f, cu.eps);
        dst[q] = p;
      }
    }
  }
}

// The step's row list on a shard: glist holds the batch's unique (clamped) ids in ascending order (k_ord_heads; *gcount of them), so
// the ids of [lo, lo + n_local) are one contiguous run of it.  Thread 0 of every workgroup finds the run by two binary searches; the
// run goes, as LOCAL row indices, into list[0 .. *count) with the rows' local claim bits set.  An empty run: *count = 0, nothing else
// written.  (The list's capacity is B (L + 1) >= *gcount.)
__global__ __launch_bounds__(256) void k_shard_list_owned(const int32_t* __restrict__ glist, const int32_t* __restrict__ gcount, int64_t lo,
                                                          int64_t n_local, int32_t* __restrict__ list, int32_t* __restrict__ count,
                                                          unsigned* __restrict__ claim) {
  __shared__ int run[2];
  if (threadIdx.x == 0) {
    const int n = *gcount;
    auto first_at_least = [&](int64_t id) {      // the first position whose id is >= `id` (n: none)
      int a = 0, b = n;
      while (a < b) {
        const int mid = a + ((b - a) >> 1);
        if ((int64_t)glist[mid] < id) a = mid + 1; else b = mid;
      }
      return a;
    };
    run[0] = first_at_least(lo);
    run[1] = first_at_least(lo + n_local);
    if (blockIdx.x == 0) *count = run[1] - run[0];
  }
  __syncthreads();
  const int first = run[0], last = run[1];
  for (int64_t i = (int64_t)first + (int64_t)blockIdx.x * 256 + threadIdx.x; i < last; i += (int64_t)gridDim.x * 256) {
    const int32_t row = (int32_t)((int64_t)glist[i] - lo);
    list[i - first] = row;
    atomicOr(claim + (row >> 5), 1u << (row & 31));
  }
}

}  // namespace
}  // namespace coper
