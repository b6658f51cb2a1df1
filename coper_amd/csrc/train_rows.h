// Deferred rows of the sampled training step (include/coper_hip.h, coper_train_defer_rows): the kernels.
//
// A row of ent_emb / pred_bias that gets no gradient for k steps needs no work in those steps: its dense AMSGrad update is a closed
// form of (p, m, v, v_hat) and k (rows_catch_up below), applied when something reads the row.  State: one int32 word per row, "current
// as of update number w" (TrainState::rows_now counts the updates), a claim bitmap of E bits, and two id lists (this call's rows; the
// rows of the call before, whose gradient rows and claim bits the next call clears).  Every kernel here touches listed rows only --
// except k_rows_sync and k_rows_stats, which walk E on request.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "train_gemm.h"

namespace coper {
namespace {

// The tables as the row kernels see them: ent_emb [E, d] and pred_bias [E] with their gradient and slots, and the per-row step words.
struct RowTables {
  float *p, *g, *m, *v, *vh;        // ent_emb
  float *bp, *bg, *bm, *bv, *bvh;   // pred_bias
  int32_t* word;                    // [E]
  int64_t E;
  int d;
  int vec;                          // d % 4 == 0 and the five ent_emb pointers 16-byte aligned: 16-byte accesses
};

// What a catch-up needs of the optimizer's state, formed on the host at launch.  The powers are the state's CURRENT ones (beta^t as the
// next update will use them) and the update i steps back used beta^t / beta^i -- carried as log2 (l2b1p, l2b2p: TrainState keeps them
// beside the doubles), so that the quotient is still right when beta1^t itself has underflowed (t > 7,000 at beta1 = 0.9).
struct RowCatchUp {
  double lr, b1, b2, eps;
  double l2b1, l2b2, l2b1p, l2b2p;  // log2 of beta1, beta2 and of the current powers
  float b2f;                        // beta2 as the dense kernel multiplies by it
  int32_t now;                      // TrainState::rows_now
  int32_t jmax;                     // terms of C kept: beta1^j below 2^-53 of the sum beyond it (from beta1: rows_jmax)
};

// 1. Claim: one thread per id of e1 [B] and lookup [B L], clamped as k_tr_conv_fwd / k_tr_score_bwd / k_tr_build_S clamp them (outside
// [0, E): row 0).  The first claimer of a row's bit appends the row; one returning atomic per wave reserves the wave's list entries.
// count <= the unique ids <= n = the list's capacity.
__global__ __launch_bounds__(256) void k_rows_claim(const int64_t* __restrict__ e1, int64_t B, const int32_t* __restrict__ lookup, int64_t n,
                                                    int64_t E, unsigned* __restrict__ claim, int32_t* __restrict__ list, int32_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool mine = false;
  int64_t row = 0;
  if (i < n) {
    row = i < B ? e1[i] : (int64_t)lookup[i - B];
    if (row < 0 || row >= E) row = 0;
    const unsigned bit = 1u << (row & 31);
    mine = (atomicOr(claim + (row >> 5), bit) & bit) == 0u;
  }
  const unsigned long long mask = __ballot(mine);
  if (mask == 0ull) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)mask) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(count, (int)__popcll(mask));
  base = __shfl(base, leader, 64);
  if (mine) list[base + (int)__popcll(mask & ((1ull << lane) - 1ull))] = (int32_t)row;
}

// The closed form's scalars for a gap of k updates, by the 64 lanes of a wave together (every lane returns the same values):
//   C = sum_{j=1..k} lr(now - k + j) beta1^j,  lr(t) = lr sqrt(1 - beta2^t) / (1 - beta1^t),  and beta1^k, beta2^k.
// Terms beyond jmax are below 2^-53 of the sum.
// x^n, n >= 0, by squaring: a dozen multiplications where pow() is a few hundred instructions per lane
__device__ __forceinline__ double rows_powi(double x, int n) {
  double r = 1.0;
  for (; n; n >>= 1, x *= x)
    if (n & 1) r *= x;
  return r;
}
__device__ __forceinline__ void rows_gap_scalars(const RowCatchUp& cu, int k, int lane, double& Cs, double& b1k, double& b2k) {
  const int kk = k < cu.jmax ? k : cu.jmax;
  // the powers as of the row's own update, beta^(t - k); update j of the gap used beta^(t - k + j - 1)
  const double q1 = exp2(cu.l2b1p - (double)k * cu.l2b1), q2 = exp2(cu.l2b2p - (double)k * cu.l2b2);
  double c = 0.0;
  for (int j = 1 + lane; j <= kk; j += 64) {
    const double bj1 = rows_powi(cu.b1, j - 1), bj2 = rows_powi(cu.b2, j - 1);
    c += cu.lr * sqrt(1.0 - q2 * bj2) / (1.0 - q1 * bj1) * (bj1 * cu.b1);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);   // (a butterfly: every lane adds the same pairs in the same order)
  Cs = c;
  b1k = rows_powi(cu.b1, k);
  b2k = rows_powi(cu.b2, k);
}

// One element of a row through k zero-gradient updates: v_hat takes beta2 v once (v only shrinks afterwards; covers a planted v > v_hat),
// m and v one rounded power each, p one rounding.
__device__ __forceinline__ void rows_elem_catch_up(float& p, float& m, float& v, float& vh, double Cs, float b1kf, float b2kf, float b2f, double eps) {
  const float vhn = fmaxf(vh, b2f * v);
  p = (float)((double)p - Cs * (double)m / (sqrt((double)vhn) + eps));
  m *= b1kf;
  v *= b2kf;
  vh = vhn;
}

// ---- a row AS OF THE CURRENT UPDATE, in registers (the CURRENT forms of the sampled scorer's row load, train_kernels.h):
// what k_rows_catch_up would store in p, formed from p, m, v, v_hat as they stand; nothing is written.
// C of every lane's own gap k (k <= 0: the row is current, 0 is returned and nothing is computed for it), by the wave together: the
// gaps of the wave are served one distinct value at a time through rows_gap_scalars, so C has the bits a catch-up of the row computes.
// EVERY lane of the wave calls this, converged.  (Rows no step has named share one gap: a wave usually serves a handful of values.)
__device__ __forceinline__ double rows_wave_C(const RowCatchUp& cu, int k, int lane) {
  double mine = 0.0;
  unsigned long long todo = __ballot(k > 0);
  while (todo != 0ull) {      // (uniform)
    const int ku = __shfl(k, __ffsll((long long)todo) - 1, 64);
    double Cs, b1k, b2k;
    rows_gap_scalars(cu, ku, lane, Cs, b1k, b2k);
    if (k == ku) mine = Cs;
    todo &= ~__ballot(k == ku);
  }
  return mine;
}
// element(s) of a row that is behind (C from rows_wave_C of its gap): rows_elem_catch_up on copies, p kept
__device__ __forceinline__ float rows_elem_current(float p, float m, float v, float vh, double Cs, const RowCatchUp& cu) {
  rows_elem_catch_up(p, m, v, vh, Cs, 1.f, 1.f, cu.b2f, cu.eps);      // (the powers of the gap scale m and v only)
  return p;
}
// p = four elements of ent_emb at float offset o (a multiple of 4; the slots are 16-byte aligned)
__device__ __forceinline__ float4 rows_current4(const RowTables& t, const RowCatchUp& cu, int64_t o, float4 p, double Cs) {
  const float4 m = *(const float4*)(t.m + o), v = *(const float4*)(t.v + o), h = *(const float4*)(t.vh + o);
  p.x = rows_elem_current(p.x, m.x, v.x, h.x, Cs, cu);
  p.y = rows_elem_current(p.y, m.y, v.y, h.y, Cs, cu);
  p.z = rows_elem_current(p.z, m.z, v.z, h.z, Cs, cu);
  p.w = rows_elem_current(p.w, m.w, v.w, h.w, Cs, cu);
  return p;
}
__device__ __forceinline__ float rows_current1(const RowTables& t, const RowCatchUp& cu, int64_t o, float p, double Cs) {
  return rows_elem_current(p, t.m[o], t.v[o], t.vh[o], Cs, cu);
}
// pred_bias[row] of a row that is behind
__device__ __forceinline__ float rows_current_bias(const RowTables& t, const RowCatchUp& cu, int64_t row, float bp, double Cs) {
  return rows_elem_current(bp, t.bm[row], t.bv[row], t.bvh[row], Cs, cu);
}

// a wave brings `row` current (gap k > 0): ent_emb's row by its lanes, pred_bias's element by lane 0; then the step word
__device__ __forceinline__ void rows_catch_up(const RowTables& t, const RowCatchUp& cu, int64_t row, int k, int lane) {
  double Cs, b1k, b2k;
  rows_gap_scalars(cu, k, lane, Cs, b1k, b2k);
  const float b1kf = (float)b1k, b2kf = (float)b2k;
  const int64_t o = row * t.d;
  if (t.vec) {
    float4 *p4 = (float4*)(t.p + o), *m4 = (float4*)(t.m + o), *v4 = (float4*)(t.v + o), *h4 = (float4*)(t.vh + o);
    for (int q = lane; q < (t.d >> 2); q += 64) {
      float4 p = p4[q], m = m4[q], v = v4[q], h = h4[q];
      rows_elem_catch_up(p.x, m.x, v.x, h.x, Cs, b1kf, b2kf, cu.b2f, cu.eps);
      rows_elem_catch_up(p.y, m.y, v.y, h.y, Cs, b1kf, b2kf, cu.b2f, cu.eps);
      rows_elem_catch_up(p.z, m.z, v.z, h.z, Cs, b1kf, b2kf, cu.b2f, cu.eps);
      rows_elem_catch_up(p.w, m.w, v.w, h.w, Cs, b1kf, b2kf, cu.b2f, cu.eps);
      p4[q] = p; m4[q] = m; v4[q] = v; h4[q] = h;
    }
  } else {
    for (int q = lane; q < t.d; q += 64)
      rows_elem_catch_up(t.p[o + q], t.m[o + q], t.v[o + q], t.vh[o + q], Cs, b1kf, b2kf, cu.b2f, cu.eps);
  }
  if (lane == 0) {
    rows_elem_catch_up(t.bp[row], t.bm[row], t.bv[row], t.bvh[row], Cs, b1kf, b2kf, cu.b2f, cu.eps);
    t.word[row] = cu.now;
  }
}

// 2. Catch up: a wave per listed row, in front of every forward kernel.  (A listed id is a clamped one: inside [0, E).)
__global__ __launch_bounds__(256) void k_rows_catch_up(RowTables t, RowCatchUp cu, const int32_t* __restrict__ list, const int32_t* __restrict__ count) {
  const int n = *count, lane = threadIdx.x & 63;
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
    const int64_t row = list[i];
    const int k = cu.now - t.word[row];
    if (k > 0) rows_catch_up(t, cu, row, k, lane);
  }
}

// 6. Sync: the same over all E rows, grid-stride; a row with gap 0 is skipped without a write.
__global__ __launch_bounds__(256) void k_rows_sync(RowTables t, RowCatchUp cu) {
  const int lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < t.E; row += (int64_t)gridDim.x * 4) {
    const int k = cu.now - t.word[row];
    if (k > 0) rows_catch_up(t, cu, row, k, lane);
  }
}

// 3. Norm: the squares of the listed rows of d(ent_emb) and d(pred_bias) into the squared-norm slots the other leaves use (every other
// row of the two buffers is zero: k_rows_rezero).
__global__ __launch_bounds__(256) void k_rows_sumsq(RowTables t, const int32_t* __restrict__ list, const int32_t* __restrict__ count,
                                                    double* __restrict__ acc) {
  __shared__ double part[4];
  const int n = *count, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double a = 0.0;
  for (int i = blockIdx.x * 4 + w; i < n; i += gridDim.x * 4) {
    const int64_t row = list[i], o = row * t.d;
    if (t.vec) {
      const float4* g4 = (const float4*)(t.g + o);
      for (int q = lane; q < (t.d >> 2); q += 64) {
        const float4 g = g4[q];
        a += (double)g.x * g.x + (double)g.y * g.y + (double)g.z * g.z + (double)g.w * g.w;
      }
    } else {
      for (int q = lane; q < t.d; q += 64) a += (double)t.g[o + q] * t.g[o + q];
    }
    if (lane == 0) a += (double)t.bg[row] * t.bg[row];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if (lane == 0) part[w] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double s = part[0] + part[1] + part[2] + part[3];
    if (s != 0.0) atomicAdd(acc + blockIdx.x % TG_SUMSQ_SLOTS, s);
  }
}

// 4. Update: k_tr_amsgrad's arithmetic on the listed rows -- the same sum of the slots, the same clip factor, the same expressions per
// element -- then the rows' step word (now + 1: current as of this update).
__device__ __forceinline__ void rows_elem_update(float g, float& p, float& m, float& v, float& vh, float scale, float lr_t, float b1, float b2, float eps) {
  const float gi = g * scale;
  const float mi = b1 * m + (1.f - b1) * gi;
  const float vi = b2 * v + (1.f - b2) * gi * gi;
  const float vhi = fmaxf(vh, vi);
  m = mi; v = vi; vh = vhi;
  p -= lr_t * mi / (sqrtf(vhi) + eps);
}
__global__ __launch_bounds__(256) void k_rows_update(RowTables t, const int32_t* __restrict__ list, const int32_t* __restrict__ count,
                                                     const double* __restrict__ ssq, float clip, float lr_t, float b1, float b2, float eps,
                                                     double gs, int32_t word_after) {
  double ss = 0;
  for (int i = 0; i < TG_SUMSQ_SLOTS; ++i) ss += ssq[i];
  const double gn = fabs(gs) * sqrt(ss);
  const float scale = (float)(gs * (double)clip / (gn > (double)clip ? gn : (double)clip));
  const int n = *count, lane = threadIdx.x & 63;
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
    const int64_t row = list[i], o = row * t.d;
    if (t.vec) {
      const float4* g4 = (const float4*)(t.g + o);
      float4 *p4 = (float4*)(t.p + o), *m4 = (float4*)(t.m + o), *v4 = (float4*)(t.v + o), *h4 = (float4*)(t.vh + o);
      for (int q = lane; q < (t.d >> 2); q += 64) {
        const float4 g = g4[q];
        float4 p = p4[q], m = m4[q], v = v4[q], h = h4[q];
        rows_elem_update(g.x, p.x, m.x, v.x, h.x, scale, lr_t, b1, b2, eps);
        rows_elem_update(g.y, p.y, m.y, v.y, h.y, scale, lr_t, b1, b2, eps);
        rows_elem_update(g.z, p.z, m.z, v.z, h.z, scale, lr_t, b1, b2, eps);
        rows_elem_update(g.w, p.w, m.w, v.w, h.w, scale, lr_t, b1, b2, eps);
        p4[q] = p; m4[q] = m; v4[q] = v; h4[q] = h;
      }
    } else {
      for (int q = lane; q < t.d; q += 64)
        rows_elem_update(t.g[o + q], t.p[o + q], t.m[o + q], t.v[o + q], t.vh[o + q], scale, lr_t, b1, b2, eps);
    }
    if (lane == 0) {
      rows_elem_update(t.bg[row], t.bp[row], t.bm[row], t.bv[row], t.bvh[row], scale, lr_t, b1, b2, eps);
      t.word[row] = word_after;
    }
  }
}

// 5. Re-zero: the rows the call before listed -- their rows of the two gradient buffers, their claim bits -- and the OTHER list's count,
// which the claim that follows appends from (nothing else reads it in between).  Several rows share a bitmap word: an atomic clears a bit.
__global__ __launch_bounds__(256) void k_rows_rezero(RowTables t, const int32_t* __restrict__ list, const int32_t* __restrict__ count,
                                                     unsigned* __restrict__ claim, int32_t* __restrict__ other_count) {
  const int n = *count, lane = threadIdx.x & 63;
  if (blockIdx.x == 0 && threadIdx.x == 0) *other_count = 0;
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += gridDim.x * 4) {
    const int64_t row = list[i], o = row * t.d;
    if (t.vec) {
      float4* g4 = (float4*)(t.g + o);
      for (int q = lane; q < (t.d >> 2); q += 64) g4[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      for (int q = lane; q < t.d; q += 64) t.g[o + q] = 0.f;
    }
    if (lane == 0) {
      t.bg[row] = 0.f;
      atomicAnd(claim + (row >> 5), ~(1u << (row & 31)));
    }
  }
}

// coper_train_row_stats: rows whose word is behind `now`, and the largest gap; out[0] += rows behind, out[1] = max gap
__global__ __launch_bounds__(256) void k_rows_stats(const int32_t* __restrict__ word, int64_t E, int32_t now, unsigned long long* __restrict__ out) {
  unsigned long long behind = 0, gap = 0;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < E; r += (int64_t)gridDim.x * 256) {
    const int k = now - word[r];
    if (k > 0) { ++behind; gap = (unsigned long long)k > gap ? (unsigned long long)k : gap; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    behind += __shfl_xor(behind, o, 64);
    const unsigned long long u = __shfl_xor(gap, o, 64);
    gap = u > gap ? u : gap;
  }
  if ((threadIdx.x & 63) == 0 && behind) { atomicAdd(out, behind); atomicMax(out + 1, gap); }
}

// ---- the step in calls (include/coper_hip.h, "Deferred rows: the step in calls").  What crosses the boundary for the two
// tables is a ROW BLOCK: ids int32 [row_cap] and vals float [row_cap, rs], rs = (d + 1 + 3) & ~3 -- columns [0, d) the row of d(ent_emb),
// column d the row's d(pred_bias), the pad columns 0.  vec: d % 4 == 0, the tables' pointers (RowTables::vec) and vals 16-byte aligned.
constexpr int ROWS_BLOCK_INFLIGHT = 4;      // rows of a wave whose loads are issued before the first store

// 7. Export: a wave per listed row (grid-stride, ROWS_BLOCK_INFLIGHT rows of a wave in flight): ids[i] = the row, vals[i] = its gradient
// row and bias gradient, copied; ids[count .. row_cap) = -1 by all threads behind; *count_out = count.  A gather of 2 rows rs 4 bytes.
// The host has checked row_cap against its bound of the list's length; the kernel takes the smaller of the two all the same.
__global__ __launch_bounds__(256) void k_rows_export(RowTables t, const int32_t* __restrict__ list, const int32_t* __restrict__ count,
                                                     int32_t* __restrict__ ids, float* __restrict__ vals, int rs, int vec, int64_t row_cap,
                                                     int32_t* __restrict__ count_out) {
  const int64_t n = (int64_t)*count < row_cap ? (int64_t)*count : row_cap;
  const int lane = threadIdx.x & 63;
  const int64_t W = (int64_t)gridDim.x * 4;
  if (blockIdx.x == 0 && threadIdx.x == 0 && count_out) *count_out = (int32_t)n;
  for (int64_t i0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i0 < n; i0 += ROWS_BLOCK_INFLIGHT * W) {
    int64_t row[ROWS_BLOCK_INFLIGHT];
#pragma unroll
    for (int u = 0; u < ROWS_BLOCK_INFLIGHT; ++u) row[u] = i0 + u * W < n ? (int64_t)list[i0 + u * W] : -1;
    if (vec) {
      const int d4 = t.d >> 2;
      for (int q = lane; q < d4; q += 64) {
        float4 v[ROWS_BLOCK_INFLIGHT];
#pragma unroll
        for (int u = 0; u < ROWS_BLOCK_INFLIGHT; ++u)
          if (row[u] >= 0) v[u] = ((const float4*)(t.g + row[u] * t.d))[q];
#pragma unroll
        for (int u = 0; u < ROWS_BLOCK_INFLIGHT; ++u)
          if (row[u] >= 0) ((float4*)(vals + (i0 + u * W) * rs))[q] = v[u];
      }
    } else {
      for (int q = lane; q < t.d; q += 64) {
        float v[ROWS_BLOCK_INFLIGHT];
#pragma unroll
        for (int u = 0; u < ROWS_BLOCK_INFLIGHT; ++u)
          if (row[u] >= 0) v[u] = t.g[row[u] * t.d + q];
#pragma unroll
        for (int u = 0; u < ROWS_BLOCK_INFLIGHT; ++u)
          if (row[u] >= 0) vals[(i0 + u * W) * rs + q] = v[u];
      }
    }
    if (lane == 0) {      // the id, the bias column, the pad columns
      float b[ROWS_BLOCK_INFLIGHT];
#pragma unroll
      for (int u = 0; u < ROWS_BLOCK_INFLIGHT; ++u)
        if (row[u] >= 0) b[u] = t.bg[row[u]];
#pragma unroll
      for (int u = 0; u < ROWS_BLOCK_INFLIGHT; ++u) {
        if (row[u] < 0) continue;
        const int64_t i = i0 + u * W;
        ids[i] = (int32_t)row[u];
        if (vec) ((float4*)(vals + i * rs))[t.d >> 2] = make_float4(b[u], 0.f, 0.f, 0.f);
        else {
          vals[i * rs + t.d] = b[u];
          for (int c = t.d + 1; c < rs; ++c) vals[i * rs + c] = 0.f;
        }
      }
    }
  }
  for (int64_t j = n + (int64_t)blockIdx.x * 256 + threadIdx.x; j < row_cap; j += (int64_t)gridDim.x * 256) ids[j] = -1;
}

// 8. Import: a thread per block entry, a wave per 64 of them, three jobs in one launch -- no job of one wave waits for another wave.
//   claim + append: k_rows_claim's form; an entry outside [0, E) is padding and does not vote.  The thread that sets a row's claim bit is
//     the one that writes its list entry (list_cap: the host's bound holds; the kernel does not rely on it for its stores).
//   catch-up: the rows this wave appended, one after the other by the whole wave (rows_catch_up; a current row has gap 0 and is skipped,
//     so a row is brought current once however often it is imported).  Rows that were listed already are current: whoever listed them
//     brought them current.
//   add: g[row] += vals[i], d(pred_bias)[row] += vals[i][d], entry after entry of the wave, ROWS_BLOCK_INFLIGHT entries' loads in
//     flight.  Plain loads and stores: the ids of a block are distinct, so an element has one writer per launch, and launches on a stream
//     add in call order.  The gradient row of a row that was not listed is zero (the mode's invariant), so the add is right for rows
//     appended by this very launch too, whichever wave appended them.  (A block that names a row twice: two waves read, add and
//     write -- some sum of the two, nothing else.)
__global__ __launch_bounds__(256) void k_rows_import(RowTables t, RowCatchUp cu, const int32_t* __restrict__ ids, const float* __restrict__ vals,
                                                     int rs, int vec, int64_t n, unsigned* __restrict__ claim, int32_t* __restrict__ list,
                                                     int32_t* __restrict__ count, int64_t list_cap) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, i_wave = i - lane;
  int row = -1;
  if (i < n) {
    row = ids[i];
    if (row < 0 || (int64_t)row >= t.E) row = -1;
  }
  bool mine = false;
  if (row >= 0) {
    const unsigned bit = 1u << (row & 31);
    mine = (atomicOr(claim + (row >> 5), bit) & bit) == 0u;
  }
  const unsigned long long valid = __ballot(row >= 0);
  if (valid == 0ull) return;      // (the whole wave)
  const unsigned long long fresh = __ballot(mine);
  if (fresh != 0ull) {
    const int leader = __ffsll((long long)fresh) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(count, (int)__popcll(fresh));
    base = __shfl(base, leader, 64);
    if (mine) {
      const int64_t at = (int64_t)base + (int64_t)__popcll(fresh & ((1ull << lane) - 1ull));
      if (at < list_cap) list[at] = row;
    }
    for (unsigned long long mm = fresh; mm != 0ull; mm &= mm - 1ull) {
      const int64_t r = __shfl(row, __ffsll((long long)mm) - 1, 64);
      const int k = cu.now - t.word[r];
      if (k > 0) rows_catch_up(t, cu, r, k, lane);
    }
  }
  unsigned long long mm = valid;
  while (mm != 0ull) {
    int64_t r[ROWS_BLOCK_INFLIGHT], e[ROWS_BLOCK_INFLIGHT];
#pragma unroll
    for (int u = 0; u < ROWS_BLOCK_INFLIGHT; ++u) {
      r[u] = -1; e[u] = 0;
      if (mm != 0ull) {
        const int j = __ffsll((long long)mm) - 1;
        mm &= mm - 1ull;
        r[u] = __shfl(row, j, 64);
        e[u] = i_wave + j;
      }
    }
    if (vec) {
      const int d4 = t.d >> 2;
      for (int q = lane; q < d4; q += 64) {
        float4 a[ROWS_BLOCK_INFLIGHT], g[ROWS_BLOCK_INFLIGHT];
#pragma unroll
        for (int u = 0; u < ROWS_BLOCK_INFLIGHT; ++u)
          if (r[u] >= 0) { a[u] = ((const float4*)(vals + e[u] * rs))[q]; g[u] = ((const float4*)(t.g + r[u] * t.d))[q]; }
#pragma unroll
        for (int u = 0; u < ROWS_BLOCK_INFLIGHT; ++u)
          if (r[u] >= 0) ((float4*)(t.g + r[u] * t.d))[q] = make_float4(g[u].x + a[u].x, g[u].y + a[u].y, g[u].z + a[u].z, g[u].w + a[u].w);
      }
    } else {
      for (int q = lane; q < t.d; q += 64) {
        float a[ROWS_BLOCK_INFLIGHT], g[ROWS_BLOCK_INFLIGHT];
#pragma unroll
        for (int u = 0; u < ROWS_BLOCK_INFLIGHT; ++u)
          if (r[u] >= 0) { a[u] = vals[e[u] * rs + q]; g[u] = t.g[r[u] * t.d + q]; }
#pragma unroll
        for (int u = 0; u < ROWS_BLOCK_INFLIGHT; ++u)
          if (r[u] >= 0) t.g[r[u] * t.d + q] = g[u] + a[u];
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < ROWS_BLOCK_INFLIGHT; ++u)
        if (r[u] >= 0) t.bg[r[u]] += vals[e[u] * rs + t.d];
    }
  }
}

}  // namespace
}  // namespace coper
