// Ordered rows of the sampled training step (include/coper_hip.h, coper_train_order_rows): the kernels.
//
// The sparse table gradient dE[lookup[b,l]] += ds[b,l] h[b], dbias[lookup[b,l]] += ds[b,l] with ONE WRITER PER ROW and one order of
// addends: the batch's ids are sorted (stable: ascending (id, b, l)), the sorted run of an id is its segment, a wave per segment adds
// the segment's entries in that order.  The segment heads are the batch's unique rows in ascending id -- the ordered row list of the
// deferred-rows mode.
//   1. key sort: LSD radix, 8-bit digits over the bits of num_ent - 1; per pass k_ord_hist (a digit histogram per tile of
//      ORD_TILE entries), k_ord_scan (exclusive, over [digit][tile]) and k_ord_scatter (in-tile rank from wave ballots plus a prefix
//      over the waves in LDS).  Integer atomics only (the LDS histogram); the output is the stable order, which is unique.
//   2. k_ord_head_count / k_ord_heads: unique ids ascending, segment offsets, the claim bits of the listed rows.
//   3. k_ord_reduce: the segment sums, stored with `=` onto the zeroed rows.
//   4. k_rows_sumsq_ord: the squared norm of the listed rows in partial sums of ORD_SUMSQ_ROWS list positions each.
// An entry is a lookup position i = b L + l (i < B L) or the e1 id of sample i - B L: the e1 rows join the list (the conv backward's
// d(img) rows land there) and add nothing to the sums -- within a segment they sort behind every lookup entry.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/coper_hip.h"
#include "train_rows.h"

namespace coper {
namespace {

constexpr int ORD_TILE = COPER_ORDER_SORT_TILE;          // entries of a sort tile: a workgroup, ORD_TILE / 256 rounds of 256
constexpr int ORD_ROUNDS = ORD_TILE / 256;
constexpr int ORD_SUMSQ_ROWS = COPER_ORDER_SUMSQ_ROWS;   // list positions per partial sum of the ordered norm
static_assert(ORD_TILE % 256 == 0 && ORD_SUMSQ_ROWS % 4 == 0, "a tile is whole rounds of a workgroup, a partial whole rounds of its waves");

// What a sort pass reads.  keys == nullptr: the first pass of the step's sort -- the ids themselves, clamped as k_rows_claim /
// k_tr_score_bwd clamp them (outside [0, E): row 0), value = the entry index.  vals == nullptr with keys: a keys-only sort.
struct OrdSrc {
  const int32_t* keys;
  const int32_t* vals;
  const int64_t* e1;        // [n - BL]
  const int32_t* lookup;    // [BL]
  int64_t BL, E;
};
__device__ __forceinline__ int32_t ord_key(const OrdSrc& s, int64_t i) {
  if (s.keys) {
    const int32_t k = s.keys[i];
    return (k < 0 || (int64_t)k >= s.E) ? 0 : k;      // (a listed id lies inside [0, E): the clamp keeps the digits inside the passes)
  }
  const int64_t r = i < s.BL ? (int64_t)s.lookup[i] : s.e1[i - s.BL];
  return (r < 0 || r >= s.E) ? 0 : (int32_t)r;
}
// the entries of this launch: the host's bound, or what the device-side count says where it is smaller
__device__ __forceinline__ int64_t ord_n(const int32_t* n_dev, int64_t n_host) {
  if (!n_dev) return n_host;
  const int64_t n = *n_dev;
  return n < n_host ? (n < 0 ? 0 : n) : n_host;
}

// hist[digit * tiles + tile] = the tile's entries with that digit
__global__ __launch_bounds__(256) void k_ord_hist(OrdSrc src, const int32_t* __restrict__ n_dev, int64_t n_host, int shift,
                                                  int32_t* __restrict__ hist) {
  __shared__ int cnt[256];
  const int64_t n = ord_n(n_dev, n_host);
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * ORD_TILE;
#pragma unroll
  for (int r = 0; r < ORD_ROUNDS; ++r) {
    const int64_t i = base + r * 256 + threadIdx.x;
    if (i < n) atomicAdd(&cnt[(ord_key(src, i) >> shift) & 255], 1);
  }
  __syncthreads();
  hist[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = cnt[threadIdx.x];
}

// scan[digit][tile] = the exclusive scan of hist over the flattened [digit][tile] order.  A workgroup per digit: the sum of every row
// in front of its own (coalesced, independent loads: 64 K words at 512 x 1001 entries, from L2), then its row 256 tiles at a time
// (shuffles inside a wave, the four wave totals through LDS).  (One workgroup over the whole array, a contiguous stretch per thread,
// took 103 us per pass: two dependent round trips per word.)
__global__ __launch_bounds__(256) void k_ord_scan(const int32_t* __restrict__ hist, int tiles, int32_t* __restrict__ scan) {
  __shared__ int red[256];
  __shared__ int wtot[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * tiles;
  int a = 0;      // (integers: any order; eight loads in flight per thread -- one at a time the loop is 251 round trips at 512 x 1001)
  int64_t i = threadIdx.x;
  for (; i + 7 * 256 < row; i += 8 * 256) {
    int v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = hist[i + u * 256];
#pragma unroll
    for (int u = 0; u < 8; ++u) a += v[u];
  }
  for (; i < row; i += 256) a += hist[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  int run = red[0];
  for (int t0 = 0; t0 < tiles; t0 += 256) {
    const int t = t0 + threadIdx.x;
    const int v = t < tiles ? hist[row + t] : 0;
    int x = v;      // inclusive over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) wtot[w] = x;
    __syncthreads();
    int before = run + x - v;
    for (int q = 0; q < w; ++q) before += wtot[q];
    if (t < tiles) scan[row + t] = before;
    run += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
  }
}

// the lanes of the wave that hold the same 8-bit digit (among the active ones): eight ballots
__device__ __forceinline__ unsigned long long ord_match8(int digit, bool active) {
  unsigned long long m = __ballot(active);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const unsigned long long v = __ballot(active && ((digit >> b) & 1));
    m &= ((digit >> b) & 1) ? v : ~v;
  }
  return m;
}

// entry i of the tile goes to scan[digit][tile] + its rank among the tile's entries of that digit in ascending i: the entries of the
// rounds before (run), of the waves before in this round (wcnt), of the lanes below in this wave (ballots)
__global__ __launch_bounds__(256) void k_ord_scatter(OrdSrc src, const int32_t* __restrict__ n_dev, int64_t n_host, int shift,
                                                     const int32_t* __restrict__ scan, int32_t* __restrict__ keys_out,
                                                     int32_t* __restrict__ vals_out) {
  __shared__ int run[256];
  __shared__ int wcnt[4][256];
  const int64_t n = ord_n(n_dev, n_host);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  run[threadIdx.x] = scan[(int64_t)threadIdx.x * gridDim.x + blockIdx.x];
  const int64_t base = (int64_t)blockIdx.x * ORD_TILE;
  for (int r = 0; r < ORD_ROUNDS; ++r) {
    if (base + r * 256 >= n) break;      // (uniform)
#pragma unroll
    for (int q = 0; q < 4; ++q) wcnt[q][threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = base + r * 256 + threadIdx.x;
    const bool active = i < n;
    int32_t key = 0, val = 0;
    if (active) {
      key = ord_key(src, i);
      val = src.keys ? (src.vals ? src.vals[i] : 0) : (int32_t)i;
    }
    const int digit = (key >> shift) & 255;
    const unsigned long long same = ord_match8(digit, active);
    const int below = (int)__popcll(same & ((1ull << lane) - 1ull));
    if (active && below == 0) wcnt[w][digit] = (int)__popcll(same);      // (the lowest lane of each digit group)
    __syncthreads();
    if (active) {
      int at = run[digit] + below;
      for (int q = 0; q < w; ++q) at += wcnt[q][digit];
      keys_out[at] = key;
      if (vals_out) vals_out[at] = val;
    }
    __syncthreads();
    run[threadIdx.x] += wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
    __syncthreads();
  }
}

// ---- segment heads.  Entry i of the sorted keys is a head when i == 0 or its key differs from the one before.
// tile_heads[tile] = the heads among the tile's entries
__global__ __launch_bounds__(256) void k_ord_head_count(const int32_t* __restrict__ keys, int64_t n, int32_t* __restrict__ tile_heads) {
  __shared__ int part[4];
  const int64_t base = (int64_t)blockIdx.x * ORD_TILE;
  int c = 0;
#pragma unroll
  for (int r = 0; r < ORD_ROUNDS; ++r) {
    const int64_t i = base + r * 256 + threadIdx.x;
    if (i < n && (i == 0 || keys[i] != keys[i - 1])) ++c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_heads[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}
// list[p] = the p-th unique id (ascending), seg[p] = where its segment starts, seg[count] = n, *count = the unique ids; claim (may be
// null): the bit of every listed row set (k_rows_rezero and k_rows_import read it)
__global__ __launch_bounds__(256) void k_ord_heads(const int32_t* __restrict__ keys, int64_t n, const int32_t* __restrict__ tile_heads,
                                                   int32_t* __restrict__ list, int32_t* __restrict__ seg, int32_t* __restrict__ count,
                                                   unsigned* __restrict__ claim) {
  __shared__ int red[256];
  __shared__ int wsum[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int a = 0;
  for (int t = threadIdx.x; t < (int)blockIdx.x; t += 256) a += tile_heads[t];      // (integers: any order)
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  int at = red[0];      // heads in front of this tile
  const int64_t base = (int64_t)blockIdx.x * ORD_TILE;
  for (int r = 0; r < ORD_ROUNDS; ++r) {
    if (base + r * 256 >= n) break;      // (uniform)
    const int64_t i = base + r * 256 + threadIdx.x;
    int32_t key = 0;
    bool head = false;
    if (i < n) {
      key = keys[i];
      head = i == 0 || key != keys[i - 1];
    }
    const unsigned long long hm = __ballot(head);
    if (lane == 0) wsum[w] = (int)__popcll(hm);
    __syncthreads();
    int p = at + (int)__popcll(hm & ((1ull << lane) - 1ull));      // heads in front of entry i
    for (int q = 0; q < w; ++q) p += wsum[q];
    if (head) {
      list[p] = key;
      seg[p] = (int32_t)i;
      if (claim) atomicOr(claim + (key >> 5), 1u << (key & 31));
    }
    if (i == n - 1) {      // the last entry closes the last segment
      const int total = p + (head ? 1 : 0);
      seg[total] = (int32_t)n;
      *count = total;
    }
    at += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
}

// ---- ordered segment reduce: a wave per segment (grid-stride over the segments: a row's sum does not depend on which wave forms it).
// dE / dbias hold rows [row_lo, row_lo + row_n) of the table (the whole table: 0, num_ent; a shard: DESIGN 6.8): a segment whose row
// lies outside is skipped whole.
//   dE[row][k] = fmaf(ds[e], h[b(e)][k], acc) over the segment's lookup entries e = b L + l in ascending e, acc from 0.f;
//   dbias[row] = acc + ds[e] the same way.  Entries >= BL (the e1 ids) end the segment and add nothing.
// Sixty-four entries' indices and ds are fetched by the lanes together and handed round by shuffles; eight rows of h are in flight
// per lane.  vec: d % 4 == 0, h and dE 16-byte aligned -- 16-byte accesses; otherwise element by element, the same chain per element.
template <bool VEC>
__device__ __forceinline__ void ord_reduce_segment(const int32_t* __restrict__ vals, int lo, int hi, const float* __restrict__ ds,
                                                   const float* __restrict__ hv, int64_t L, int64_t BL, int d, int lane,
                                                   float* __restrict__ dE_row, float* __restrict__ dbias_at) {
  const int nq = VEC ? (d >> 2) : d;
  for (int q0 = 0; q0 < nq; q0 += 64) {
    const int q = q0 + lane;
    const bool on = q < nq;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float bacc = 0.f;
    for (int e0 = lo; e0 < hi; e0 += 64) {
      const int m = hi - e0 < 64 ? hi - e0 : 64;
      int32_t v = -1;
      float g = 0.f;
      if (lane < m) {
        v = vals[e0 + lane];
        if ((int64_t)v < BL) g = ds[v]; else v = -1;
      }
      const unsigned long long live = __ballot(v >= 0);
      const int cnt = (int)__popcll(live);      // (the live entries are the first cnt: the e1 entries sort behind them)
      int u = 0;
      for (; u + 8 <= cnt; u += 8) {
        float gg[8];
        float4 hh[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int64_t b = (int64_t)__shfl(v, u + j, 64) / L;
          gg[j] = __shfl(g, u + j, 64);
          if (on) {
            if (VEC) hh[j] = ((const float4*)(hv + b * d))[q];
            else hh[j].x = hv[b * d + q];
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (on) {
            acc.x = fmaf(gg[j], hh[j].x, acc.x);
            if (VEC) { acc.y = fmaf(gg[j], hh[j].y, acc.y); acc.z = fmaf(gg[j], hh[j].z, acc.z); acc.w = fmaf(gg[j], hh[j].w, acc.w); }
          }
          bacc = fmaf(gg[j], 1.f, bacc);
        }
      }
      for (; u < cnt; ++u) {
        const int64_t b = (int64_t)__shfl(v, u, 64) / L;
        const float gg = __shfl(g, u, 64);
        if (on) {
          if (VEC) {
            const float4 hh = ((const float4*)(hv + b * d))[q];
            acc.x = fmaf(gg, hh.x, acc.x); acc.y = fmaf(gg, hh.y, acc.y); acc.z = fmaf(gg, hh.z, acc.z); acc.w = fmaf(gg, hh.w, acc.w);
          } else
            acc.x = fmaf(gg, hv[b * d + q], acc.x);
        }
        bacc = fmaf(gg, 1.f, bacc);
      }
      if (cnt < m) break;      // (uniform: the rest of the segment is e1 entries)
    }
    if (on) {
      if (VEC) ((float4*)dE_row)[q] = acc;
      else dE_row[q] = acc.x;
    }
    if (q0 == 0 && lane == 0) *dbias_at = bacc;
  }
}
__global__ __launch_bounds__(256) void k_ord_reduce(const int32_t* __restrict__ list, const int32_t* __restrict__ seg,
                                                    const int32_t* __restrict__ count, const int32_t* __restrict__ vals,
                                                    const float* __restrict__ ds, const float* __restrict__ hv, int64_t L, int64_t BL, int d,
                                                    int vec, int64_t row_lo, int64_t row_n, float* __restrict__ dE,
                                                    float* __restrict__ dbias) {
  const int n = *count, lane = threadIdx.x & 63;
  for (int s = blockIdx.x * 4 + (threadIdx.x >> 6); s < n; s += gridDim.x * 4) {
    const int64_t row = (int64_t)list[s] - row_lo;
    if (row < 0 || row >= row_n) continue;      // (wave-uniform: a segment of another shard -- nothing of it is read)
    const int lo = seg[s], hi = seg[s + 1];
    if (vec) ord_reduce_segment<true>(vals, lo, hi, ds, hv, L, BL, d, lane, dE + row * d, dbias + row);
    else ord_reduce_segment<false>(vals, lo, hi, ds, hv, L, BL, d, lane, dE + row * d, dbias + row);
  }
}

// ---- the ordered norm of the listed rows (the second form of k_rows_sumsq): workgroup i STORES the squares of list positions
// [i ORD_SUMSQ_ROWS, (i + 1) ORD_SUMSQ_ROWS) at slab[i] (0 behind the list's end) -- wave w the positions w, w + 4, ... of the stretch
// one after the other, its lanes' sums through a butterfly, the four waves in index order.  k_tr_fold_det adds the partials in its fixed
// order; a partial behind the list's end is an exact 0, so neither the grid nor the list's capacity reaches the sum.
__global__ __launch_bounds__(256) void k_rows_sumsq_ord(RowTables t, const int32_t* __restrict__ list, const int32_t* __restrict__ count,
                                                        double* __restrict__ slab) {
  __shared__ double part[4];
  const int n = *count, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t lo = (int64_t)blockIdx.x * ORD_SUMSQ_ROWS;
  double a = 0.0;
  for (int64_t i = lo + w; i < lo + ORD_SUMSQ_ROWS && i < n; i += 4) {
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
  if (threadIdx.x == 0) slab[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

}  // namespace
}  // namespace coper
