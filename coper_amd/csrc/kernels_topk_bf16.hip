// Pruned top-k of the filtered rows (coper_rank_counts with 0 < k <= 128): the logits are never materialised, also
// not for the top-k.  Kernels of the bf16x3 mode; the fp32-exact mode shares the threshold and selection kernels
// (launch_topk_pruned_f32; its block maxima and VALU rescoring live in kernels_score.hip).
//
// The per-shard top-k is what the entity-sharded ranker exchanges (the masked row of
// metrics.py:44-46 is the thing it is the top of).  At 1.25 M entities per shard a [B, |E_shard|] logit
// matrix is 20 GB per 4096 queries, so the selection works on block maxima instead:
//
//   1. the count pass itself (k_score_count_bf16x3<.., GM>) writes, next to the rank counters, the largest logit
//      of every (32-entity block, query): gmax[block][query], 1/32 of the logits, coalesced 128-B rows;
//   2. k_topk_threshold_emit: per query, the m-th largest block maximum tau, m = k + (filter entries of the
//      query), by radix select on the float bits.  m distinct blocks have their maximum >= tau and at most
//      `filter entries` of those maxima are masked, so at least k unmasked logits >= tau exist: every entity of
//      the row's top-k sits in a block whose maximum is >= tau.  Exactly m blocks are emitted (all above tau, and
//      the lowest-numbered ones equal to tau), so the candidate list has a fixed place k*q + indptr[q] and no
//      size exchange with the host is needed;
//   3. the candidate slots are grouped by entity block (k_topk_blk_scan / k_topk_blk_scatter, device-side counters)
//      and k_topk_score_blocks re-computes 32 logits x 32 slots per wave with the instruction sequence of every
//      other bf16x3 kernel (bit-identical values), masking the known answers except the target;
//   4. k_topk_select_cand, one wave per query: candidates >= tau are compacted into LDS and placed by counting the
//      survivors ahead of each, (score desc, id asc).
//
// Work beyond the count pass: (k*B + nnz) blocks of 32 logits instead of B*|E|.
#include "bf16x3_chain.h"
#include "coper_internal.h"

namespace coper {

// order-preserving map float -> uint32
__device__ __forceinline__ uint32_t tk_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

#ifndef COPER_TK_DEPTH
#define COPER_TK_DEPTH 4
#endif
constexpr int TK_DEPTH = COPER_TK_DEPTH;   // 16-byte loads a thread keeps in flight per batch (two batches overlap).  Measured on
// the 10M-entity table (threshold kernel, 4,096 queries): 4 -> 3.49 ms, 2 -> 3.60, 8 -> 4.03, 16 -> 4.60

// One sweep of a thread's share of the block axis: gmax[block][query] read as float4 (4 queries of one block), TK_DEPTH
// loads per batch and the next batch in flight while the current one is consumed (the sweeps are latency-bound).
template <typename F>
__device__ __forceinline__ void tk_sweep(const float4* __restrict__ col, int64_t qs4, int64_t g_lo, int64_t g_hi, F&& f) {
  constexpr int D = TK_DEPTH;
  int64_t g = g_lo;
  if (g + D <= g_hi) {
    float4 cur[D];
#pragma unroll
    for (int u = 0; u < D; ++u) cur[u] = col[(g + u) * qs4];
    for (; g + 2 * D <= g_hi; g += D) {
      float4 nxt[D];
#pragma unroll
      for (int u = 0; u < D; ++u) nxt[u] = col[(g + D + u) * qs4];
#pragma unroll
      for (int u = 0; u < D; ++u) f(g + u, cur[u]);
#pragma unroll
      for (int u = 0; u < D; ++u) cur[u] = nxt[u];
    }
#pragma unroll
    for (int u = 0; u < D; ++u) f(g + u, cur[u]);
    g += D;
  }
  for (; g < g_hi; ++g) f(g, col[g * qs4]);
}

// The same, for the blocks g = first, first + step, ...: at any moment the threads of a workgroup -- and the workgroups of
// the other strips, which move through the block axis at the same pace -- read neighbouring rows of gmax.  For the sweeps
// whose result does not depend on the visiting order: histograms, and the fast path's emission (slots by counter, ties by id).
template <typename F>
__device__ __forceinline__ void tk_sweep_strided(const float4* __restrict__ col, int64_t qs4, int64_t first, int64_t step, int64_t G, F&& f) {
  constexpr int D = TK_DEPTH;
  int64_t g = first;
  if (g + (D - 1) * step < G) {
    float4 cur[D];
#pragma unroll
    for (int u = 0; u < D; ++u) cur[u] = col[(g + u * step) * qs4];
    for (; g + (2 * D - 1) * step < G; g += D * step) {
      float4 nxt[D];
#pragma unroll
      for (int u = 0; u < D; ++u) nxt[u] = col[(g + (D + u) * step) * qs4];
#pragma unroll
      for (int u = 0; u < D; ++u) f(g + u * step, cur[u]);
#pragma unroll
      for (int u = 0; u < D; ++u) cur[u] = nxt[u];
    }
#pragma unroll
    for (int u = 0; u < D; ++u) f(g + u * step, cur[u]);
    g += D * step;
  }
  for (; g < G; g += step) f(g, col[g * qs4]);
}

constexpr int TK_BIN = 64;   // block maxima per query that may share the threshold's upper 16 bits on the fast path
// Round 5 -- the coarse seed (long block axes: the 10M-entity table and its shards).  The three sweeps above read every block
// maximum three times (2.56 GB each for 4,096 queries against 10 M entities).  Instead: ONE sweep that only keeps the largest key
// of every TK_GRP consecutive visits of a thread (1/16 of the data, written to `coarse`), an exact radix select of the m-th
// largest COARSE key tau_c on that level (four passes over 1/16), and then only the groups whose coarse key reaches tau_c are
// read again: the m-th largest maximum tau is >= tau_c (the m largest coarse keys are m maxima >= tau_c), so every block with a
// maximum >= tau lies in such a group -- about m groups per query.  Their maxima >= tau_c go to an LDS list (TK_CL entries per
// query) that is ranked (key desc, block asc) exactly as the bin list of the fast path is; a list that overflows (queries with
// hundreds of known answers: m = k + their number) sends the strip down the three-sweep route.
constexpr int TK_CL = 128;   // candidate-list entries per query on the coarse route (>= TK_BIN: the two routes share the lists)

// Threshold + candidate blocks of a strip of NQS = 4 * QV queries (QV = 8: 32 queries; QV = 4: 16).
// thread = (sub-range of the block axis, 4 queries); HCOPY histogram copies (sub-range % HCOPY) thin out same-bank
// LDS atomics.  A strip takes the first of three routes that finishes it (k_topk_threshold_emit):
//   coarse   (long block axes, see above) one sweep, a select on the coarse level, a ranked list;
//   fast     three sweeps: 1, 2 radix-select the upper 16 bits of the m-th largest (two 8-bit digits); 3: blocks above that
//            16-bit bin are candidates (slot by an LDS counter), blocks inside it go to a short LDS list; the list is ranked in
//            LDS ((key desc, block asc): exact ties go to the lowest-numbered blocks) and its first `rem` entries complete the
//            m candidates;
//   general  a bin with more than TK_BIN blocks (heavy ties, clustered maxima): two more radix digits, a counting sweep and
//            an ordered emission sweep, rewriting the strip's slots.
#ifdef COPER_DBG_TK_OVER
// diagnostic build: strips that left the fast path (a query of the strip has more than TK_BIN maxima in its threshold bin)
__device__ int g_tk_over;
extern "C" __attribute__((visibility("default"))) int coper_dbg_tk_over() {
  int v = -1, z = 0;
  if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_tk_over), sizeof v) != hipSuccess) return -1;
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_tk_over), &z, sizeof z);
  return v;
}
#endif

// A thread's walk over the coarse keys it wrote (TK_GRP): eight 16-byte loads in flight per batch -- the walk is a handful of
// groups per thread (10 on a 1.25 M-row shard, 77 on the 10M table), one load at a time it was a round trip per group and pass.
template <typename F>
__device__ __forceinline__ void tk_coarse_walk(const uint4* __restrict__ my, int64_t n_grp, F&& f) {
  constexpr int D = 8;
  int64_t jg = 0;
  for (; jg + D <= n_grp; jg += D) {
    uint4 v[D];
#pragma unroll
    for (int u = 0; u < D; ++u) v[u] = my[(jg + u) * TK_THREADS];
#pragma unroll
    for (int u = 0; u < D; ++u) f(jg + u, v[u]);
  }
  if (jg < n_grp) {
    uint4 v[D];
#pragma unroll
    for (int u = 0; u < D; ++u) v[u] = my[(jg + u < n_grp ? jg + u : n_grp - 1) * TK_THREADS];
#pragma unroll
    for (int u = 0; u < D; ++u)
      if (jg + u < n_grp) f(jg + u, v[u]);
  }
}

// The strip's dynamic LDS: the kernel's views are its members, the launch asks for its size.
template <int QV, int HCOPY>
struct TkLds {
  static constexpr int NQS = tk_strip_queries(QV), SUB = tk_sub_ranges(QV);
  uint32_t hist[HCOPY * 256 * NQS];           // [HCOPY][256 digits][NQS]
  uint32_t prefix[NQS], rem[NQS];             // digits of the m-th largest key found so far, its rank among the keys that share them
  uint32_t slot[NQS], bn[NQS];                // fast path: candidates emitted so far; entries of the query's list
  uint32_t cgt[SUB * NQS], ceq[SUB * NQS];    // [SUB][NQS]   (general route)
  uint32_t bkey[NQS * TK_CL];                 // [NQS][TK_CL]   (fast path: TK_BIN of them)
  int32_t bg[NQS * TK_CL];                    // [NQS][TK_CL]
};
template <int QV, int HCOPY>
constexpr size_t tk_emit_lds() { return sizeof(TkLds<QV, HCOPY>); }

// What the phases of a strip share: its LDS, the launch's arguments, and the thread's place in the strip.
template <int QV, int HCOPY>
struct TkStrip {
  static constexpr int NQS = tk_strip_queries(QV), SUB = tk_sub_ranges(QV);
  TkLds<QV, HCOPY>& lds;
  uint32_t* myhist;              // this thread's histogram copy, at its four queries
  // the launch
  int64_t G, q0, Bc;
  int k;
  const int64_t* __restrict__ indptr;
  int32_t *__restrict__ cand_blk, *__restrict__ cand_q;
  uint32_t* __restrict__ cand_tau;
  // the thread: queries 4 qv .. 4 qv + 3 of the strip, sub-range sr of the block axis
  int qv, sr;
  int64_t strip, qs0;            // qs0: first query of the strip within the chunk
  const float4* __restrict__ col;   // + g * qs4: the four queries' maxima of block g
  int64_t qs4, g_lo, g_hi;       // [g_lo, g_hi): the thread's share of the sweeps that go in block order
  bool valid[4];
  int64_t off[4], slots[4];      // the queries' slot ranges in cand_blk / cand_q

  __device__ __forceinline__ TkStrip(TkLds<QV, HCOPY>& L, const float* __restrict__ gmax, int64_t G_, int64_t Qs, int64_t q0_, int64_t Bc_, int k_,
                                     const int64_t* __restrict__ indptr_, int32_t* __restrict__ cand_blk_, int32_t* __restrict__ cand_q_,
                                     uint32_t* __restrict__ cand_tau_, int pair_xcd)
      : lds(L), G(G_), q0(q0_), Bc(Bc_), k(k_), indptr(indptr_), cand_blk(cand_blk_), cand_q(cand_q_), cand_tau(cand_tau_) {
    qv = threadIdx.x % QV; sr = threadIdx.x / QV;
    myhist = L.hist + (sr % HCOPY) * 256 * NQS + 4 * qv;
    // 16-query strips are 64 B of a 128-B line of gmax: the two strips of a line go to workgroups 8 apart, i.e. to the same
    // XCD (workgroup w runs on XCD w % 8) -- one L2 then fetches the line once, where neighbouring workgroups (two XCDs)
    // fetched it twice
    strip = blockIdx.x;
    if (QV == 4 && pair_xcd && (gridDim.x & 15) == 0) strip = (((int64_t)blockIdx.x >> 4) * 8 + (blockIdx.x & 7)) * 2 + ((blockIdx.x >> 3) & 1);
    qs0 = strip * NQS;
    const int64_t gs = (G + SUB - 1) / SUB;
    g_lo = sr * gs < G ? sr * gs : G;
    g_hi = g_lo + gs < G ? g_lo + gs : G;
    col = (const float4*)(gmax + qs0) + qv;
    qs4 = Qs >> 2;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t ql = qs0 + 4 * qv + c;
      valid[c] = ql < Bc;
      off[c] = slots[c] = 0;
      if (valid[c]) {
        const int64_t qg = q0 + ql;
        const int64_t beg = indptr[qg] - indptr[0];
        off[c] = (int64_t)k * qg + beg;
        slots[c] = (int64_t)k + (indptr[qg + 1] - indptr[0] - beg);
      }
    }
  }
};

// Every query starts as "the m-th largest of all keys", m = k + its filter entries, clamped to the number of blocks; no
// candidate emitted, the lists empty.
template <int QV, int HCOPY>
__device__ __forceinline__ void tk_strip_reset(const TkStrip<QV, HCOPY>& st) {
  if (threadIdx.x < st.NQS) {
    const int64_t ql = st.qs0 + threadIdx.x;
    int64_t m64 = 0;
    if (ql < st.Bc) {
      m64 = (int64_t)st.k + (st.indptr[st.q0 + ql + 1] - st.indptr[st.q0 + ql]);
      if (m64 > st.G) m64 = st.G;
    }
    st.lds.prefix[threadIdx.x] = 0;
    st.lds.rem[threadIdx.x] = (uint32_t)m64;
    st.lds.slot[threadIdx.x] = 0;
    st.lds.bn[threadIdx.x] = 0;
  }
}

// From the histogram of one radix digit (complete: the caller's sweep has ended) the digit of the rem-th largest among the keys
// that share the prefix; prefix and rem move on to the next pass.
template <int QV, int HCOPY>
__device__ __forceinline__ void tk_pick_digit(const TkStrip<QV, HCOPY>& st, int shift) {
  __syncthreads();
  if (threadIdx.x < st.NQS) {
    const int qi = threadIdx.x;
    const uint32_t rem = st.lds.rem[qi];
    if (rem > 0) {
      uint32_t cum = 0;
      int dg = 255;
      for (; dg > 0; --dg) {
        uint32_t cnt = 0;
#pragma unroll
        for (int hc = 0; hc < HCOPY; ++hc) cnt += st.lds.hist[(hc * 256 + dg) * st.NQS + qi];
        if (cum + cnt >= rem) break;
        cum += cnt;
      }
      st.lds.prefix[qi] |= (uint32_t)dg << shift;
      st.lds.rem[qi] = rem - cum;
    }
  }
  __syncthreads();
}

// One 8-bit digit of the m-th largest block maximum: a histogram sweep over the keys that share the digits found so far.
template <int QV, int HCOPY>
__device__ __forceinline__ void tk_radix_pass(const TkStrip<QV, HCOPY>& st, int pass) {
  const int shift = 24 - 8 * pass;
  const uint32_t mask = pass ? ~0u << (32 - 8 * pass) : 0u;   // the digits found so far
  for (int j = threadIdx.x; j < HCOPY * 256 * st.NQS; j += TK_THREADS) st.lds.hist[j] = 0;
  __syncthreads();
  uint32_t prefix[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) prefix[c] = st.lds.prefix[4 * st.qv + c];
  // block maxima cluster: consecutive values of a query mostly share the digit (in the first pass -- sign and the upper
  // exponent bits -- nearly all of them), so a thread counts runs in registers and adds a run at once; one LDS atomic per
  // value on a handful of addresses was what the sweep spent its time on
  uint32_t run_d[4] = {0, 0, 0, 0}, run_n[4] = {0, 0, 0, 0};
  tk_sweep_strided(st.col, st.qs4, (int64_t)st.sr, (int64_t)st.SUB, st.G, [&](int64_t, const float4& v4) {
    const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint32_t key = tk_key(vv[c]);
      if ((key & mask) == prefix[c]) {
        const uint32_t dgt = (key >> shift) & 255;
        if (dgt != run_d[c]) {
          if (run_n[c]) atomicAdd(&st.myhist[run_d[c] * st.NQS + c], run_n[c]);
          run_d[c] = dgt;
          run_n[c] = 0;
        }
        ++run_n[c];
      }
    }
  });
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (run_n[c]) atomicAdd(&st.myhist[run_d[c] * st.NQS + c], run_n[c]);
  tk_pick_digit(st, shift);
}

// Ranks the queries' LDS lists (STRIDE entries each, lds.bn of them used) by (key desc, block asc) and writes the first `want`
// entries of each to the candidate slots from `base` on.  whole: the list holds every block that can be a candidate (coarse
// route): base 0, want m; otherwise it is the threshold bin's (fast path): lds.slot candidates precede it, lds.rem are wanted.
// The entry that completes the m candidates carries tau, what the selection may discard unseen: logits below tau, when tau is
// a real m-th largest (at least k unmasked logits >= tau exist then); with every block a candidate (m clamped to G) or a -inf
// tau nothing is discarded.
template <int STRIDE, int QV, int HCOPY>
__device__ __forceinline__ void tk_rank_list(const TkStrip<QV, HCOPY>& st, bool whole) {
  const uint32_t kinf = tk_key(-INFINITY);
  for (int t = threadIdx.x; t < st.NQS * STRIDE; t += TK_THREADS) {
    const int qi = t / STRIDE, e = t % STRIDE;
    const int64_t ql = st.qs0 + qi;
    const uint32_t nb = st.lds.bn[qi];
    if (ql >= st.Bc || (uint32_t)e >= nb) continue;
    const int64_t qg = st.q0 + ql;
    const int64_t beg = st.indptr[qg] - st.indptr[0];
    const int64_t nslots = (int64_t)st.k + (st.indptr[qg + 1] - st.indptr[0] - beg);
    const uint32_t base = whole ? 0u : st.lds.slot[qi];
    const uint32_t want = whole ? (uint32_t)(nslots < st.G ? nslots : st.G) : st.lds.rem[qi];
    const uint32_t key = st.lds.bkey[qi * STRIDE + e];
    const int32_t g = st.lds.bg[qi * STRIDE + e];
    uint32_t ahead = 0;
    for (uint32_t t2 = 0; t2 < nb; ++t2) {
      const uint32_t k2 = st.lds.bkey[qi * STRIDE + t2];
      ahead += (k2 > key || (k2 == key && st.lds.bg[qi * STRIDE + t2] < g)) ? 1u : 0u;
    }
    if (ahead >= want) continue;
    const int64_t o = (int64_t)st.k * qg + beg;
    st.cand_blk[o + base + ahead] = key > kinf ? g : -1;   // blocks whose maximum is -inf hold nothing: their slots stay unused
    if (ahead == want - 1) st.cand_tau[qg] = (nslots <= st.G && key > kinf) ? key : 0u;
  }
}

// Query ids of all slots of the thread's query c; slots past the `used` candidates are unused.
template <int QV, int HCOPY>
__device__ __forceinline__ void tk_fill_slots(const TkStrip<QV, HCOPY>& st, int c, int64_t used) {
  if (!st.valid[c]) return;
  for (int64_t j = st.sr; j < st.slots[c]; j += st.SUB) {
    st.cand_q[st.off[c] + j] = (int32_t)(st.q0 + st.qs0 + 4 * st.qv + c);
    if (j >= used) st.cand_blk[st.off[c] + j] = -1;
  }
}

// Candidates are scored block by block: how many slots want block g (nseg counters per block thin out the same-address
// atomics when there are few blocks).
template <int QV, int HCOPY>
__device__ __forceinline__ void tk_count_blocks(const TkStrip<QV, HCOPY>& st, int32_t* __restrict__ blk_cnt, int nseg) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (!st.valid[c] || !blk_cnt) continue;      // (blk_cnt == NULL: 64-entity candidates, counted after their expansion: k_topk_expand64)
    for (int64_t j = st.sr; j < st.slots[c]; j += st.SUB) {
      const int32_t g = st.cand_blk[st.off[c] + j];
      if (g >= 0) atomicAdd(&blk_cnt[(int64_t)g * nseg + ((st.off[c] + j) & (nseg - 1))], 1);
    }
  }
}

// ---- the coarse route (see TK_CL above).  false: a list overflowed, and the strip is reset for the three-sweep route.
template <int QV, int HCOPY>
__device__ __forceinline__ bool tk_route_coarse(const TkStrip<QV, HCOPY>& st, uint4* __restrict__ coarse, int64_t NG) {
  const int qv = st.qv, sr = st.sr;
  const int64_t G = st.G;
  uint4* my = coarse + ((int64_t)st.strip * NG) * TK_THREADS + threadIdx.x;      // my group jg: my[jg * TK_THREADS]
  const int64_t n_vis = (int64_t)sr < G ? (G - sr + st.SUB - 1) / st.SUB : 0;     // my visits: blocks sr, sr + SUB, ...
  const int64_t n_grp = (n_vis + TK_GRP - 1) / TK_GRP;
  {   // sweep 1: the largest key of every TK_GRP visits
    uint32_t gm[4] = {0u, 0u, 0u, 0u};
    int64_t gj = 0;
    tk_sweep_strided(st.col, st.qs4, (int64_t)st.sr, (int64_t)st.SUB, st.G, [&](int64_t g, const float4& v4) {
      const int64_t jg = ((g - sr) / st.SUB) / TK_GRP;
      if (jg != gj) { my[gj * TK_THREADS] = make_uint4(gm[0], gm[1], gm[2], gm[3]); gm[0] = gm[1] = gm[2] = gm[3] = 0u; gj = jg; }
      const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) { const uint32_t key = tk_key(vv[c]); gm[c] = key > gm[c] ? key : gm[c]; }
    });
    if (n_vis > 0) my[gj * TK_THREADS] = make_uint4(gm[0], gm[1], gm[2], gm[3]);
  }
  // the m-th largest coarse key of every query: four radix digits over the keys this thread wrote itself
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const uint32_t cmask = pass ? ~0u << (32 - 8 * pass) : 0u;
    for (int j = threadIdx.x; j < HCOPY * 256 * st.NQS; j += TK_THREADS) st.lds.hist[j] = 0;
    __syncthreads();
    uint32_t prefix[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) prefix[c] = st.lds.prefix[4 * qv + c];
    tk_coarse_walk(my, n_grp, [&](int64_t, const uint4& k4) {
      const uint32_t kk[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if ((kk[c] & cmask) == prefix[c]) atomicAdd(&st.myhist[((kk[c] >> shift) & 255) * st.NQS + c], 1u);
    });
    tk_pick_digit(st, shift);
  }
  // the groups that reach tau_c: their maxima >= tau_c into the query's list
  {
    uint32_t tauc[4];
    bool live[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { tauc[c] = st.lds.prefix[4 * qv + c]; live[c] = st.valid[c]; }
    tk_coarse_walk(my, n_grp, [&](int64_t jg, const uint4& k4) {
      const uint32_t kk[4] = {k4.x, k4.y, k4.z, k4.w};
      bool q_[4], any = false;
#pragma unroll
      for (int c = 0; c < 4; ++c) { q_[c] = live[c] && kk[c] >= tauc[c]; any |= q_[c]; }
      if (!any) return;
      for (int u0 = 0; u0 < TK_GRP; u0 += 8) {      // the group's maxima again, eight loads in flight
        float4 f8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int64_t g = sr + (jg * TK_GRP + u0 + u) * (int64_t)st.SUB;
          f8[u] = st.col[(g < G ? g : (int64_t)sr) * st.qs4];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int64_t g = sr + (jg * TK_GRP + u0 + u) * (int64_t)st.SUB;
          if (g >= G) continue;
          const float vv[4] = {f8[u].x, f8[u].y, f8[u].z, f8[u].w};
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if (!q_[c]) continue;
            const uint32_t key = tk_key(vv[c]);
            if (key >= tauc[c]) {
              const uint32_t i = atomicAdd(&st.lds.bn[4 * qv + c], 1u);
              if (i < (uint32_t)TK_CL) { st.lds.bkey[(4 * qv + c) * TK_CL + i] = key; st.lds.bg[(4 * qv + c) * TK_CL + i] = (int32_t)g; }
            }
          }
        }
      }
    });
  }
  __syncthreads();
  bool over = false;
  if (threadIdx.x < st.NQS) over = st.lds.bn[threadIdx.x] > (uint32_t)TK_CL;
  if (__syncthreads_or(over ? 1 : 0)) {
    tk_strip_reset(st);
    __syncthreads();
    return false;
  }
  tk_rank_list<TK_CL>(st, true);
#pragma unroll
  for (int c = 0; c < 4; ++c) tk_fill_slots(st, c, st.slots[c] < G ? st.slots[c] : G);
  return true;
}

// ---- the fast path.  false: a threshold bin holds more than TK_BIN blocks, nothing the strip wrote so far counts.
template <int QV, int HCOPY>
__device__ __forceinline__ bool tk_route_fast(const TkStrip<QV, HCOPY>& st) {
  const int qv = st.qv;
  tk_radix_pass(st, 0);
  tk_radix_pass(st, 1);
  // sweep 3: above the 16-bit bin -> candidate; inside it -> LDS list
  {
    uint32_t p16[4];
    bool live[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      p16[c] = st.lds.prefix[4 * qv + c] >> 16;
      live[c] = st.valid[c] && st.lds.rem[4 * qv + c] > 0;
    }
    tk_sweep_strided(st.col, st.qs4, (int64_t)st.sr, (int64_t)st.SUB, st.G, [&](int64_t g, const float4& v4) {
      const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (!live[c]) continue;
        const uint32_t key = tk_key(vv[c]);
        const uint32_t k16 = key >> 16;
        if (k16 > p16[c]) {
          st.cand_blk[st.off[c] + atomicAdd(&st.lds.slot[4 * qv + c], 1u)] = (int32_t)g;
        } else if (k16 == p16[c]) {
          const uint32_t i = atomicAdd(&st.lds.bn[4 * qv + c], 1u);
          if (i < (uint32_t)TK_BIN) { st.lds.bkey[(4 * qv + c) * TK_BIN + i] = key; st.lds.bg[(4 * qv + c) * TK_BIN + i] = (int32_t)g; }
        }
      }
    });
  }
  __syncthreads();
  bool over = false;
  if (threadIdx.x < st.NQS) over = st.lds.bn[threadIdx.x] > (uint32_t)TK_BIN;
  if (__syncthreads_or(over ? 1 : 0)) return false;
  tk_rank_list<TK_BIN>(st, false);
#pragma unroll
  for (int c = 0; c < 4; ++c) tk_fill_slots(st, c, (int64_t)st.lds.slot[4 * qv + c] + st.lds.rem[4 * qv + c]);
  return true;
}

// ---- the general route, after the fast path's two digits: the remaining two, then count and emit in block order
template <int QV, int HCOPY>
__device__ __forceinline__ void tk_route_general(const TkStrip<QV, HCOPY>& st) {
  const int qv = st.qv, sr = st.sr;
  const uint32_t kinf = tk_key(-INFINITY);
  tk_radix_pass(st, 2);
  tk_radix_pass(st, 3);
  uint32_t tau[4], cgt[4] = {0, 0, 0, 0}, ceq[4] = {0, 0, 0, 0};
#pragma unroll
  for (int c = 0; c < 4; ++c) tau[c] = st.lds.prefix[4 * qv + c];
  tk_sweep(st.col, st.qs4, st.g_lo, st.g_hi, [&](int64_t, const float4& v4) {
    const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint32_t key = tk_key(vv[c]);
      cgt[c] += key > tau[c] ? 1u : 0u;
      ceq[c] += key == tau[c] ? 1u : 0u;
    }
  });
#pragma unroll
  for (int c = 0; c < 4; ++c) { st.lds.cgt[sr * st.NQS + 4 * qv + c] = cgt[c]; st.lds.ceq[sr * st.NQS + 4 * qv + c] = ceq[c]; }
  __syncthreads();
  // bgt, beq: blocks above / at tau in the sub-ranges before mine; c1: blocks above tau; need: blocks at tau that are wanted
  uint32_t bgt[4], beq[4], c1[4], need[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int qi = 4 * qv + c;
    bgt[c] = beq[c] = c1[c] = 0;
    for (int s2 = 0; s2 < st.SUB; ++s2) {
      const uint32_t x = st.lds.cgt[s2 * st.NQS + qi];
      if (s2 < sr) { bgt[c] += x; beq[c] += st.lds.ceq[s2 * st.NQS + qi]; }
      c1[c] += x;
    }
    need[c] = tau[c] > kinf ? st.lds.rem[qi] : 0u;
    if (st.valid[c] && sr == 0) st.cand_tau[st.q0 + st.qs0 + qi] = (st.slots[c] <= st.G && tau[c] > kinf) ? tau[c] : 0u;
    tk_fill_slots(st, c, (int64_t)(c1[c] + need[c]));
  }
  tk_sweep(st.col, st.qs4, st.g_lo, st.g_hi, [&](int64_t g, const float4& v4) {
    const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (!st.valid[c]) continue;
      const uint32_t key = tk_key(vv[c]);
      if (key > tau[c]) {
        st.cand_blk[st.off[c] + bgt[c]++] = (int32_t)g;
      } else if (key == tau[c]) {
        if (beq[c] < need[c]) st.cand_blk[st.off[c] + c1[c] + beq[c]] = (int32_t)g;
        ++beq[c];
      }
    }
  });
}

template <int QV, int HCOPY>
__global__ __launch_bounds__(TK_THREADS) void k_topk_threshold_emit(const float* __restrict__ gmax, int64_t G, int64_t Qs, int64_t q0,
                                                                    int64_t Bc, int k, const int64_t* __restrict__ indptr,
                                                                    int32_t* __restrict__ cand_blk, int32_t* __restrict__ cand_q,
                                                                    int32_t* __restrict__ blk_cnt, int nseg,
                                                                    uint32_t* __restrict__ cand_tau, int pair_xcd,
                                                                    uint4* __restrict__ coarse, int64_t NG) {
  extern __shared__ uint32_t tk_lds[];
  const TkStrip<QV, HCOPY> st(*(TkLds<QV, HCOPY>*)tk_lds, gmax, G, Qs, q0, Bc, k, indptr, cand_blk, cand_q, cand_tau, pair_xcd);
  tk_strip_reset(st);
  bool done = coarse && tk_route_coarse(st, coarse, NG);
  if (!done) done = tk_route_fast(st);
  if (!done) {
#ifdef COPER_DBG_TK_OVER
    if (threadIdx.x == 0) atomicAdd(&g_tk_over, 1);
#endif
    tk_route_general(st);
  }
  // cand_blk is read back by other threads than the ones that wrote it
  __threadfence_block();
  __syncthreads();
  tk_count_blocks(st, blk_cnt, nseg);
}

// Large tables (topk_expand == 2): the threshold kernel worked on 64-entity block maxima; every candidate slot becomes two slots, the block's two
// 32-entity halves (2g, 2g + 1) -- what the grouping, the re-scoring and the selection below are written for.  A query's slots
// stay contiguous: [2 off, 2 (off + n)).
__global__ __launch_bounds__(256) void k_topk_expand64(const int32_t* __restrict__ blk64, const int32_t* __restrict__ q64, int64_t T64,
                                                       int32_t* __restrict__ cand_blk, int32_t* __restrict__ cand_q,
                                                       int32_t* __restrict__ blk_cnt, int nseg) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= T64) return;
  const int32_t g = blk64[j], q = q64[j];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int64_t j2 = 2 * j + u;
    cand_blk[j2] = g >= 0 ? 2 * g + u : -1;
    cand_q[j2] = q;
    if (g >= 0) atomicAdd(&blk_cnt[(int64_t)(2 * g + u) * nseg + (j2 & (nseg - 1))], 1);
  }
}


// ---- group the candidate slots by entity block: every block's slots padded to a multiple of 32 (one wave each)
// blk_off[g] = first position of block g in `sorted`, blk_off[G] = total (a multiple of 32)
__global__ __launch_bounds__(1024) void k_topk_blk_scan(const int32_t* __restrict__ blk_cnt, int64_t G, int32_t* __restrict__ blk_off) {
  __shared__ int32_t part[1024];
  const int64_t per = (G + 1023) / 1024;
  const int64_t lo_g = threadIdx.x * per, hi_g = lo_g + per < G ? lo_g + per : G;
  int32_t sum = 0;
  for (int64_t g = lo_g; g < hi_g; ++g) sum += (blk_cnt[g] + 31) & ~31;
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {   // inclusive scan
    const int32_t add = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  int32_t run = part[threadIdx.x] - sum;
  for (int64_t g = lo_g; g < hi_g; ++g) { blk_off[g] = run; run += (blk_cnt[g] + 31) & ~31; }
  if (threadIdx.x == 1023) blk_off[G] = part[1023];
}

// Long block axes (the 10M-entity table: 312,500 counters): the same exclusive scan in three coalesced launches -- chunk sums,
// a scan of the chunk sums, chunk-local scans.  The single workgroup above walks 305 counters per thread with a stride of
// 1.2 KB between lanes: 0.58 ms; these take ~0.02 ms together.
__global__ __launch_bounds__(256) void k_topk_blk_chunk_sums(const int32_t* __restrict__ blk_cnt, int64_t G, int32_t* __restrict__ chunk_sum) {
  __shared__ int32_t red[256];
  const int64_t base = (int64_t)blockIdx.x * TK_SCAN_CHUNK;
  int32_t sum = 0;
#pragma unroll
  for (int j = 0; j < TK_SCAN_CHUNK / 256; ++j) {
    const int64_t g = base + threadIdx.x + 256 * j;
    if (g < G) sum += (blk_cnt[g] + 31) & ~31;
  }
  red[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) chunk_sum[blockIdx.x] = red[0];
}

// exclusive scan of the chunk sums in place (one workgroup; any number of chunks), total -> blk_off[G]
__global__ __launch_bounds__(1024) void k_topk_blk_chunk_scan(int32_t* __restrict__ chunk_sum, int nchunk, int32_t* __restrict__ total_out) {
  __shared__ int32_t part[1024];
  __shared__ int32_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int c0 = 0; c0 < nchunk; c0 += 1024) {
    const int i = c0 + threadIdx.x;
    const int32_t v = i < nchunk ? chunk_sum[i] : 0;
    part[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      const int32_t add = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
      __syncthreads();
      part[threadIdx.x] += add;
      __syncthreads();
    }
    if (i < nchunk) chunk_sum[i] = carry + part[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry += part[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(256) void k_topk_blk_chunk_apply(const int32_t* __restrict__ blk_cnt, int64_t G, const int32_t* __restrict__ chunk_off,
                                                              int32_t* __restrict__ blk_off) {
  __shared__ int32_t v[TK_SCAN_CHUNK];
  __shared__ int32_t tsum[256];
  const int64_t base = (int64_t)blockIdx.x * TK_SCAN_CHUNK;
#pragma unroll
  for (int j = 0; j < TK_SCAN_CHUNK / 256; ++j) {
    const int64_t g = base + threadIdx.x + 256 * j;
    v[threadIdx.x + 256 * j] = g < G ? ((blk_cnt[g] + 31) & ~31) : 0;
  }
  __syncthreads();
  // thread t owns counters [16 t, 16 t + 16) of the chunk
  int32_t loc[16], s = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) { loc[j] = s; s += v[16 * threadIdx.x + j]; }
  tsum[threadIdx.x] = s;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int32_t add = (int)threadIdx.x >= o ? tsum[threadIdx.x - o] : 0;
    __syncthreads();
    tsum[threadIdx.x] += add;
    __syncthreads();
  }
  const int32_t off = chunk_off[blockIdx.x] + tsum[threadIdx.x] - s;
#pragma unroll
  for (int j = 0; j < 16; ++j) v[16 * threadIdx.x + j] = off + loc[j];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < TK_SCAN_CHUNK / 256; ++j) {
    const int64_t g = base + threadIdx.x + 256 * j;
    if (g < G) blk_off[g] = v[threadIdx.x + 256 * j];
  }
}

// blk_off[0..GV] from blk_cnt[0..GV): one workgroup for short axes, three coalesced launches for long ones (chunk sums in `tmp`)
static void tk_launch_blk_scan(const int32_t* blk_cnt, int64_t GV, int32_t* blk_off, int32_t* tmp, int64_t tmp_cap, hipStream_t s) {
  const int64_t nchunk = (GV + TK_SCAN_CHUNK - 1) / TK_SCAN_CHUNK;
  if (GV <= 4 * TK_SCAN_CHUNK || !tmp || nchunk > tmp_cap) {
    hipLaunchKernelGGL(k_topk_blk_scan, dim3(1), dim3(1024), 0, s, blk_cnt, GV, blk_off);
    return;
  }
  hipLaunchKernelGGL(k_topk_blk_chunk_sums, dim3((unsigned)nchunk), dim3(256), 0, s, blk_cnt, GV, tmp);
  hipLaunchKernelGGL(k_topk_blk_chunk_scan, dim3(1), dim3(1024), 0, s, tmp, (int)nchunk, blk_off + GV);
  hipLaunchKernelGGL(k_topk_blk_chunk_apply, dim3((unsigned)nchunk), dim3(256), 0, s, blk_cnt, GV, tmp, blk_off);
}

__global__ __launch_bounds__(256) void k_topk_blk_scatter(const int32_t* __restrict__ cand_blk, int64_t T, const int32_t* __restrict__ blk_off,
                                                          int32_t* __restrict__ blk_cur, int nseg, int32_t* __restrict__ sorted) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= T) return;
  const int32_t g = cand_blk[w];
  if (g < 0) return;
  const int64_t vb = (int64_t)g * nseg + (w & (nseg - 1));
  sorted[blk_off[vb] + atomicAdd(&blk_cur[vb], 1)] = (int32_t)w;
}

// One wave per 32 candidate slots of one entity block: A = the block's fragments (read as the count pass reads them),
// B column c = the query of slot c (gathered from the row-major planes, as the pair kernel does).  Lane (c, half)
// ends with 16 rows of its slot's 32 logits; known answers of the slot's query, except its target, become -inf.
__global__ __launch_bounds__(256) void k_topk_score_blocks(const uint4* __restrict__ Ehi, const uint4* __restrict__ Elo,
                                                           const float* __restrict__ bias_pad, const uint4* __restrict__ Hrm_hi,
                                                           const uint4* __restrict__ Hrm_lo, int KS, int half_tail, int64_t G,
                                                           const int64_t* __restrict__ e2, const int64_t* __restrict__ indptr,
                                                           const int64_t* __restrict__ idx, const int32_t* __restrict__ cand_blk,
                                                           const int32_t* __restrict__ cand_q, const int32_t* __restrict__ blk_off,
                                                           const int32_t* __restrict__ sorted, int64_t lo,
                                                           float* __restrict__ cand_val, const int32_t* __restrict__ x3s) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5, c = lane & 31;
  const int sexp = x3s[1];   // the accumulators' power of two (split16.h): candidate values stay in the units of the block maxima
  const int64_t i = (int64_t)blockIdx.x * 4 + wave;
  if (i * 32 >= blk_off[G]) return;   // G here: number of (block, segment) counters
  const int64_t g = cand_blk[sorted[i * 32]];   // the first slot of a wave's 32 is always in use
  const int32_t w = sorted[i * 32 + c];          // -1: padding
  const int64_t q = w >= 0 ? cand_q[w] : 0;
  f32x16 acc;
  {
    const float4* bp = (const float4*)(bias_pad + g * 32 + 4 * half);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 b4 = bp[2 * j];
      acc[4 * j + 0] = x3_scale(b4.x, sexp); acc[4 * j + 1] = x3_scale(b4.y, sexp);
      acc[4 * j + 2] = x3_scale(b4.z, sexp); acc[4 * j + 3] = x3_scale(b4.w, sexp);
    }
  }
  const uint4* pa_h = Ehi + g * KS * 64 + lane;
  const uint4* pa_l = Elo + g * KS * 64 + lane;
  const uint4* pb_h = Hrm_hi + q * (2 * KS) + half;
  const uint4* pb_l = Hrm_lo + q * (2 * KS) + half;
  // pairs of k-steps, then the last one of an odd count (bf16x3_chain.h); batches of two pairs
  for (int ks = 0; ks < KS; ks += 4) {
    uint4 ah[4], al[4], bh[4], bl[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = ks + u < KS ? ks + u : KS - 1;
      ah[u] = pa_h[k * 64]; al[u] = pa_l[k * 64];
      bh[u] = pb_h[k * 2]; bl[u] = pb_l[k * 2];
    }
#pragma unroll
    for (int u = 0; u < 4; u += 2) {   // wave-uniform
      if (ks + u + 1 < KS) { BX3_PAIR(ah[u], al[u], bh[u], bl[u], ah[u + 1], al[u + 1], bh[u + 1], bl[u + 1], acc); }
      else if (ks + u < KS) { BX3_LAST_BY(half_tail, ah[u], al[u], bh[u], bl[u], acc); }
    }
  }
  if (w < 0) return;
  // known answers of this lane's query inside the block, except the target (metrics.py:45-46)
  const int64_t target = e2[q];
  uint32_t masked = 0;
  for (int64_t j = indptr[q]; j < indptr[q + 1]; ++j) {
    const int64_t f = idx[j];
    const int64_t r = f - lo - g * 32;
    if (f != target && r >= 0 && r < 32) masked |= 1u << (int)r;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float4 v = make_float4(acc[4 * j + 0], acc[4 * j + 1], acc[4 * j + 2], acc[4 * j + 3]);
    const int row = 8 * j + 4 * half;
    if ((masked >> (row + 0)) & 1u) v.x = -INFINITY;
    if ((masked >> (row + 1)) & 1u) v.y = -INFINITY;
    if ((masked >> (row + 2)) & 1u) v.z = -INFINITY;
    if ((masked >> (row + 3)) & 1u) v.w = -INFINITY;
    *(float4*)(cand_val + (int64_t)w * 32 + row) = v;
  }
}

// One wave per query.  Only candidates >= tau (cand_tau, from the threshold kernel) can be in the top-k: they are
// compacted into LDS (a few dozen out of (k + filter entries) * 32) and placed by counting, for each survivor, the
// survivors ahead of it in (score desc, entity id asc) order.  More survivors than the LDS list holds (tiny entity
// sets where tau is -inf, heavy ties): k rounds of arg-max through memory instead.
constexpr int TK_SURV = 256;   // survivors per query held in LDS
__global__ __launch_bounds__(256) void k_topk_select_cand(float* __restrict__ cand_val, const int32_t* __restrict__ cand_blk,
                                                          const uint32_t* __restrict__ cand_tau, const int64_t* __restrict__ indptr,
                                                          int64_t B, int k, int64_t lo, float* __restrict__ out_val,
                                                          int64_t* __restrict__ out_idx, const int32_t* __restrict__ x3s, int xf) {
  __shared__ float s_v[4][TK_SURV];
  const int dexp = x3s ? -x3s[1] : 0;   // x3 mode: candidate values carry 2^(e_E + e_h); what is written out does not
  __shared__ int s_id[4][TK_SURV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t q = (int64_t)blockIdx.x * 4 + wave;
  if (q >= B) return;
  const int64_t beg = indptr[q] - indptr[0];
  const int64_t off = xf * ((int64_t)k * q + beg);           // (xf = 2: slots expanded from 64-entity candidates)
  const int n = xf * (int)((int64_t)k + (indptr[q + 1] - indptr[0] - beg)) * 32;
  float* val = cand_val + off * 32;
  const int32_t* blk = cand_blk + off;
  float* ov = out_val + q * k;
  int64_t* oi = out_idx + q * k;
  const uint32_t tau = cand_tau[q];
  int S = 0;   // survivors so far (wave-uniform)
  for (int j0 = 0; j0 < n; j0 += 64 * 4) {
    float v[4];
    int32_t b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + 64 * u + lane;
      b[u] = j < n ? blk[j >> 5] : -1;
      v[u] = b[u] >= 0 ? val[j] : -INFINITY;   // unused slots (block -1) hold nothing
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool keep = v[u] > -INFINITY && tk_key(v[u]) >= tau;
      const unsigned long long m = __ballot(keep);
      if (keep) {
        const int pos = S + __popcll(m & ((1ull << lane) - 1ull));
        if (pos < TK_SURV) { s_v[wave][pos] = v[u]; s_id[wave][pos] = b[u] * 32 + ((j0 + 64 * u + lane) & 31); }
      }
      S += __popcll(m);
    }
  }
  if (S <= TK_SURV) {
    __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the list is wave-local
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < S; i += 64) {
      const float v = s_v[wave][i];
      const int id = s_id[wave][i];
      int ahead = 0;
      for (int t = 0; t < S; ++t) {
        const float v2 = s_v[wave][t];
        const int i2 = s_id[wave][t];
        ahead += (v2 > v || (v2 == v && i2 < id)) ? 1 : 0;
      }
      if (ahead < k) { ov[ahead] = x3_scale(v, dexp); oi[ahead] = lo + id; }
    }
    for (int r = S + lane; r < k; r += 64) { ov[r] = -INFINITY; oi[r] = -1; }
    return;
  }
  for (int round = 0; round < k; ++round) {
    float best = -INFINITY;
    int bid = 0x7fffffff, bpos = -1;
    for (int j = lane; j < n; j += 64) {
      const int32_t b = blk[j >> 5];
      if (b < 0) continue;
      const float v = val[j];
      if (!(v > -INFINITY)) continue;
      const int id = b * 32 + (j & 31);
      if (v > best || (v == best && id < bid)) { best = v; bid = id; bpos = j; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float v2 = __shfl_xor(best, o);
      const int i2 = __shfl_xor(bid, o);
      const int p2 = __shfl_xor(bpos, o);
      if (v2 > best || (v2 == best && i2 < bid)) { best = v2; bid = i2; bpos = p2; }
    }
    // every lane holds the winner now; the lane that read it retires it (its own later reads see its own store)
    if (lane == 0) {
      ov[round] = bpos >= 0 ? x3_scale(best, dexp) : -INFINITY;
      oi[round] = bpos >= 0 ? lo + bid : -1;
    }
    if (bpos >= 0 && (bpos & 63) == lane) val[bpos] = -INFINITY;
  }
}

static bool tk_pair_xcd() {
  static const bool on = getenv("COPER_TK_NO_XCD_PAIRS") == nullptr;   // A/B switch
  return on;
}

template <int QV, int HCOPY>
static void tk_launch_emit(coper_handle* h, int64_t G, int64_t qs, int64_t q0, int64_t bc, int k, const int64_t* indptr, hipStream_t s,
                           int32_t* out_blk, int32_t* out_q, int32_t* out_cnt) {
  const size_t lds = tk_emit_lds<QV, HCOPY>();
  static uint64_t attr_done = 0;   // per instantiation, one bit per device (function attributes are per device)
  const uint64_t bit = 1ull << (h->cfg.device & 63);
  if (!(attr_done & bit)) {
    (void)hipFuncSetAttribute((const void*)k_topk_threshold_emit<QV, HCOPY>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_done |= bit;
  }
  // the coarse route (TK_GRP): long block axes, when the scratch was reserved for this (G, qs)
  static const bool no_coarse = getenv("COPER_TK_NO_COARSE") != nullptr;     // A/B switch, read once
  uint4* coarse = (!no_coarse && G >= TK_COARSE_MIN_BLOCKS && h->topk.tk_coarse_ws && tk_coarse_bytes(G, qs, QV) <= h->topk.tk_coarse_ws.size()) ? (uint4*)h->topk.tk_coarse_ws : nullptr;
  hipLaunchKernelGGL((k_topk_threshold_emit<QV, HCOPY>), dim3((unsigned)tk_strips(qs, QV)), dim3(TK_THREADS), lds, s, h->topk.gmax_ws, G, qs, q0, bc,
                     k, indptr, out_blk, out_q, out_cnt, topk_nseg(G), h->topk.cand_tau_ws, tk_pair_xcd() ? 1 : 0, coarse, tk_coarse_groups(G, QV));
}

// strip width / histogram copies of the threshold kernel by shape
static void tk_dispatch_emit(coper_handle* h, int64_t G, int64_t qs, int64_t q0, int64_t bc, int k, const int64_t* indptr, hipStream_t s,
                             int32_t* out_blk, int32_t* out_q, int32_t* out_cnt) {
  static const char* force = getenv("COPER_TK_EMIT");   // experiments: "8_1", "8_2", "4_4"
  if (force && force[0] == '8' && force[2] == '1') return tk_launch_emit<8, 1>(h, G, qs, q0, bc, k, indptr, s, out_blk, out_q, out_cnt);
  if (force && force[0] == '8' && force[2] == '2') return tk_launch_emit<8, 2>(h, G, qs, q0, bc, k, indptr, s, out_blk, out_q, out_cnt);
  if (force && force[0] == '4') return tk_launch_emit<4, 4>(h, G, qs, q0, bc, k, indptr, s, out_blk, out_q, out_cnt);
  // long block axis: more histogram copies; half-width strips (twice the workgroups) when 32-query strips would
  // not cover the chip
  if (G < 4096) tk_launch_emit<8, 1>(h, G, qs, q0, bc, k, indptr, s, out_blk, out_q, out_cnt);
  else if (qs / 32 >= h->num_cus) tk_launch_emit<8, 2>(h, G, qs, q0, bc, k, indptr, s, out_blk, out_q, out_cnt);
  else tk_launch_emit<4, 4>(h, G, qs, q0, bc, k, indptr, s, out_blk, out_q, out_cnt);
}

// ---- the workspaces of a plan: reserved here, beside the launchers that use them.  Reservation and use read one plan, so holds() is
// the only comparison a launcher makes ----
bool TopkWs::holds(const TopkPlan& p) const {
  return p.fits && p.gmax_floats <= gmax_ws.size() && (size_t)p.T <= cand_cap && p.list_len <= cand_blk_ws.size() && p.list_len <= cand_q_ws.size() &&
         p.cand_val_len <= cand_val_ws.size() && p.sorted_cap <= cand_sorted_ws.size() && p.coarse_bytes <= tk_coarse_ws.size() &&
         (size_t)p.B <= cand_tau_ws.size() && p.blk_cnt_len <= blk_cnt_ws.size() && p.blk_off_len <= blk_off_ws.size();
}

int TopkWs::ensure(coper_handle* h, const TopkPlan& p, hipStream_t s) {
  if (holds(p)) return COPER_OK;
  StreamGrow grow{h, s};
  int rc;
  if ((rc = grow(tk_coarse_ws, p.coarse_bytes, "top-k coarse level")) || (rc = grow(gmax_ws, p.gmax_floats, "block maxima"))) return rc;
  if ((size_t)p.T > cand_cap || p.list_len > cand_blk_ws.size() || p.sorted_cap > cand_sorted_ws.size()) {
    // the group of four moves together: a growth that fails part-way leaves it marked unusable, and the next call allocates it again
    if ((rc = grow.sync())) return rc;
    cand_cap = 0; cand_blk_ws.reset(); cand_q_ws.reset(); cand_val_ws.reset(); cand_sorted_ws.reset();
    if ((rc = grow(cand_blk_ws, p.list_len, "candidate blocks")) || (rc = grow(cand_q_ws, p.list_len, "candidate queries")) ||
        (rc = grow(cand_val_ws, p.cand_val_len, "candidate logits")) || (rc = grow(cand_sorted_ws, p.sorted_cap, "sorted candidates")))
      return rc;
    cand_cap = (size_t)p.T;
  }
  if ((rc = grow(cand_tau_ws, (size_t)p.B, "candidate thresholds")) || (rc = grow(blk_cnt_ws, p.blk_cnt_len, "block counts"))) return rc;
  return grow(blk_off_ws, p.blk_off_len, "block offsets");
}

// ---- the candidate pipeline, each step once ----
// reset the candidate lists; slots no query owns (filt_nnz may be a capacity larger than the CSR) must read as unused
static int tk_reset_lists(coper_handle* h, const TopkPlan& p, bool grouped, hipStream_t s) {
  TopkWs& w = h->topk;
  COPER_HIP_TRY(h, hipMemsetAsync(w.cand_blk_ws, 0xFF, sizeof(int32_t) * p.list_len, s));
  COPER_HIP_TRY(h, hipMemsetAsync(w.blk_cnt_ws, 0, sizeof(int32_t) * p.blk_cnt_len, s));          // counts | scatter cursors
  if (grouped) COPER_HIP_TRY(h, hipMemsetAsync(w.cand_sorted_ws, 0xFF, sizeof(int32_t) * p.sorted_cap, s));
  return COPER_OK;
}

// chunks of qc queries: count(q0, bc, gmax, qs) is the route's count launch, which writes the chunk's block maxima; then the threshold
// kernel emits k_blocks + (filter entries) blocks per query -- into the 64-entity level's own lists, behind the expanded ones, when XF > 1
template <typename Count>
static int tk_chunks(coper_handle* h, const TopkPlan& p, const int64_t* indptr, hipStream_t s, Count count) {
  TopkWs& w = h->topk;
  for (int64_t q0 = 0; q0 < p.B; q0 += p.qc) {
    const int64_t bc = p.B - q0 < p.qc ? p.B - q0 : p.qc;
    const int64_t qs = (bc + 127) / 128 * 128;
    if (int rc = count(q0, bc, w.gmax_ws.get(), qs)) return rc;
    if (p.XF > 1) tk_dispatch_emit(h, p.Gm, qs, q0, bc, p.k_blocks, indptr, s, w.cand_blk_ws + p.T, w.cand_q_ws + p.T, nullptr);
    else tk_dispatch_emit(h, p.G, qs, q0, bc, p.k_blocks, indptr, s, w.cand_blk_ws, w.cand_q_ws, w.blk_cnt_ws);
  }
  return COPER_OK;
}

// x3: the candidate slots grouped by entity block and re-scored; known answers except e2[q] are masked
static void tk_group_rescore(coper_handle* h, const TopkPlan& p, const int64_t* e2, const int64_t* indptr, const int64_t* idx, hipStream_t s) {
  TopkWs& w = h->topk;
  if (p.XF > 1)
    hipLaunchKernelGGL(k_topk_expand64, dim3((unsigned)((p.T64 + 255) / 256)), dim3(256), 0, s, w.cand_blk_ws + p.T, w.cand_q_ws + p.T, p.T64,
                       w.cand_blk_ws, w.cand_q_ws, w.blk_cnt_ws, p.nseg);
  tk_launch_blk_scan(w.blk_cnt_ws, p.GV, w.blk_off_ws, w.blk_off_ws + p.GV + 1, p.scan_tmp_cap, s);
  hipLaunchKernelGGL(k_topk_blk_scatter, dim3((unsigned)((p.T + 255) / 256)), dim3(256), 0, s, w.cand_blk_ws, p.T, w.blk_off_ws,
                     w.blk_cnt_ws + p.GV, p.nseg, w.cand_sorted_ws);
  const int64_t waves = (int64_t)p.sorted_cap / 32;
  hipLaunchKernelGGL(k_topk_score_blocks, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, (const uint4*)h->Ef16_hi,
                     (const uint4*)h->Ef16_lo, h->bias_pad, (const uint4*)h->hrm16_hi, (const uint4*)h->hrm16_lo, h->dm.KS16, h->dm.x3_tail == BX3_TAIL_HALF ? 1 : 0, p.GV, e2,
                     indptr, idx, w.cand_blk_ws, w.cand_q_ws, w.blk_off_ws, w.cand_sorted_ws, (int64_t)h->cfg.shard_lo,
                     w.cand_val_ws, h->x3s);
}

int launch_topk_pruned_bf16x3(coper_handle* h, PassCtx& ctx, const TopkPlan& p, const float* hvec, const float* tgt_x, const int64_t* e2,
                              const int64_t* indptr, const int64_t* idx, int32_t* ng, int32_t* ne, float* topk_val, int64_t* topk_idx, hipStream_t s) {
  int rc;
  if (!h->topk.holds(p)) return fail(h, COPER_ESTATE, "pruned top-k: workspace not reserved");
  score_count_begin_bf16x3(ctx, p.B, ng, ne, s);
  auto count = [&](int64_t q0, int64_t bc, float* gmax, int64_t qs) { return score_count3_chunk_bf16x3(h, ctx, q0, bc, hvec, tgt_x, e2, indptr, idx, ng, ne, gmax, qs, s); };
  if ((rc = tk_reset_lists(h, p, true, s)) || (rc = tk_chunks(h, p, indptr, s, count))) return rc;
  tk_group_rescore(h, p, e2, indptr, idx, s);
  hipLaunchKernelGGL(k_topk_select_cand, dim3((unsigned)((p.B + 3) / 4)), dim3(256), 0, s, h->topk.cand_val_ws, h->topk.cand_blk_ws, h->topk.cand_tau_ws,
                     indptr, p.B, p.k_blocks, (int64_t)h->cfg.shard_lo, topk_val, topk_idx, h->x3s, p.XF);
  COPER_HIP_TRY(h, hipGetLastError());
  return COPER_OK;
}

// fp32-exact mode: same threshold / selection kernels on the block maxima of k_score_count_f32; candidates are
// rescored by the VALU chain (kernels_score.hip), which needs no grouping by block
int launch_topk_pruned_f32(coper_handle* h, const TopkPlan& p, const float* hvec, const float* tgt, const int64_t* e2, const int64_t* indptr,
                           const int64_t* idx, int32_t* ng, int32_t* ne, float* topk_val, int64_t* topk_idx, hipStream_t s) {
  int rc;
  if (!h->topk.holds(p)) return fail(h, COPER_ESTATE, "pruned top-k: workspace not reserved");
  score_count_begin_f32(h, hvec, p.B, ng, ne, s);
  auto count = [&](int64_t q0, int64_t bc, float* gmax, int64_t qs) { return score_count_chunk_f32(h, q0, bc, tgt, ng, ne, gmax, qs, s); };
  if ((rc = tk_reset_lists(h, p, false, s)) || (rc = tk_chunks(h, p, indptr, s, count)) ||
      (rc = launch_topk_score_blocks_f32(h, hvec, p.T, e2, indptr, idx, s)))
    return rc;
  hipLaunchKernelGGL(k_topk_select_cand, dim3((unsigned)((p.B + 3) / 4)), dim3(256), 0, s, h->topk.cand_val_ws, h->topk.cand_blk_ws, h->topk.cand_tau_ws,
                     indptr, p.B, p.k_blocks, (int64_t)h->cfg.shard_lo, topk_val, topk_idx, (const int32_t*)nullptr, 1);
  COPER_HIP_TRY(h, hipGetLastError());
  return COPER_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// coper_predict_topk, COPER_SCORE_BF16X3: the top-k of a query WITHOUT a target, exact by the fp32 chain.
//
// The matrix-core logits only prune.  Steps 1 - 3 are the pruned top-k above with two changes: the count kernel runs for its block
// maxima alone (a band no logit reaches: score_count3_maxima_bf16x3), and the threshold kernel is asked for k + PREDICT_SLACK, so it
// emits m + s blocks (m = k + filter entries) and leaves t_last, the smallest emitted maximum, in cand_tau.  Every listed id is masked:
// the kernels that exempt a target read one that no entity has (-1).  Then, one workgroup per query (k_predict_select_x3):
//   u_k   = the k-th largest x3 logit among the unmasked entities of the emitted blocks;
//   tau_q = the band's bound for the query (x3_band_tau: a function of |h_q| and the table's constants), so every x3 logit is within
//           tau_q / 2 of its chain value -- what the band audit checks, and what this kernel audits on every pair it re-scores;
//   kept  = the candidates with x3 logit >= u_k - tau_q.  With v_k the chain's k-th largest value: u_k >= v_k - tau_q / 2 (the chain's
//           top k have x3 logits that large) and v_k >= u_k - tau_q / 2 (the x3 top k have chain values that large), so every member
//           of the chain's top-k has an x3 logit >= v_k - tau_q / 2 >= u_k - tau_q: it is kept, PROVIDED it was emitted.  An entity
//           of a block that was not emitted has an x3 logit <= t_last; the query is RESOLVED when t_last < u_k - tau_q.
//   The kept candidates are re-scored by the chain (exact_chain_pair on the registered fp32 rows) and the k largest by
//   (chain value desc, id asc) are the answer.
// A query that is not resolved (near-ties beyond the slack, more survivors than the LDS list holds) is listed on the device and
// served by k_predict_rows in the same call: the chain logits of its whole row into a scratch row, k rounds of arg-max.  No host
// synchronisation on either route.  (-inf thresholds / every block emitted: nothing is un-emitted, the query is resolved.)
// ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float tk_unkey(uint32_t key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

constexpr int PS_CAP = 2048;   // survivors (candidates >= t_last) per query held in LDS

struct PredictArgs {
  const float* cand_val; const int32_t* cand_blk; const uint32_t* cand_tau; const int64_t* indptr;
  const float* hvec; const float* ent; const float* bias; const unsigned* consts; const int32_t* x3s;
  float* out_val; int64_t* out_idx; int32_t* q_kept; uint32_t* q_ratio;
  int64_t B, lo; int k, ks, xf, d; float kappa;
};

__global__ __launch_bounds__(256) void k_predict_select_x3(const PredictArgs A) {
  __shared__ float s_v[PS_CAP];     // x3 logit of the survivor (accumulator units: x 2^(e_E + e_h))
  __shared__ int s_id[PS_CAP];      // its local row
  __shared__ float s_c[PS_CAP];     // its chain logit; -inf: not kept
  __shared__ float s_red[4];
  __shared__ int s_n, s_nk;
  __shared__ float s_uk;
  __shared__ uint32_t s_ratio;
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  const int k = A.k, d = A.d;
  const int sexp = A.x3s[1];
  const float* hr = A.hvec + q * d;
  if (tid == 0) { s_n = 0; s_nk = 0; s_uk = -INFINITY; s_ratio = 0u; }
  // |h_q|^2 -> tau_q
  float s2 = 0.f;
  for (int i = tid; i < d; i += 256) { const float v = hr[i]; s2 = fmaf(v, v, s2); }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s2 += __shfl_xor(s2, o);
  if ((tid & 63) == 0) s_red[tid >> 6] = s2;
  __syncthreads();
  s2 = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
  // (rounded up: a wider bound can only keep more candidates and resolve fewer queries)
  const float tau = x3_band_tau(s2 * 1.00001f, A.kappa, A.consts, d, A.x3s) * 1.0001f;
  const float tau_s = x3_scale(tau, sexp);
  const int64_t beg = A.indptr[q] - A.indptr[0];
  const int64_t off = A.xf * ((int64_t)A.ks * q + beg);
  const int n = A.xf * (int)((int64_t)A.ks + (A.indptr[q + 1] - A.indptr[0] - beg)) * 32;
  const float* val = A.cand_val + off * 32;
  const int32_t* blk = A.cand_blk + off;
  const uint32_t tkey = A.cand_tau[q];
  for (int j = tid; j < n; j += 256) {
    const int32_t b = blk[j >> 5];
    if (b < 0) continue;               // unused slot
    const float v = val[j];
    if (!(v > -INFINITY) || tk_key(v) < tkey) continue;
    const int pos = atomicAdd(&s_n, 1);
    if (pos < PS_CAP) { s_v[pos] = v; s_id[pos] = b * 32 + (j & 31); }
  }
  __syncthreads();
  const int S = s_n;
  float* ov = A.out_val + q * k;
  int64_t* oi = A.out_idx + q * k;
  bool resolved = S <= PS_CAP;
  if (resolved && S >= k) {
    for (int i = tid; i < S; i += 256) {
      const float v = s_v[i];
      const int id = s_id[i];
      int ahead = 0;
      for (int t = 0; t < S; ++t) {
        const float v2 = s_v[t];
        ahead += (v2 > v || (v2 == v && s_id[t] < id)) ? 1 : 0;
      }
      if (ahead == k - 1) s_uk = v;
    }
  }
  __syncthreads();
  float thr = -INFINITY;
  if (resolved && S >= k) {
    thr = s_uk - tau_s;
    thr -= fabsf(thr) * 2.4e-7f;       // (the subtraction's own rounding, downwards)
    resolved = tkey == 0u || tk_unkey(tkey) < thr;
  } else if (resolved) {
    resolved = tkey == 0u;             // fewer than k survivors: only when everything was emitted
  }
  if (!resolved) {                     // (workgroup-uniform)
    if (tid == 0) { A.q_kept[q] = -1; A.q_ratio[q] = 0u; }
    return;
  }
  float rmax = 0.f;
  for (int i = tid; i < S; i += 256) {
    float c = -INFINITY;
    if (s_v[i] >= thr) {
      const int64_t row = s_id[i];
      float unused = 0.f;
      exact_chain_pair(A.ent + row * d, nullptr, hr, A.bias[row], 0.f, d, c, unused);
      rmax = fmaxf(rmax, fabsf(x3_scale(s_v[i], -sexp) - c) / (0.5f * tau));
      atomicAdd(&s_nk, 1);
    }
    s_c[i] = c;
  }
  if (rmax > 0.f) atomicMax(&s_ratio, __float_as_uint(rmax));     // (non-negative floats order as their bits; NaN bits are largest: seen)
  __syncthreads();
  const int C = s_nk;
  for (int i = tid; i < S; i += 256) {
    const float c = s_c[i];
    if (!(c > -INFINITY)) continue;
    const int id = s_id[i];
    int ahead = 0;
    for (int t = 0; t < S; ++t) {
      const float c2 = s_c[t];
      ahead += (c2 > c || (c2 == c && s_id[t] < id)) ? 1 : 0;
    }
    if (ahead < k) { ov[ahead] = c; oi[ahead] = A.lo + id; }
  }
  for (int r = C + tid; r < k; r += 256) { ov[r] = -INFINITY; oi[r] = -1; }
  if (tid == 0) { A.q_kept[q] = C; A.q_ratio[q] = s_ratio; }
}

// one workgroup: the per-query words of the select kernel into the list of unresolved queries and the statistics
__global__ __launch_bounds__(1024) void k_predict_reduce(const int32_t* __restrict__ q_kept, const uint32_t* __restrict__ q_ratio, int64_t B,
                                                         int32_t* __restrict__ unres, uint32_t* __restrict__ stats) {
  __shared__ int s_cnt;
  __shared__ unsigned long long s_sum;
  __shared__ uint32_t s_max;
  if (threadIdx.x == 0) { s_cnt = 0; s_sum = 0ull; s_max = 0u; }
  __syncthreads();
  unsigned long long sum = 0ull;
  uint32_t mx = 0u;
  for (int64_t q = threadIdx.x; q < B; q += 1024) {
    const int32_t c = q_kept[q];
    if (c < 0) unres[atomicAdd(&s_cnt, 1)] = (int32_t)q;
    else { sum += (unsigned long long)c; const uint32_t r = q_ratio[q]; mx = r > mx ? r : mx; }
  }
  if (sum) atomicAdd(&s_sum, sum);
  if (mx) atomicMax(&s_max, mx);
  __syncthreads();
  if (threadIdx.x == 0) {
    stats[4] = (uint32_t)s_cnt;
    stats[0] += (uint32_t)s_cnt;
    stats[2] = s_max > stats[2] ? s_max : stats[2];
    *(unsigned long long*)(stats + 6) += s_sum;
  }
}

// The unconditional route: workgroup w serves the unresolved queries w, w + grid, ...: the chain logit of every unfiltered entity of
// the shard into the workgroup's scratch row (a known answer: -inf; the CSR rows are ascending: binary search), then k rounds of a
// workgroup-wide arg-max in (value desc, id asc) order.
__global__ __launch_bounds__(256) void k_predict_rows(const int32_t* __restrict__ unres, const uint32_t* __restrict__ stats,
                                                      const float* __restrict__ hvec, const float* __restrict__ ent,
                                                      const float* __restrict__ bias, const int64_t* __restrict__ indptr,
                                                      const int64_t* __restrict__ idx, int64_t lo, int64_t n_local, int d, int k,
                                                      float* __restrict__ rows, float* __restrict__ out_val, int64_t* __restrict__ out_idx) {
  __shared__ float s_val[256];
  __shared__ int s_idx[256];
  const int n_unres = (int)stats[4];
  float* row = rows + (int64_t)blockIdx.x * n_local;
  for (int u = blockIdx.x; u < n_unres; u += gridDim.x) {
    const int64_t q = unres[u];
    const float* hr = hvec + q * d;
    const int64_t fb = indptr[q], fe = indptr[q + 1];
    for (int64_t j = threadIdx.x; j < n_local; j += 256) {
      const int64_t gid = lo + j;
      int64_t a = fb, b = fe;
      while (a < b) { const int64_t m = (a + b) >> 1; if (idx[m] < gid) a = m + 1; else b = m; }
      float v = -INFINITY, unused = 0.f;
      if (!(a < fe && idx[a] == gid)) exact_chain_pair(ent + j * d, nullptr, hr, bias[j], 0.f, d, v, unused);
      row[j] = v;
    }
    __syncthreads();
    for (int round = 0; round < k; ++round) {
      float best = -INFINITY;
      int bi = 0x7fffffff;
      for (int64_t j = threadIdx.x; j < n_local; j += 256) {
        const float v = row[j];
        if (v > best || (v == best && v > -INFINITY && (int)j < bi)) { best = v; bi = (int)j; }
      }
      s_val[threadIdx.x] = best;
      s_idx[threadIdx.x] = bi;
      __syncthreads();
      for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) {
          const float v2 = s_val[threadIdx.x + o];
          const int i2 = s_idx[threadIdx.x + o];
          if (v2 > s_val[threadIdx.x] || (v2 == s_val[threadIdx.x] && i2 < s_idx[threadIdx.x])) { s_val[threadIdx.x] = v2; s_idx[threadIdx.x] = i2; }
        }
        __syncthreads();
      }
      if (threadIdx.x == 0) {
        const float v = s_val[0];
        const int i = s_idx[0];
        const bool ok = i != 0x7fffffff && v > -INFINITY;
        out_val[q * k + round] = ok ? v : -INFINITY;
        out_idx[q * k + round] = ok ? lo + i : -1;
        if (ok) row[i] = -INFINITY;   // taken
      }
      __syncthreads();
    }
  }
}

// workgroups (= scratch rows) of k_predict_rows: at most 64 MiB of rows, 256 workgroups, one per query
static int64_t predict_rows_workgroups(const coper_handle* h, int64_t B) {
  const int64_t w = std::min(std::min(((int64_t)64 << 20) / (h->dm.n_local * 4), (int64_t)256), B);
  return w < 1 ? 1 : w;
}

int PredictWs::ensure(coper_handle* h, int64_t B, hipStream_t s) {
  StreamGrow grow{h, s};
  int rc;
  if ((rc = grow(pred_ids_ws, (size_t)(2 * B + 1), "predict ids")) || h->cfg.score_mode == COPER_SCORE_F32) return rc;
  if ((rc = grow(pred_q_ws, (size_t)(3 * B), "predict per-query words")) ||
      (rc = grow(pred_rows_ws, (size_t)(predict_rows_workgroups(h, B) * h->dm.n_local), "predict rows")))
    return rc;
  if (pred_stats) return COPER_OK;
  if ((rc = grow(pred_stats, 8, "predict statistics"))) return rc;
  COPER_HIP_TRY(h, hipMemsetAsync(pred_stats, 0, 8 * sizeof(uint32_t), s));
  return COPER_OK;
}

int predict_filter_args(coper_handle* h, int64_t B, bool raw, const int64_t** no_target, const int64_t** indptr, const int64_t** idx, hipStream_t s) {
  int64_t* ids = h->pred.pred_ids_ws;
  COPER_HIP_TRY(h, hipMemsetAsync(ids, 0xFF, sizeof(int64_t) * B, s));
  *no_target = ids;
  if (!raw) return COPER_OK;
  COPER_HIP_TRY(h, hipMemsetAsync(ids + B, 0, sizeof(int64_t) * (B + 1), s));
  *indptr = *idx = ids + B;      // (idx is never read: every row is empty)
  return COPER_OK;
}

int predict_stats_read(coper_handle* h, bool reset, uint32_t v[8], hipStream_t s) {
  if (!h->pred.pred_stats) return COPER_OK;
  COPER_HIP_TRY(h, hipMemcpyAsync(v, h->pred.pred_stats, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  if (reset) COPER_HIP_TRY(h, hipMemsetAsync(h->pred.pred_stats, 0, 8 * sizeof(uint32_t), s));
  COPER_HIP_TRY(h, hipStreamSynchronize(s));
  return COPER_OK;
}

int launch_predict_topk_bf16x3(coper_handle* h, const TopkPlan& p, const float* hvec, const int64_t* no_target, const int64_t* indptr,
                               const int64_t* idx, int k, float* topk_val, int64_t* topk_idx, hipStream_t s) {
  const Dims& dm = h->dm;
  TopkWs& w = h->topk;
  PredictWs& pw = h->pred;
  const int64_t B = p.B, W = predict_rows_workgroups(h, B);
  int rc;
  if (!w.holds(p) || (size_t)(3 * B) > pw.pred_q_ws.size() || !pw.pred_stats || (size_t)(W * dm.n_local) > pw.pred_rows_ws.size())
    return fail(h, COPER_ESTATE, "predict top-k: workspace not reserved");
  // a band no logit reaches (0x7f7f7f7f = 3.4e38 on both ends): the count kernel counts nothing and marks nothing
  COPER_HIP_TRY(h, hipMemsetAsync(h->tband_ws, 0x7f, sizeof(float) * h->tband_ws.size(), s));
  auto count = [&](int64_t q0, int64_t bc, float* gmax, int64_t qs) { return score_count3_maxima_bf16x3(h, q0, bc, h->cnt_ws, gmax, qs, s); };
  if ((rc = tk_reset_lists(h, p, true, s)) || (rc = tk_chunks(h, p, indptr, s, count))) return rc;
  tk_group_rescore(h, p, no_target, indptr, idx, s);
  PredictArgs A;
  A.cand_val = w.cand_val_ws; A.cand_blk = w.cand_blk_ws; A.cand_tau = w.cand_tau_ws; A.indptr = indptr;
  A.hvec = hvec; A.ent = h->lv.ent_emb->ptr; A.bias = h->lv.pred_bias->ptr; A.consts = h->band_consts; A.x3s = h->x3s;
  A.out_val = topk_val; A.out_idx = topk_idx; A.q_kept = pw.pred_q_ws; A.q_ratio = (uint32_t*)(pw.pred_q_ws + B);
  A.B = B; A.lo = (int64_t)h->cfg.shard_lo; A.k = k; A.ks = p.k_blocks; A.xf = p.XF; A.d = dm.d; A.kappa = band_kappa(h);
  hipLaunchKernelGGL(k_predict_select_x3, dim3((unsigned)B), dim3(256), 0, s, A);
  hipLaunchKernelGGL(k_predict_reduce, dim3(1), dim3(1024), 0, s, (const int32_t*)pw.pred_q_ws, (const uint32_t*)(pw.pred_q_ws + B), B,
                     pw.pred_q_ws + 2 * B, (uint32_t*)pw.pred_stats);
  hipLaunchKernelGGL(k_predict_rows, dim3((unsigned)W), dim3(256), 0, s, (const int32_t*)(pw.pred_q_ws + 2 * B), (const uint32_t*)pw.pred_stats,
                     hvec, A.ent, A.bias, indptr, idx, A.lo, dm.n_local, dm.d, k, pw.pred_rows_ws, topk_val, topk_idx);
  COPER_HIP_TRY(h, hipGetLastError());
  return COPER_OK;
}

}  // namespace coper
