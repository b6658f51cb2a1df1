// The kernels of the training step (coper_train.hip, which alone includes this file) and the constants the host code shares with
// them, in the order of the step: forward, scorer, backward, optimizer; then the kernels of coper_train_forward and coper_train_grad.
#pragma once
#include "coper_internal.h"
#include "train_common.h"
#include "train_gemm.h"
#include "train_rows.h"

namespace coper {
namespace {

constexpr float BN_EPS = 1e-3f;
constexpr int TR_LK_NSL = 4;     // F slices of the looked-up dense layer's forward (partial sums in T->dx)
constexpr int TR_ZERO_MAX = 16;
constexpr int TR_COLSUM_SLICES = 20;   // column-sum scratch: one slice per use within a step (RedLayout::colsum_slice)
constexpr int TR_CS_SLOTS = 16;   // copies of a column-sum slice that many workgroups add to (workgroup w: copy w % slots)
constexpr int TR_MAX_PARAMS = 40;
constexpr int TR_EXP_CACHE = 8;
// column-sum slices (RedLayout::colsum_slice): FCBN, then layer i of generator chain g (distinct for up to four hidden layers); Conv1BN's
// statistics and backward sums live in TR_CS_SLOTS copies instead (RedLayout::cs_slots), slices 0 and 2 stay free
enum ColsumSlice { CS_FCBN = 1, CS_CHAIN = 3 };
constexpr int cs_chain(int g, int i) { return CS_CHAIN + 4 * g + i; }
enum CsSlots { CSS_BN1_FWD = 0, CSS_BN1_BWD = 1 };
enum SideSlot { SJ_SCORER_BWD = 1, SJ_DP = 2 };      // fork / join slots of the side streams (SideJoin: TrainState::ev_fork[i] / ev_join[i])

// ------------------------------------------------------------------------------------------------
// forward kernels
// ------------------------------------------------------------------------------------------------
// one workgroup per query: gather the image, 3x3 VALID cross-correlation + bias -> y[b, p, c]
__global__ __launch_bounds__(256) void k_tr_conv_fwd(const int64_t* __restrict__ e1, const int64_t* __restrict__ rel,
                                                     const float* __restrict__ ent, const float* __restrict__ rel_emb,
                                                     const float* __restrict__ K, const float* __restrict__ kb, int64_t E,
                                                     int64_t R, int d, int r, int in_h, int in_w, int stacked, int C, int Ho,
                                                     int Wo, float* __restrict__ img_out, float* __restrict__ c_out,
                                                     float* __restrict__ y, const float* __restrict__ K_ps,
                                                     const float* __restrict__ kb_ps, int fh, int fw) {
  extern __shared__ float lds[];  // img[in_h*in_w] | taps[fh*fw*C] | kb[C]
  const int nt = fh * fw;
  float* img = lds;
  float* taps = img + in_h * in_w;
  float* bias = taps + nt * C;
  const int64_t b = blockIdx.x;
  int64_t row = e1[b];
  if (row < 0 || row >= E) row = 0;
  int64_t rid = rel[b];
  if (rid < 0 || rid >= R) rid = 0;
  for (int t = threadIdx.x; t < d; t += 256) img[t] = ent[row * d + t];
  if (stacked)
    for (int t = threadIdx.x; t < r; t += 256) img[d + t] = rel_emb[rid * r + t];
  if (c_out)
    for (int t = threadIdx.x; t < r; t += 256) c_out[b * r + t] = rel_emb[rid * r + t];
  // per-sample filters (generated / looked up, models.py:374-380) or the shared static ones
  const float* Ksrc = K_ps ? K_ps + b * (int64_t)nt * C : K;
  const float* bsrc = kb_ps ? kb_ps + b * C : kb;
  for (int t = threadIdx.x; t < nt * C; t += 256) taps[t] = Ksrc[t];
  for (int t = threadIdx.x; t < C; t += 256) bias[t] = bsrc[t];
  __syncthreads();
  const int isz = in_h * in_w;
  for (int t = threadIdx.x; t < isz; t += 256) img_out[b * isz + t] = img[t];
  const int P = Ho * Wo;
  float* yb = y + b * (int64_t)P * C;
  for (int idx = threadIdx.x; idx < P * C; idx += 256) {
    const int cc = idx % C, p = idx / C;
    const int i = p / Wo, j = p - i * Wo;
    float a = 0.f;
    if (fh == 3 && fw == 3) {   // the shipped shape, unrolled; same summation order as the general loop
#pragma unroll
      for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = 0; v < 3; ++v) a = fmaf(img[(i + u) * in_w + j + v], taps[(u * 3 + v) * C + cc], a);
    } else {
      for (int u = 0; u < fh; ++u)
        for (int v = 0; v < fw; ++v) a = fmaf(img[(i + u) * in_w + j + v], taps[(u * fw + v) * C + cc], a);
    }
    yb[idx] = a + bias[cc];
  }
}

// per-column sums of a [rows, cols] matrix in double: out[0..cols) = sum, out[cols..2cols) = sum of squares
// (partial sums by row chunk, then atomics on doubles: order-dependent only in the last bits of a double)
// everything the step accumulates into with atomics, zeroed by ONE launch (was a dozen memsets of ~5 us each)
struct ZeroList {
  void* p[TR_ZERO_MAX];
  size_t bytes[TR_ZERO_MAX];   // multiples of 4
  int n;
};
__global__ __launch_bounds__(256) void k_tr_zero_list(ZeroList zl) {
  const int e = blockIdx.y;
  if (e >= zl.n) return;
  char* base = (char*)zl.p[e];
  const size_t bytes = zl.bytes[e];
  const size_t head = ((16 - ((uintptr_t)base & 15)) & 15) < bytes ? ((16 - ((uintptr_t)base & 15)) & 15) : bytes;
  const size_t n16 = (bytes - head) / 16, tail0 = head + n16 * 16;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  for (size_t i = t; i < n16; i += stride) ((uint4*)(base + head))[i] = make_uint4(0, 0, 0, 0);
  for (size_t i = t * 4; i < head; i += stride * 4) *(uint32_t*)(base + i) = 0;
  for (size_t i = tail0 + t * 4; i < bytes; i += stride * 4) *(uint32_t*)(base + i) = 0;
}

// the TR_CS_SLOTS copies of a slice are folded into copy 0 by a launch of one workgroup (k_tr_fold_slots), so readers see one slice.  (Round 6 also tried the fold by the
// LAST workgroup of the adding launch -- a ticket behind a __threadfence: every workgroup then waits for its own stores to drain
// before the ticket, 140 us against 12 for k_tr_bn1_bwd_sums -- and the fold in every reading workgroup: + 10 us on 9,216 of them.)
__global__ __launch_bounds__(256) void k_tr_fold_slots(double* __restrict__ base, int n2, int nslots) {
  for (int j = threadIdx.x; j < n2; j += 256) {
    double v[TR_CS_SLOTS];
#pragma unroll
    for (int z = 0; z < TR_CS_SLOTS; ++z) v[z] = z < nslots ? base[(size_t)z * n2 + j] : 0.0;
    double a = 0;
#pragma unroll
    for (int z = 0; z < TR_CS_SLOTS; ++z) a += v[z];
    base[j] = a;
  }
}
// DET (deterministic mode): workgroup w STORES its partial sums in a slab of its own, out[w][2 cols]; k_tr_fold_det adds the slabs
template <bool DET>
__global__ __launch_bounds__(256) void k_tr_col_sums(const float* __restrict__ m, int64_t rows, int cols, double* __restrict__ out, int nslots) {
  // per-column sum and sum of squares in double; a block reduces its row lanes in LDS and issues ONE atomic pair per
  // column (many blocks adding to the same few addresses are contention-bound: 14x slower per add -- 1024 workgroups on the 64
  // addresses of Conv1BN's statistics took 33 us for a 3 us read, so those go to TR_CS_SLOTS copies of the slice)
  __shared__ double sh[2][256];
  if constexpr (DET) out += (size_t)blockIdx.x * 2 * cols;
  else out += (size_t)(blockIdx.x % nslots) * 2 * cols;
  if (cols <= 256) {
    const int cpt = 256 / cols;                         // row lanes per column
    const int col = threadIdx.x % cols, rl = threadIdx.x / cols;
    double s = 0, q = 0;
    if (rl < cpt) {
      const int64_t st = (int64_t)gridDim.x * cpt;
      int64_t rr = (int64_t)blockIdx.x * cpt + rl;
      for (; rr + 3 * st < rows; rr += 4 * st) {          // four loads in flight, added in row order
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = m[(rr + u * st) * cols + col];
#pragma unroll
        for (int u = 0; u < 4; ++u) { s += (double)v[u]; q += (double)v[u] * v[u]; }
      }
      for (; rr < rows; rr += st) {
        const double v = m[rr * cols + col];
        s += v;
        q += v * v;
      }
    }
    sh[0][threadIdx.x] = s;
    sh[1][threadIdx.x] = q;
    __syncthreads();
    if (threadIdx.x < cols) {
      for (int l = 1; l < cpt; ++l) { s += sh[0][threadIdx.x + l * cols]; q += sh[1][threadIdx.x + l * cols]; }
      if constexpr (DET) { out[col] = s; out[cols + col] = q; }
      else {
      atomicAdd(&out[col], s);
      atomicAdd(&out[cols + col], q);
      }
    }
  } else {
    for (int cc = threadIdx.x; cc < cols; cc += 256) {
      double s = 0, q = 0;
      for (int64_t rr = blockIdx.x; rr < rows; rr += gridDim.x) {
        const double v = m[rr * cols + cc];
        s += v;
        q += v * v;
      }
      if constexpr (DET) { out[cc] = s; out[cols + cc] = q; }
      else {
      atomicAdd(&out[cc], s);
      atomicAdd(&out[cols + cc], q);
      }
    }
  }
}

// BN statistics -> (mean, inv_std) used by forward and backward; moving statistics updated in place.
// unbiased_moving: [TF-semantics] the fused 4-D kernel feeds the unbiased variance into the moving average.
// unbiased_moving bit 1 (value 2): leave the moving statistics alone (coper_train_forward: a fetch without train_op runs none of
// the UPDATE_OPS, models.py:194-200).
__global__ void k_tr_bn_finish(const double* __restrict__ sums, int cols, double n, int use_batch, float momentum,
                               int unbiased_moving, float* __restrict__ mov_mean, float* __restrict__ mov_var,
                               float* __restrict__ mean_out, float* __restrict__ inv_out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  if (use_batch) {
    const double mean = sums[c] / n;
    double var = sums[cols + c] / n - mean * mean;
    if (var < 0) var = 0;
    mean_out[c] = (float)mean;
    inv_out[c] = (float)(1.0 / sqrt(var + (double)BN_EPS));
    if (unbiased_moving & 2) return;
    const double var_m = (unbiased_moving & 1) ? var * (n / (n - 1.0)) : var;
    mov_mean[c] = (float)((double)mov_mean[c] * momentum + mean * (1.0 - (double)momentum));
    mov_var[c] = (float)((double)mov_var[c] * momentum + var_m * (1.0 - (double)momentum));
  } else {
    mean_out[c] = mov_mean[c];
    inv_out[c] = 1.0f / sqrtf(mov_var[c] + BN_EPS);
  }
}

// x = keep * relu(bn(y)) / (1 - rate)     (elementwise over [B, P, C]; flat index = the dropout counter)
// the largest |value| a workgroup of 256 wrote -> one of TG_MAX_SLOTS slots (train_gemm.h: tg_pack's max_slots): the elementwise
// kernel that PRODUCES a GEMM operand leaves its maximum behind, so that the pack needs no pass of its own over the tensor (round 6)
__device__ __forceinline__ void tr_block_max_to_slot(float v_abs, unsigned* __restrict__ slots) {
  unsigned m = __float_as_uint(v_abs);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned u = __shfl_xor(m, o, 64); m = u > m ? u : m; }
  __shared__ unsigned s_bm[4];
  if ((threadIdx.x & 63) == 0) s_bm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned a = s_bm[0] > s_bm[1] ? s_bm[0] : s_bm[1], b = s_bm[2] > s_bm[3] ? s_bm[2] : s_bm[3], w = a > b ? a : b;
    if (w) atomicMax(slots + (blockIdx.x & (TG_MAX_SLOTS - 1)), w);
  }
}

__global__ __launch_bounds__(256) void k_tr_bn1_fwd(const float* __restrict__ y, const float* __restrict__ mean,
                                                    const float* __restrict__ inv, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, int C, int64_t total, uint32_t seed,
                                                    uint32_t step, uint32_t ioff, uint32_t thr, float keep_scale, float* __restrict__ x,
                                                    unsigned* __restrict__ max_slots) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float out = 0.f;
  if (i < total) {
    const int c = (int)(i % C);
    float v = (y[i] - mean[c]) * inv[c] * gamma[c] + beta[c];
    v = v > 0.f ? v : 0.f;
    out = dropout_keep_u32(seed, step, 1u, (uint32_t)i + ioff, thr) ? v * keep_scale : 0.f;
    x[i] = out;
  }
  if (max_slots) tr_block_max_to_slot(out, max_slots);       // (x >= 0)
}

// z1 = keep * (z0 + bias_b) / (1 - rate).  Static: z0 from the GEMM, bias_b = fc_bias[k].  Generated:
// z0[b,k] = sum_rho c[b,rho] T[rho][b,k] (T[rho] = x P[rho], the batched GEMM), bias_b = sum_rho c[b,rho] Pb[rho,k]
__global__ __launch_bounds__(256) void k_tr_fc_post(const float* __restrict__ z0, const float* __restrict__ fc_bias,
                                                    const float* __restrict__ cw, int rw, const float* __restrict__ cb,
                                                    const float* __restrict__ Pb, int rb, int d, int64_t total, uint32_t seed,
                                                    uint32_t step, uint32_t ioff, uint32_t thr, float keep_scale, float* __restrict__ z1) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int k = (int)(i % d);
  const int64_t b = i / d;
  float v;
  if (Pb) {
    v = 0.f;
    for (int rho = 0; rho < rw; ++rho) v = fmaf(cw[b * rw + rho], z0[(int64_t)rho * total + i], v);
    for (int rho = 0; rho < rb; ++rho) v = fmaf(cb[b * rb + rho], Pb[rho * d + k], v);
  } else {
    v = z0[i] + fc_bias[k];
  }
  z1[i] = dropout_keep_u32(seed, step, 2u, (uint32_t)i + ioff, thr) ? v * keep_scale : 0.f;
}

// the generated dense layer straight from the K slices of its product (tg_gemm_nt: leave_slices): T[rho][b, k] = the slices of
// part[z][b][rho d + k] added in slice order -- what k_tg_reduce stores, kept for the backward pass -- and z1 as k_tr_fc_post forms it.
// One kernel instead of two, the 13 MB of T written once and not read back (round 6: 39.8 us -> the slices' 65 MB at stream rate).
template <int NS>
__global__ __launch_bounds__(256) void k_tr_fc_post_slices(const float* __restrict__ part, const float* __restrict__ cw, int rw,
                                                           const float* __restrict__ cb, const float* __restrict__ Pb, int rb, int d,
                                                           int64_t total, uint32_t seed, uint32_t step, uint32_t ioff, uint32_t thr, float keep_scale,
                                                           float* __restrict__ Tf, float* __restrict__ z1) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int k = (int)(i % d);
  const int64_t b = i / d;
  const int64_t N = (int64_t)rw * d, MN = (total / d) * N;
  const float* p = part + b * N + k;
  float v = 0.f;
#pragma unroll 4
  for (int rho = 0; rho < rw; ++rho) {
    float t[NS];
#pragma unroll
    for (int z = 0; z < NS; ++z) t[z] = p[(int64_t)z * MN + (int64_t)rho * d];
    float a = 0.f;
#pragma unroll
    for (int z = 0; z < NS; ++z) a += t[z];
    Tf[(int64_t)rho * total + i] = a;
    v = fmaf(cw[b * rw + rho], a, v);
  }
  for (int rho = 0; rho < rb; ++rho) v = fmaf(cb[b * rb + rho], Pb[rho * d + k], v);
  z1[i] = dropout_keep_u32(seed, step, 2u, (uint32_t)i + ioff, thr) ? v * keep_scale : 0.f;
}

__global__ __launch_bounds__(256) void k_tr_fcbn_fwd(const float* __restrict__ z1, const float* __restrict__ mean,
                                                     const float* __restrict__ inv, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, int d, int64_t total,
                                                     float* __restrict__ hv) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int k = (int)(i % d);
  const float v = (z1[i] - mean[k]) * inv[k] * gamma[k] + beta[k];
  hv[i] = v > 0.f ? v : 0.f;
}

// sampled scorer + loss + d(loss)/ds.  One workgroup per query; h[b] in LDS; one lookup entry per thread.
// DET (here and in the other loss kernels): the workgroup's loss share is STORED at loss_acc[blockIdx.x], a slab k_tr_fold_det adds
// SHARD (here and in the other sampled-scorer kernels): ent / pred_bias hold rows [sh_lo, sh_lo + sh_n) of the E-row
// table, and only an entry whose (clamped) id lies there is served -- the same chain per entry; an entry of another shard costs no
// row read, no store and no loss term.  Without SHARD the two bounds are not read.
// CURRENT (with SHARD; the forward-only sharded call in the deferred-rows mode): the table may hold a row several updates
// behind -- the row load forms it AS OF THE CURRENT UPDATE in registers (rows_wave_C / rows_elem_catch_up on p, m, v, v_hat and the
// row's word: the value k_rows_catch_up would store, bit for bit) and writes nothing; a row with gap 0 is read as it stands.  The
// waves make every trip of the entry loop whole, so that a gap's scalars are formed by 64 lanes together.
template <bool DET, bool SHARD = false, bool CURRENT = false>
__global__ __launch_bounds__(256) void k_tr_score_loss(const float* __restrict__ hv, const float* __restrict__ ent,
                                                       const float* __restrict__ pred_bias,
                                                       const int32_t* __restrict__ lookup, const float* __restrict__ labels,
                                                       int64_t E, int d, int64_t L, float ls_eps, float inv_E, float inv_BL,
                                                       float* __restrict__ ds, double* __restrict__ loss_acc, int64_t sh_lo = 0,
                                                       int64_t sh_n = 0, RowTables rt = RowTables(), RowCatchUp cu = RowCatchUp()) {
  static_assert(!CURRENT || SHARD, "the CURRENT row load is a form of the SHARD kernels");
  extern __shared__ float hl[];
  __shared__ double part[256];
  const int64_t b = blockIdx.x;
  for (int k = threadIdx.x; k < d; k += 256) hl[k] = hv[b * d + k];
  __syncthreads();
  double acc = 0.0;
  const int64_t Lw = CURRENT ? (L + 255) / 256 * 256 : L;
  for (int64_t l = threadIdx.x; l < Lw; l += 256) {
    int64_t row = 0;
    [[maybe_unused]] double Cs = 0.0;
    [[maybe_unused]] bool behind = false;
    if constexpr (CURRENT) {
      bool own = l < L;
      if (own) {
        row = lookup[b * L + l];
        row = ((row < 0 || row >= E) ? 0 : row) - sh_lo;
        own = row >= 0 && row < sh_n;
      }
      const int gap = own ? cu.now - rt.word[row] : 0;
      behind = gap > 0;
      Cs = rows_wave_C(cu, gap, (int)(threadIdx.x & 63));
      if (!own) continue;
    } else {
    row = lookup[b * L + l];
    if (row < 0 || row >= E) row = 0;
    if constexpr (SHARD) {
      row -= sh_lo;
      if (row < 0 || row >= sh_n) continue;
    }
    }
    const float* er = ent + row * d;
    float s = 0.f;
    if ((d & 3) == 0) {   // 16-byte loads of the gathered row; the fma chain keeps its order
      const float4* er4 = (const float4*)er;
      for (int k4 = 0; k4 < d / 4; ++k4) {
        float4 e = er4[k4];
        if constexpr (CURRENT) { if (behind) e = rows_current4(rt, cu, row * d + 4 * k4, e, Cs); }
        s = fmaf(hl[4 * k4 + 0], e.x, s); s = fmaf(hl[4 * k4 + 1], e.y, s);
        s = fmaf(hl[4 * k4 + 2], e.z, s); s = fmaf(hl[4 * k4 + 3], e.w, s);
      }
    } else {
      for (int k = 0; k < d; ++k) {
        float e = er[k];
        if constexpr (CURRENT) { if (behind) e = rows_current1(rt, cu, row * d + k, e, Cs); }
        s = fmaf(hl[k], e, s);
      }
    }
    float pb = pred_bias[row];
    if constexpr (CURRENT) { if (behind) pb = rows_current_bias(rt, cu, row, pb, Cs); }
    s += pb;
    const float t = (1.f - ls_eps) * labels[b * L + l] + inv_E;                  // models.py:450
    const float as = fabsf(s);
    acc += (double)(fmaxf(s, 0.f) - s * t + log1pf(expf(-as)));                 // sigmoid cross-entropy with logits
    const float sg = 1.f / (1.f + expf(-s));
    ds[b * L + l] = (sg - t) * inv_BL;
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if constexpr (DET) loss_acc[blockIdx.x] = part[0];
    else atomicAdd(loss_acc, part[0]);
  }
}

// The sampled scorer of a training step in ONE pass over the gathered rows (round 6): scores, loss, ds AND dh = sum_l ds E[row].
// k_tr_score_loss + k_tr_dh_gather4 each read the B L rows of d floats (410 MB at 512 x 1000 x 200: 61 + 45 us); sigmoid
// cross-entropy is elementwise, so ds[b, l] is known as soon as row l's score is, while the row is still in registers.
// k_tr_dh_gather4's layout: a thread owns four features (one 16-byte load) of one of 256 / (d / 4) row slots, SF_U rows per
// slot and batch; the next batch's rows are requested before this batch is touched.  Per batch: every thread's four-term
// share of its rows' dot products -> LDS; one thread per row adds the d / 4 shares in feature order, forms loss and ds;
// every thread adds ds x its registers to its dh share.  (An earlier fused form -- a wave per row, butterfly sums -- was
// latency end to end: 242 us.)
#ifndef COPER_SF_U
#define COPER_SF_U 12
#endif
constexpr int SF_U = COPER_SF_U;      // rows per slot and batch
constexpr int SF_MAX_L = 8192;       // lookup entries of a query held in LDS (32 KB)
// SHARD (k_tr_score_loss's comment): the sample's owned entries are compacted in LDS -- stable, ascending l: ids[j] the
// local row of the j-th owned entry, pos[j] its l -- and the batch loop below runs over the compacted count Ln in place of L, so the
// rows of other shards are never requested.  A row's score chain does not depend on where in a batch the row sits, so ds[b, l] is
// the whole-table launch's value; dh and the loss share add the owned terms in the order this kernel gives Ln entries.  A shard
// that owns every entry compacts to the identity.  (LDS: int pos[L] behind ids.)
// CURRENT (k_tr_score_loss's comment): the compaction also forms, wave by wave, C of every owned entry's gap (LDS: double
// cnow[L] and a byte behind[L] more); the row fetch and the bias load of an entry that is behind apply it to what they loaded.
template <bool DET, bool SHARD = false, bool CURRENT = false>
__global__ __launch_bounds__(256) void k_tr_score_loss_dh(const float* __restrict__ hv, const float* __restrict__ ent,
                                                          const float* __restrict__ pred_bias, const int32_t* __restrict__ lookup,
                                                          const float* __restrict__ labels, int64_t E, int d, int L, float ls_eps,
                                                          float inv_E, float inv_BL, float* __restrict__ ds, float* __restrict__ dh,
                                                          double* __restrict__ loss_acc, int64_t sh_lo = 0, int64_t sh_n = 0,
                                                          RowTables rt = RowTables(), RowCatchUp cu = RowCatchUp()) {
  static_assert(!CURRENT || SHARD, "the CURRENT row load is a form of the SHARD kernels");
  extern __shared__ float4 sf_lds[];   // float4 [slots][d4] (the slots' dh shares at the end) | float part[RB][d4 + 1] | float g[RB] | int ids[L]
  __shared__ double red[256];
  const int64_t b = blockIdx.x;
  const int d4 = d >> 2, slots = 256 / d4 > 256 / SF_U ? 256 / SF_U : 256 / d4, RB = SF_U * slots, PS = d4 + 1;      // (RB <= 256: a thread per row of a batch)
  // threads that share a row's sum of partial products (a power of two, neighbours in a wave)
  const int tpr = 256 / RB >= 8 ? 8 : (256 / RB >= 4 ? 4 : (256 / RB >= 2 ? 2 : 1));
  float* part = (float*)(sf_lds + slots * d4);
  float* gsh = part + RB * PS;
  int* ids = (int*)(gsh + RB);
  const int slot = threadIdx.x / d4, q4 = threadIdx.x - slot * d4;
  const bool live = slot < slots;
  // the query's rows, range-checked once (a row id is read by the thread that loads the row, by the thread that scores it, ...)
  int Ln = L;      // the entries the batch loop walks
  [[maybe_unused]] int* const pos = ids + L;
  [[maybe_unused]] double* const cnow = (double*)(pos + L);      // (8-byte aligned: RB is a multiple of 4, ids and pos are 8 L bytes)
  [[maybe_unused]] unsigned char* const behind = (unsigned char*)(cnow + L);
  if constexpr (SHARD) {
    __shared__ int wown[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int base = 0;      // owned entries in front of this round (uniform)
    for (int l0 = 0; l0 < L; l0 += 256) {
      const int l = l0 + (int)threadIdx.x;
      int64_t row = -1;
      if (l < L) {
        row = lookup[b * L + l];
        row = ((row < 0 || row >= E) ? 0 : row) - sh_lo;
      }
      const bool own = row >= 0 && row < sh_n;
      [[maybe_unused]] int gap = 0;
      [[maybe_unused]] double Cs = 0.0;
      if constexpr (CURRENT) {
        gap = own ? cu.now - rt.word[row] : 0;
        Cs = rows_wave_C(cu, gap, lane);
      }
      const unsigned long long om = __ballot(own);
      if (lane == 0) wown[w] = (int)__popcll(om);
      __syncthreads();
      int at = base + (int)__popcll(om & ((1ull << lane) - 1ull));
      for (int q = 0; q < w; ++q) at += wown[q];
      if (own) {      // (at <= l < L)
        ids[at] = (int)row;
        pos[at] = l;
        if constexpr (CURRENT) {
          cnow[at] = Cs;
          behind[at] = gap > 0 ? 1 : 0;
        }
      }
      base += wown[0] + wown[1] + wown[2] + wown[3];
      __syncthreads();
    }
    Ln = base;
    if (Ln == 0) {      // (uniform) nothing of this sample lives here: an exact zero row, a zero loss share
      for (int k = threadIdx.x; k < d; k += 256) dh[b * d + k] = 0.f;
      if (threadIdx.x == 0) {
        if constexpr (DET) loss_acc[blockIdx.x] = 0.0;
      }
      return;
    }
  } else {
  for (int l = threadIdx.x; l < L; l += 256) {
    const int32_t row = lookup[b * L + l];
    ids[l] = (row < 0 || row >= E) ? 0 : row;
  }
  }
  // where entry j of the walk sits in the sample's [L] arrays
  auto at_l = [&](int j) { if constexpr (SHARD) return pos[j]; else return j; };
  const float4 h4 = live ? *(const float4*)(hv + b * d + 4 * q4) : make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  double lacc = 0.0;
  float4 va[SF_U], vb[SF_U];
  // (every load of the loop is unconditional, with clamped indices, and issued in ONE order -- this batch's label and bias, then the
  //  next batch's rows: the vector-memory counter retires in order, so a wait for a load issued after the prefetch would drain it,
  //  and a load under a branch makes the compiler wait for everything)
#define SF_FETCH(l0_, dst_)                                                                   \
  {                                                                                           \
    _Pragma("unroll") for (int u = 0; u < SF_U; ++u) {                                        \
      const int l = (l0_) + u * slots + slot;                                                 \
      const int lj = l < Ln ? l : Ln - 1;                                                     \
      const int64_t row = ids[lj];                                                            \
      dst_[u] = *(const float4*)(ent + row * d + 4 * qc);                                     \
      if constexpr (CURRENT) {                                                                \
        if (behind[lj]) dst_[u] = rows_current4(rt, cu, row * d + 4 * qc, dst_[u], cnow[lj]); \
      }                                                                                       \
    }                                                                                         \
  }
  const int qc = live ? q4 : 0;                                  // (threads past the last slot load, and drop, a valid address)
  const int sr = threadIdx.x / tpr, sj = threadIdx.x % tpr;      // scoring: row sr of the batch, share sj of its partial products
  const int q_lo = (int)((int64_t)d4 * sj / tpr), q_hi = (int)((int64_t)d4 * (sj + 1) / tpr);
#define SF_BATCH(l0_, cur_, nxt_)                                                             \
  {                                                                                           \
    const int lb = (l0_);                                                                     \
    const bool on = sr < RB && lb + sr < Ln;   /* (uniform over the tpr neighbours of a row) */ \
    const int lc = lb + sr < Ln ? lb + sr : Ln - 1;                                           \
    const float lab = labels[b * L + at_l(lc)];                                               \
    float pb = pred_bias[ids[lc]];                                                            \
    if constexpr (CURRENT) {                                                                  \
      if (behind[lc]) pb = rows_current_bias(rt, cu, ids[lc], pb, cnow[lc]);                  \
    }                                                                                         \
    SF_FETCH(lb + RB, nxt_);                                                                  \
    if (live) {                                                                               \
      _Pragma("unroll") for (int u = 0; u < SF_U; ++u) {                                      \
        float pz = h4.x * cur_[u].x;                                                          \
        pz = fmaf(h4.y, cur_[u].y, pz); pz = fmaf(h4.z, cur_[u].z, pz); pz = fmaf(h4.w, cur_[u].w, pz); \
        part[(u * slots + slot) * PS + q4] = pz;                                              \
      }                                                                                       \
    }                                                                                         \
    __syncthreads();                                                                          \
    float sc = 0.f;                                                                           \
    if (on) {                                                                                 \
      const float* pr = part + sr * PS;                                                       \
      for (int q = q_lo; q < q_hi; ++q) sc += pr[q];                                          \
    }                                                                                         \
    for (int o = 1; o < tpr; o <<= 1) sc += __shfl_xor(sc, o, 64);   /* (the same sum in every neighbour) */ \
    if (on && sj == 0) {                                                                      \
      sc += pb;                                                                               \
      const float t = (1.f - ls_eps) * lab + inv_E;                    /* models.py:450 */    \
      const float as = fabsf(sc);                                                             \
      lacc += (double)(fmaxf(sc, 0.f) - sc * t + log1pf(expf(-as)));   /* sigmoid cross-entropy with logits */ \
      const float sg = 1.f / (1.f + expf(-sc));                                               \
      const float g = (sg - t) * inv_BL;                                                      \
      ds[b * L + at_l(lb + sr)] = g;                                                          \
      gsh[sr] = g;                                                                            \
    }                                                                                         \
    __syncthreads();                                                                          \
    if (live) {                                                                               \
      _Pragma("unroll") for (int u = 0; u < SF_U; ++u)                                        \
        if (lb + u * slots + slot < Ln) {                                                     \
          const float g = gsh[u * slots + slot];                                              \
          acc.x = fmaf(g, cur_[u].x, acc.x); acc.y = fmaf(g, cur_[u].y, acc.y);               \
          acc.z = fmaf(g, cur_[u].z, acc.z); acc.w = fmaf(g, cur_[u].w, acc.w);               \
        }                                                                                     \
    }                                                                                         \
  }
  SF_FETCH(0, va);
  for (int l0 = 0; l0 < Ln; l0 += 2 * RB) {
    SF_BATCH(l0, va, vb);
    if (l0 + RB < Ln) SF_BATCH(l0 + RB, vb, va);      // (uniform)
  }
#undef SF_BATCH
#undef SF_FETCH
  if (live) sf_lds[slot * d4 + q4] = acc;
  red[threadIdx.x] = lacc;
  __syncthreads();
  if (live && slot == 0) {
    for (int s2 = 1; s2 < slots; ++s2) {   // fixed order
      const float4 o = sf_lds[s2 * d4 + q4];
      acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w;
    }
    *(float4*)(dh + b * d + 4 * q4) = acc;
  }
  if (threadIdx.x == 0) {      // (the loss terms, in thread order)
    double a = 0.0;
    for (int t = 0; t < 256; ++t) a += red[t];
    if constexpr (DET) loss_acc[blockIdx.x] = a;
    else atomicAdd(loss_acc, a);
  }
}

// ------------------------------------------------------------------------------------------------
// backward kernels
// ------------------------------------------------------------------------------------------------
// dh[b,k] = sum_l ds[b,l] E[lookup[b,l], k];  SCATTER: also dE[lookup, k] += ds h[b,k], dbias[lookup] += ds by
// float atomics (the route for entity tables too large for the dense S matrix below)
// SHARD (k_tr_score_loss's comment; without SCATTER only): an entry of another shard is a (0, 0) addend with nothing loaded -- acc
// starts at +0 and no sum of this chain is -0, so fmaf(0, 0, acc) returns acc: the owned entries' chain in ascending l.
template <bool SCATTER, bool SHARD = false>
__global__ __launch_bounds__(256) void k_tr_score_bwd(const float* __restrict__ hv, const float* __restrict__ ent,
                                                      const int32_t* __restrict__ lookup, const float* __restrict__ ds,
                                                      int64_t E, int d, int64_t L, float* __restrict__ dh,
                                                      float* __restrict__ dE, float* __restrict__ dbias, int64_t sh_lo = 0,
                                                      int64_t sh_n = 0) {
  static_assert(!(SCATTER && SHARD), "the sharded step scatters nothing: its table gradient is k_ord_reduce's");
  const int64_t b = blockIdx.x;
  for (int k0 = 0; k0 < d; k0 += 256) {   // a thread per feature, 256 features at a time (d <= 256: one trip; 640: three)
  const int k = k0 + threadIdx.x;
  const float hk = k < d ? hv[b * d + k] : 0.f;
  float acc = 0.f;
  int64_t l = 0;
  // eight gathered rows in flight per thread: the loop is a chain of dependent loads otherwise (ids -> row)
  for (; l + 8 <= L; l += 8) {
    int64_t row[8];
    float g[8], ev[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      row[u] = lookup[b * L + l + u];
      if (row[u] < 0 || row[u] >= E) row[u] = 0;
      if constexpr (SHARD) {
        row[u] -= sh_lo;
        if (row[u] < 0 || row[u] >= sh_n) row[u] = -1;
        g[u] = row[u] >= 0 ? ds[b * L + l + u] : 0.f;
      } else
      g[u] = ds[b * L + l + u];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) ev[u] = (k < d && (!SHARD || row[u] >= 0)) ? ent[row[u] * d + k] : 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) {   // same summation order as the plain loop
      acc = fmaf(g[u], ev[u], acc);
      if (SCATTER) {
        if (k < d) atomicAdd(&dE[row[u] * d + k], g[u] * hk);
        if (k == 0) atomicAdd(&dbias[row[u]], g[u]);   // (k == 0 only in the first trip)
      }
    }
  }
  for (; l < L; ++l) {
    int64_t row = lookup[b * L + l];
    if (row < 0 || row >= E) row = 0;
    if constexpr (SHARD) {
      row -= sh_lo;
      if (row < 0 || row >= sh_n) continue;
    }
    const float g = ds[b * L + l];
    if (k < d) {
      acc = fmaf(g, ent[row * d + k], acc);
      if (SCATTER) atomicAdd(&dE[row * d + k], g * hk);
    }
    if (SCATTER && k == 0) atomicAdd(&dbias[row], g);
  }
  if (k < d) dh[b * d + k] = acc;
  }
}

// dh[b,:] = sum_l ds[b,l] E[lookup[b,l], :] without the scatter (the dense-route backward adds dE by a GEMM): the gather is
// bandwidth work -- B L rows of d floats (410 MB at 512 x 1000 x 200) -- and needs tens of KB in flight per CU: a thread owns
// four features (16-byte loads) of one of 256 / (d / 4) row slots, eight rows ahead, so a workgroup keeps 8 * slots rows
// (32 KB at d = 200) in flight; the slots' partial sums meet in LDS.  (The per-feature form with eight 4-byte loads in
// flight per thread read at 3.1 TB/s.)
// SHARD: as k_tr_score_bwd -- an entry of another shard is a (0, 0) addend with nothing loaded.
template <bool SHARD = false>
__global__ __launch_bounds__(256) void k_tr_dh_gather4(const float* __restrict__ ent, const int32_t* __restrict__ lookup,
                                                       const float* __restrict__ ds, int64_t E, int d, int64_t L,
                                                       float* __restrict__ dh, int64_t sh_lo = 0, int64_t sh_n = 0) {
  extern __shared__ float4 sh4[];   // [slots][d / 4]
  const int64_t b = blockIdx.x;
  const int d4 = d >> 2, slots = 256 / d4;
  const int slot = threadIdx.x / d4, q4 = threadIdx.x - slot * d4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (slot < slots) {
    const int32_t* lk = lookup + b * L;
    const float* gs = ds + b * L;
    int64_t l = slot;
    for (; l + 7 * slots < L; l += 8 * slots) {
      int64_t row[8];
      float g[8];
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        row[u] = lk[l + u * slots];
        if (row[u] < 0 || row[u] >= E) row[u] = 0;
        if constexpr (SHARD) {
          row[u] -= sh_lo;
          if (row[u] < 0 || row[u] >= sh_n) row[u] = -1;
          g[u] = row[u] >= 0 ? gs[l + u * slots] : 0.f;
        } else
        g[u] = gs[l + u * slots];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if constexpr (SHARD) v[u] = row[u] >= 0 ? *(const float4*)(ent + row[u] * d + 4 * q4) : make_float4(0.f, 0.f, 0.f, 0.f);
        else v[u] = *(const float4*)(ent + row[u] * d + 4 * q4);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        acc.x = fmaf(g[u], v[u].x, acc.x); acc.y = fmaf(g[u], v[u].y, acc.y);
        acc.z = fmaf(g[u], v[u].z, acc.z); acc.w = fmaf(g[u], v[u].w, acc.w);
      }
    }
    for (; l < L; l += slots) {
      int64_t row = lk[l];
      if (row < 0 || row >= E) row = 0;
      if constexpr (SHARD) {
        row -= sh_lo;
        if (row < 0 || row >= sh_n) continue;
      }
      const float g = gs[l];
      const float4 v = *(const float4*)(ent + row * d + 4 * q4);
      acc.x = fmaf(g, v.x, acc.x); acc.y = fmaf(g, v.y, acc.y); acc.z = fmaf(g, v.z, acc.z); acc.w = fmaf(g, v.w, acc.w);
    }
    sh4[slot * d4 + q4] = acc;
  }
  __syncthreads();
  if (slot == 0) {
    for (int s2 = 1; s2 < slots; ++s2) {   // fixed order
      const float4 o = sh4[s2 * d4 + q4];
      acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w;
    }
    *(float4*)(dh + b * d + 4 * q4) = acc;
  }
}

// dense route of the scorer backward (small entity tables): S[b, lookup[b,l]] += ds[b,l], dbias[lookup] += ds;
// then dE = S^T h is a GEMM instead of B*L*d float atomics.
// Round 6: S is built ROW BY ROW in LDS -- a workgroup per query zeroes a stretch of its row in LDS (<= TR_S_CHUNK columns),
// adds its L sampled gradients with LDS atomics, writes the stretch out coalesced and keeps its largest magnitude for the pack of S
// (tg_pack's max_slots) -- instead of B L float atomics into a zero-filled 30 MB matrix, a pass over it for its maximum and a
// zeroing launch share: k_tr_scatter_ds 54 us + k_tg_absmax_exp 18 + the zero list's 30 MB at FB15k-237 shapes.  dbias = the column
// sums of S (k_tr_col_sums_add).  Duplicate ids of a row add in the order the LDS serves them, as the global atomics did.
constexpr int TR_S_CHUNK = 32768;      // columns per LDS stretch (128 KB)
__global__ __launch_bounds__(256) void k_tr_build_S(const int32_t* __restrict__ lookup, const float* __restrict__ ds, int64_t E, int64_t L,
                                                    float* __restrict__ S, unsigned* __restrict__ max_slots) {
  extern __shared__ float s_row[];
  const int64_t b = blockIdx.x;
  const int32_t* lk = lookup + b * L;
  const float* g = ds + b * L;
  float mx = 0.f;
  for (int64_t c0 = 0; c0 < E; c0 += TR_S_CHUNK) {
    const int n = (int)(E - c0 < TR_S_CHUNK ? E - c0 : TR_S_CHUNK);
    for (int i = threadIdx.x; i < n; i += 256) s_row[i] = 0.f;
    __syncthreads();
    for (int64_t l = threadIdx.x; l < L; l += 256) {
      int64_t row = lk[l];
      if (row < 0 || row >= E) row = 0;
      if (row >= c0 && row < c0 + n) atomicAdd(&s_row[row - c0], g[l]);
    }
    __syncthreads();
    float* out = S + b * E + c0;
    for (int i = threadIdx.x; i < n; i += 256) {
      const float v = s_row[i];
      out[i] = v;
      mx = fmaxf(mx, fabsf(v));
    }
    __syncthreads();
  }
  tr_block_max_to_slot(mx, max_slots);
}

// out[c] += sum over rows of S[row, c]: row stretches of 64 per workgroup row, one float atomic per (stretch, column)
// DET: stretch z STORES its sums at out[z][cols] (a slab; k_tr_fold_f32_det adds the stretches in ascending z)
template <bool DET>
__global__ __launch_bounds__(256) void k_tr_col_sums_add(const float* __restrict__ S, int64_t rows, int64_t cols, float* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  const int64_t r0 = (int64_t)blockIdx.y * 64, r1 = r0 + 64 < rows ? r0 + 64 : rows;
  float a = 0.f;
  int64_t r = r0;
  for (; r + 8 <= r1; r += 8) {          // eight loads in flight (one at a time, a 64-row stretch was 64 dependent round trips: 17 - 20 us)
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = S[(r + u) * cols + c];
#pragma unroll
    for (int u = 0; u < 8; ++u) a += v[u];
  }
  for (; r < r1; ++r) a += S[r * cols + c];
  if constexpr (DET) { out[(size_t)blockIdx.y * cols + c] = a; return; }
  if (a != 0.f) atomicAdd(&out[c], a);
}

// out[i, j] += sum over rows b of w[b, i] v[b, j]   (a [ni x B] x [B x nj] product with a short ni: the generated dense bias'
// projection gradient dPb[rho, k] = sum_b c[b, rho] dz0[b, k]): a workgroup per (i, stretch of 64 rows), a thread per j
// DET: stretch z STORES its [ni, nj] partial product at out[z] (a slab; k_tr_fold_f32_det adds the stretches in ascending z)
template <bool DET>
__global__ __launch_bounds__(256) void k_tr_wsum_rows_add(const float* __restrict__ w, const float* __restrict__ v, int64_t rows, int ni, int nj,
                                                          float* __restrict__ out) {
  const int i = blockIdx.x;
  const int64_t r0 = (int64_t)blockIdx.y * 64, r1 = r0 + 64 < rows ? r0 + 64 : rows;
  for (int j = threadIdx.x; j < nj; j += 256) {
    float a = 0.f;
    int64_t r = r0;
    for (; r + 8 <= r1; r += 8) {
      float x[8], c[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { x[u] = v[(r + u) * nj + j]; c[u] = w[(r + u) * ni + i]; }
#pragma unroll
      for (int u = 0; u < 8; ++u) a = fmaf(c[u], x[u], a);
    }
    for (; r < r1; ++r) a = fmaf(w[r * ni + i], v[r * nj + j], a);
    if constexpr (DET) out[((size_t)blockIdx.y * ni + i) * nj + j] = a;
    else atomicAdd(&out[(int64_t)i * nj + j], a);
  }
}

// 1-vs-all training (lookup == NULL, models.py:159-162,434-437): S holds the logits h E^T from a GEMM; add the bias,
// accumulate the loss, overwrite with d(loss)/d(logit)
template <bool DET>
__global__ __launch_bounds__(256) void k_tr_dense_loss(float* __restrict__ S, const float* __restrict__ pred_bias,
                                                       const float* __restrict__ labels, int64_t E, int64_t total, float ls_eps,
                                                       float inv_E, float inv_BL, double* __restrict__ loss_acc) {
  __shared__ double part[256];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float s = S[i] + pred_bias[i % E];
    const float t = (1.f - ls_eps) * labels[i] + inv_E;
    acc += (double)(fmaxf(s, 0.f) - s * t + log1pf(expf(-fabsf(s))));
    S[i] = (1.f / (1.f + expf(-s)) - t) * inv_BL;
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if constexpr (DET) loss_acc[blockIdx.x] = part[0];
    else atomicAdd(loss_acc, part[0]);
  }
}

// out[c] = sum_b S[b, c]   (pred_bias gradient of the 1-vs-all route)
__global__ __launch_bounds__(256) void k_tr_col_sum_f32(const float* __restrict__ S, int64_t rows, int64_t cols, float* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  float a = 0.f;
  for (int64_t b = 0; b < rows; ++b) a += S[b * cols + c];
  out[c] = a;
}

// 1-vs-all training from SPARSE labels (coper_train_step_csr): k_tr_dense_loss on one chunk of entity columns [c0, c0 + w) of the
// logits, S [B, w], with the label of (sample b, column c) taken from MEMBERSHIP of c in the sample's sorted id list instead of a
// dense [B, |E|] matrix.  A workgroup per (sample, stretch of TR_CSR_STRETCH columns): two binary searches bound the row's entries
// inside the stretch, the lanes set their bits in an LDS bitmask (integer atomics), and the elementwise pass is a plain stream --
// 16 bytes per lane where the row stride allows it (vec: w % 4 == 0, S and the bias chunk 16-byte aligned), the four label bits of a
// lane from one LDS word that eight neighbouring lanes read together (a broadcast: no bank conflict).  The work of a row with
// thousands of positives and of an empty one differs by the bit-setting loop only.  Ids outside the stretch -- so every id outside
// [0, |E|) -- set nothing; a lab_row outside the table is an empty row.  Per element the expression is k_tr_dense_loss's.
constexpr int TR_CSR_STRETCH = 2048;      // columns per workgroup: a 64-word bitmask, two 16-byte accesses per lane
template <bool DET>
__global__ __launch_bounds__(256) void k_tr_csr_loss(float* __restrict__ S, const float* __restrict__ pred_bias_c /* + c0 */,
                                                     const int64_t* __restrict__ indptr, const int64_t* __restrict__ idx,
                                                     const int64_t* __restrict__ lab_row, int64_t n_rows, int64_t c0, int64_t w,
                                                     int64_t n_stretch, int vec, float ls_eps, float inv_E, float inv_BL,
                                                     double* __restrict__ loss_acc) {
  __shared__ unsigned mask[TR_CSR_STRETCH / 32];
  __shared__ double part[256];
  const int tid = threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x / n_stretch, j0 = ((int64_t)blockIdx.x % n_stretch) * TR_CSR_STRETCH;
  const int n = (int)(w - j0 < TR_CSR_STRETCH ? w - j0 : TR_CSR_STRETCH);
  const int64_t g0 = c0 + j0;      // the entity of the stretch's first column
  if (tid < TR_CSR_STRETCH / 32) mask[tid] = 0u;
  const int64_t row = lab_row ? lab_row[b] : b;
  int64_t lo = 0, hi = 0;
  if (row >= 0 && row < n_rows) { lo = indptr[row]; hi = indptr[row + 1]; }
  auto lower_bound = [&](int64_t key) {      // the first entry of [lo, hi) that is >= key
    int64_t a = lo, z = hi;
    while (a < z) {
      const int64_t m = a + ((z - a) >> 1);
      if (idx[m] < key) a = m + 1; else z = m;
    }
    return a;
  };
  const int64_t p0 = lower_bound(g0), p1 = lower_bound(g0 + n);
  __syncthreads();
  for (int64_t p = p0 + tid; p < p1; p += 256) {
    const int64_t e = idx[p] - g0;
    if (e >= 0 && e < n) atomicOr(&mask[e >> 5], 1u << (e & 31));
  }
  __syncthreads();
  float* const Sr = S + b * w + j0;
  const float* const pb = pred_bias_c + j0;
  double acc = 0.0;
  auto element = [&](float logit, float bias, unsigned bit) {
    const float s = logit + bias;
    const float t = (1.f - ls_eps) * (bit ? 1.f : 0.f) + inv_E;
    acc += (double)(fmaxf(s, 0.f) - s * t + log1pf(expf(-fabsf(s))));
    return (1.f / (1.f + expf(-s)) - t) * inv_BL;
  };
  if (vec) {
    for (int j = tid * 4; j < n; j += 1024) {      // (n % 4 == 0 with w % 4 == 0)
      float4 v = *reinterpret_cast<const float4*>(Sr + j);
      const float4 bb = *reinterpret_cast<const float4*>(pb + j);
      const unsigned bits = mask[j >> 5] >> (j & 31);
      v.x = element(v.x, bb.x, bits & 1u);
      v.y = element(v.y, bb.y, bits & 2u);
      v.z = element(v.z, bb.z, bits & 4u);
      v.w = element(v.w, bb.w, bits & 8u);
      *reinterpret_cast<float4*>(Sr + j) = v;
    }
  } else {
    for (int j = tid; j < n; j += 256) Sr[j] = element(Sr[j], pb[j], (mask[j >> 5] >> (j & 31)) & 1u);
  }
  part[tid] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    if constexpr (DET) loss_acc[blockIdx.x] = part[0];
    else atomicAdd(loss_acc, part[0]);
  }
}
// out[b, c0 + j] = S[b, j] + pred_bias[c0 + j]: a chunk's logits into the [B, |E|] pred_out of coper_train_forward_csr (E: the row
// stride of out -- the handle's own rows, n_local, on an entity shard: coper_train_shard_forward_csr's pred_local)
__global__ __launch_bounds__(256) void k_tr_add_bias_out_cols(const float* __restrict__ S, const float* __restrict__ pred_bias_c, int64_t w,
                                                              int64_t total, int64_t E, float* __restrict__ out_c /* + c0 */) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total) out_c[(i / w) * E + i % w] = S[i] + pred_bias_c[i % w];
}
// dst += src: a later chunk's share of dh, added in chunk order
__global__ __launch_bounds__(256) void k_tr_add_to(float* __restrict__ dst, const float* __restrict__ src, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] += src[i];
}

// ---- g_MLP generator chain pieces (small matrices: B <= a few thousand, widths <= a few hundred)
// out[b,j] = sum_i in[b,i] P[i,j]
__global__ __launch_bounds__(256) void k_tr_small_mm(const float* __restrict__ in, const float* __restrict__ P, int64_t B, int ni, int nj,
                                                     float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * nj) return;
  const int64_t b = idx / nj;
  const int j = (int)(idx % nj);
  float a = 0.f;
  for (int i = 0; i < ni; ++i) a = fmaf(in[b * ni + i], P[(int64_t)i * nj + j], a);
  out[idx] = a;
}
// dv[b,i] (+)= sum_j du[b,j] P[i,j]
__global__ __launch_bounds__(256) void k_tr_small_mm_nt(const float* __restrict__ du, const float* __restrict__ P, int64_t B, int ni, int nj,
                                                        int accumulate, float* __restrict__ dv) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * ni) return;
  const int64_t b = idx / ni;
  const int i = (int)(idx % ni);
  float a = accumulate ? dv[idx] : 0.f;
  for (int j = 0; j < nj; ++j) a = fmaf(du[b * nj + j], P[(int64_t)i * nj + j], a);
  dv[idx] = a;
}
// dP[i,j] = sum_b v[b,i] du[b,j]   (one thread per entry; B is small)
__global__ __launch_bounds__(256) void k_tr_small_mm_tn(const float* __restrict__ v, const float* __restrict__ du, int64_t B, int ni, int nj,
                                                        float* __restrict__ dP) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)ni * nj) return;
  const int i = (int)(idx / nj), j = (int)(idx % nj);
  float a = 0.f;
  for (int64_t b = 0; b < B; ++b) a = fmaf(v[b * ni + i], du[b * nj + j], a);
  dP[idx] = a;
}
// a = relu(BN(u)) (or relu(u) when the generator has no BN); v_next = dropout(a)
__global__ __launch_bounds__(256) void k_tr_chain_act(const float* __restrict__ u, const float* __restrict__ st, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, int n, int64_t total, uint32_t seed, uint32_t step, uint32_t ioff,
                                                      uint32_t stage, uint32_t thr, float keep_scale, float* __restrict__ a,
                                                      float* __restrict__ vnext) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int k = (int)(i % n);
  float v = u[i];
  if (gamma) v = (v - st[k]) * st[n + k] * gamma[k] + beta[k];
  v = v > 0.f ? v : 0.f;
  a[i] = v;
  vnext[i] = dropout_keep_u32(seed, step, stage, (uint32_t)i + ioff, thr) ? v * keep_scale : 0.f;
}
// g = keep * dv_next / (1 - rate)   (dropout backward; the ReLU / BN part is k_tr_fcbn_bwd)
__global__ __launch_bounds__(256) void k_tr_chain_drop_bwd(const float* __restrict__ dvn, int64_t total, uint32_t seed, uint32_t step, uint32_t ioff,
                                                           uint32_t stage, uint32_t thr, float keep_scale, float* __restrict__ g) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  g[i] = dropout_keep_u32(seed, step, stage, (uint32_t)i + ioff, thr) ? dvn[i] * keep_scale : 0.f;
}
__global__ __launch_bounds__(256) void k_tr_add(const float* __restrict__ a, int64_t n, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] += a[i];
}

// ---- g_lookup dense layer (ParameterLookup, models.py:79-94): W = table[rel[b]] of shape [F, d], per sample
// forward partials: part[sl][b][k] = sum_{f in slice sl} x[b,f] W[rel[b]][f,k]     (grid: B x NSL, thread = k)
__global__ __launch_bounds__(256) void k_tr_lookup_fwd(const float* __restrict__ x, const float* __restrict__ Wt,
                                                       const int64_t* __restrict__ rel, int64_t R, int64_t F, int d, int nsl,
                                                       int64_t B, float* __restrict__ part) {
  extern __shared__ float xs[];
  const int64_t b = blockIdx.x;
  const int sl = blockIdx.y;
  const int64_t f0 = F * sl / nsl, f1 = F * (sl + 1) / nsl;
  int64_t rid = rel[b];
  if (rid < 0 || rid >= R) rid = 0;
  for (int64_t f = f0 + threadIdx.x; f < f1; f += 256) xs[f - f0] = x[b * F + f];
  __syncthreads();
  const int k = threadIdx.x;
  if (k >= d) return;
  const float* W = Wt + (rid * F + f0) * d + k;
  float a = 0.f;
  for (int64_t f = 0; f < f1 - f0; ++f) a = fmaf(xs[f], W[f * d], a);
  part[((int64_t)sl * B + b) * d + k] = a;
}
// dW[r][f,k] = sum_{b: rel[b] = r} x[b,f] dz[b,k]   (grid: F-chunks x R; relations absent from the batch are skipped:
// their rows keep stale values and the optimiser kernels treat them as zero through the row mask)
__global__ __launch_bounds__(256) void k_tr_lookup_dW(const float* __restrict__ x, const float* __restrict__ dz,
                                                      const int32_t* __restrict__ perm, const int32_t* __restrict__ offset,
                                                      const int32_t* __restrict__ count, int64_t F, int d, int rows_per_wg,
                                                      float* __restrict__ dWt) {
  const int64_t r = blockIdx.y;
  const int n = count[r];
  if (n == 0) return;
  const int off = offset[r];
  const int k = threadIdx.x;
  if (k >= d) return;
  const int64_t f0 = (int64_t)blockIdx.x * rows_per_wg;
  for (int64_t f = f0; f < f0 + rows_per_wg && f < F; ++f) {
    float a = 0.f;
    for (int j = 0; j < n; ++j) {
      const int64_t b = perm[off + j];
      a = fmaf(x[b * F + f], dz[b * d + k], a);
    }
    dWt[(r * F + f) * d + k] = a;
  }
}
// dx[b,f] = sum_k dz[b,k] W[rel[b]][f,k]   (one wave per row f, lanes over k)
__global__ __launch_bounds__(256) void k_tr_lookup_dx(const float* __restrict__ dz, const float* __restrict__ Wt,
                                                      const int64_t* __restrict__ rel, int64_t R, int64_t F, int d,
                                                      float* __restrict__ dx) {
  extern __shared__ float dzs[];
  const int64_t b = blockIdx.y;
  int64_t rid = rel[b];
  if (rid < 0 || rid >= R) rid = 0;
  for (int k = threadIdx.x; k < d; k += 256) dzs[k] = dz[b * d + k];
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int64_t f = (int64_t)blockIdx.x * 64 + wave; f < F && f < (int64_t)(blockIdx.x + 1) * 64; f += 4) {
    const float* W = Wt + (rid * F + f) * d;
    float a = 0.f;
    for (int k = lane; k < d; k += 64) a = fmaf(dzs[k], W[k], a);
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if (lane == 0) dx[b * F + f] = a;
  }
}
// z1 = keep * (sum of the forward partials + bias_table[rel[b]]) / (1 - rate)
__global__ __launch_bounds__(256) void k_tr_lookup_post(const float* __restrict__ part, int nsl, const float* __restrict__ bias_t,
                                                        const int64_t* __restrict__ rel, int64_t R, int d, int64_t total,
                                                        uint32_t seed, uint32_t step, uint32_t ioff, uint32_t thr, float keep_scale,
                                                        float* __restrict__ z1) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  int64_t rid = rel[i / d];
  if (rid < 0 || rid >= R) rid = 0;
  float v = bias_t[rid * d + i % d];
  for (int sl = 0; sl < nsl; ++sl) v += part[(int64_t)sl * total + i];
  z1[i] = dropout_keep_u32(seed, step, 2u, (uint32_t)i + ioff, thr) ? v * keep_scale : 0.f;
}
// dz0 = keep * dz1 / (1 - rate) (in place);  dbias_table[rel[b], k] += dz0[b,k]   (DET: the rows are added by k_tr_rows_by_key_det)
template <bool DET>
__global__ __launch_bounds__(256) void k_tr_lookup_post_bwd(float* __restrict__ dz, const int64_t* __restrict__ rel, int64_t R, int d,
                                                            int64_t total, uint32_t seed, uint32_t step, uint32_t ioff, uint32_t thr,
                                                            float keep_scale, float* __restrict__ dbias_t) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  int64_t rid = rel[i / d];
  if (rid < 0 || rid >= R) rid = 0;
  const float v = dropout_keep_u32(seed, step, 2u, (uint32_t)i + ioff, thr) ? dz[i] * keep_scale : 0.f;
  dz[i] = v;
  if constexpr (!DET) atomicAdd(&dbias_t[rid * d + i % d], v);
}

// FCBN backward, one workgroup per feature k (a column of [B, d]): gamma/beta gradients and dz1
// (dh and dz1 may be the same buffer: every element is read, then written, by one thread)
__global__ __launch_bounds__(256) void k_tr_fcbn_bwd(const float* __restrict__ z1, const float* __restrict__ hv, const float* dh,
                                                     const float* __restrict__ mean, const float* __restrict__ inv,
                                                     const float* __restrict__ gamma, int64_t B, int d, int use_batch,
                                                     float* __restrict__ dgamma, float* __restrict__ dbeta, float* dz1) {
  __shared__ double s1[256], s2[256];
  const int k = blockIdx.x;
  if (!mean) {   // generator layer without BN: ReLU only
    for (int64_t b = threadIdx.x; b < B; b += 256) dz1[b * d + k] = hv[b * d + k] > 0.f ? dh[b * d + k] : 0.f;
    return;
  }
  const float mu = mean[k], iv = inv[k], ga = gamma[k];
  double a1 = 0, a2 = 0;
  for (int64_t b = threadIdx.x; b < B; b += 256) {
    const float g = hv[b * d + k] > 0.f ? dh[b * d + k] : 0.f;   // through the ReLU
    const float zh = (z1[b * d + k] - mu) * iv;
    a1 += g;
    a2 += (double)g * zh;
  }
  s1[threadIdx.x] = a1; s2[threadIdx.x] = a2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { s1[threadIdx.x] += s1[threadIdx.x + o]; s2[threadIdx.x] += s2[threadIdx.x + o]; }
    __syncthreads();
  }
  const double S1 = s1[0], S2 = s2[0];
  if (threadIdx.x == 0) { dbeta[k] = (float)S1; dgamma[k] = (float)S2; }
  for (int64_t b = threadIdx.x; b < B; b += 256) {
    const float g = hv[b * d + k] > 0.f ? dh[b * d + k] : 0.f;
    const float zh = (z1[b * d + k] - mu) * iv;
    float dz;
    if (use_batch) dz = (float)((double)ga * iv * ((double)g - S1 / (double)B - (double)zh * S2 / (double)B));
    else dz = ga * iv * g;
    dz1[b * d + k] = dz;
  }
}

// The two halves of k_tr_fcbn_bwd for a step whose batch statistics span several ranks (coper_train_sync_*): the sums of
// this rank's rows leave the kernel, the caller's exchange adds the ranks', the second half applies the formula with the sums of the
// WHOLE batch.  The same thread-to-row assignment and the same LDS tree as k_tr_fcbn_bwd, so one rank alone reproduces its bits.
// sums [2 d] doubles: sum of g | sum of g z_hat.
__global__ __launch_bounds__(256) void k_tr_fcbn_bwd_sums(const float* __restrict__ z1, const float* __restrict__ hv, const float* __restrict__ dh,
                                                          const float* __restrict__ mean, const float* __restrict__ inv, int64_t B, int d,
                                                          double* __restrict__ sums) {
  __shared__ double s1[256], s2[256];
  const int k = blockIdx.x;
  const float mu = mean[k], iv = inv[k];
  double a1 = 0, a2 = 0;
  for (int64_t b = threadIdx.x; b < B; b += 256) {
    const float g = hv[b * d + k] > 0.f ? dh[b * d + k] : 0.f;   // through the ReLU
    const float zh = (z1[b * d + k] - mu) * iv;
    a1 += g;
    a2 += (double)g * zh;
  }
  s1[threadIdx.x] = a1; s2[threadIdx.x] = a2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { s1[threadIdx.x] += s1[threadIdx.x + o]; s2[threadIdx.x] += s2[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { sums[k] = s1[0]; sums[d + k] = s2[0]; }
}
// all: the sums over the whole batch of n samples (the dz1 formula);  own: this rank's (its share of the gamma / beta gradients -- the
// caller's all-reduce of the gradients adds the ranks' shares, so the whole batch's sums here would count every rank G times)
// (dh and dz1 may be the same buffer, as in k_tr_fcbn_bwd)
__global__ __launch_bounds__(256) void k_tr_fcbn_bwd_apply(const float* __restrict__ z1, const float* __restrict__ hv, const float* dh,
                                                           const float* __restrict__ mean, const float* __restrict__ inv,
                                                           const float* __restrict__ gamma, int64_t B, int d, double n,
                                                           const double* __restrict__ all, const double* __restrict__ own,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta, float* dz1) {
  const int k = blockIdx.x;
  const float mu = mean[k], iv = inv[k], ga = gamma[k];
  const double S1 = all[k], S2 = all[d + k];
  if (threadIdx.x == 0) { dbeta[k] = (float)own[k]; dgamma[k] = (float)own[d + k]; }
  for (int64_t b = threadIdx.x; b < B; b += 256) {
    const float g = hv[b * d + k] > 0.f ? dh[b * d + k] : 0.f;
    const float zh = (z1[b * d + k] - mu) * iv;
    dz1[b * d + k] = (float)((double)ga * iv * ((double)g - S1 / n - (double)zh * S2 / n));
  }
}
// out[j] = parts[0][j] + parts[1][j] + ... in ascending g: the ranks' shares of a batch-wide sum as the caller gathered them, [G][n].
// Every rank folds the same buffer in the same order, so every rank holds the same bits; one part alone passes through unchanged.
__global__ __launch_bounds__(256) void k_tr_fold_parts(const double* __restrict__ parts, int G, int n, double* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  double a = parts[j];
  for (int g = 1; g < G; ++g) a += parts[(size_t)g * n + j];
  out[j] = a;
}

// dz0 = keep * dz1 / (1 - rate) (in place); dense-bias gradients: static dfc_bias[k] += dz0; generated
// dPb[rho,k] += c[b,rho] dz0[b,k], dc[b,rho] = sum_k dz0[b,k] Pb[rho,k]   (DET: dfc_bias is the column sum of dz0, a launch of its own)
template <bool DET>
__global__ __launch_bounds__(256) void k_tr_fc_post_bwd(float* __restrict__ dz, const float* __restrict__ c,
                                                        const float* __restrict__ Pb, int r, int d, uint32_t seed,
                                                        uint32_t step, uint32_t ioff, uint32_t thr, float keep_scale,
                                                        float* __restrict__ dfc_bias, float* __restrict__ dPb,
                                                        float* __restrict__ dc) {
  extern __shared__ float row[];  // dz0[b, :]
  const int64_t b = blockIdx.x;
  for (int k = threadIdx.x; k < d; k += 256) {
    const int64_t i = b * d + k;
    const float v = dropout_keep_u32(seed, step, 2u, (uint32_t)i + ioff, thr) ? dz[i] * keep_scale : 0.f;
    dz[i] = v;
    row[k] = v;
    if constexpr (!DET)
    if (!Pb) atomicAdd(&dfc_bias[k], v);
  }
  __syncthreads();
  if (Pb) {
    // (dPb[rho, k] = sum_b c[b, rho] dz0[b, k] is a small product of its own behind this kernel since round 6: B workgroups adding
    //  r d values each to the same r d addresses took 32 us)
    for (int rho = threadIdx.x; rho < r; rho += 256) {
      float a = 0.f;
      for (int k = 0; k < d; ++k) a = fmaf(row[k], Pb[rho * d + k], a);
      dc[b * r + rho] = a;
    }
  }
}

// dT[rho][b,k] = c[b,rho] dz[b,k]   (operand of the batched weight-gradient GEMM dP[rho] = x^T dT[rho])
__global__ __launch_bounds__(256) void k_tr_scale_rows(const float* __restrict__ dz, const float* __restrict__ c, int r, int d,
                                                       int64_t total, float* __restrict__ dT, unsigned* __restrict__ max_slots) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float mx = 0.f;
  if (i < total) {
    const int64_t b = i / d;
    const float g = dz[i];
    for (int rho = 0; rho < r; ++rho) {
      const float v = c[b * r + rho] * g;
      dT[(int64_t)rho * total + i] = v;
      mx = fmaxf(mx, fabsf(v));
    }
  }
  if (max_slots) tr_block_max_to_slot(mx, max_slots);
}

// dx[b,f] = sum_rho c[b,rho] dA[b,rho*F+f];  dc[b,rho] += sum_f x[b,f] dA[b,rho*F+f]
// dx[b, f] = sum_rho c[b, rho] dA[b, rho, f]   (one pass over dA, eight loads in flight)

// dc[b, rho] = sum_k dz[b, k] T[rho][b][k]: z[b] = sum_rho c[b, rho] T[rho][b] with the forward partials T = x P[rho]
// still in place, so the context gradient needs no second pass over dA.  One wave per (b, rho).
__global__ __launch_bounds__(256) void k_tr_dc_from_partials(const float* __restrict__ dz, const float* __restrict__ Tf, int64_t B, int r,
                                                             int d, float* __restrict__ dc) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= B * r) return;
  const int64_t b = w / r;
  const int rho = (int)(w - b * r);
  const float* t = Tf + ((int64_t)rho * B + b) * d;
  const float* g = dz + b * d;
  float a = 0.f;
  for (int k = lane; k < d; k += 64) a = fmaf(g[k], t[k], a);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o);
  if (lane == 0) dc[b * r + rho] = a;
}

// Conv1BN backward, pass 1: g = dx * keep/(1-rate) through the ReLU; per-channel sums of g and g*yhat
// (dbeta, dgamma).  g overwrites dx.
// NS > 0 (round 6): dx arrives as the NS K slices of its product (tg_gemm_nt: leave_slices), added here in slice order -- the slice sum's
// launch, its store of dx and this kernel's read of it are gone.
template <int NS>
__global__ __launch_bounds__(256) void k_tr_bn1_bwd_sums(float* __restrict__ dx, const float* __restrict__ part, const float* __restrict__ y,
                                                         const float* __restrict__ mean, const float* __restrict__ inv,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, int C,
                                                         int64_t total, uint32_t seed, uint32_t step, uint32_t ioff, uint32_t thr,
                                                         float keep_scale, double* __restrict__ sums, int nslots) {
  __shared__ double s1[256], s2[256];
  sums += (size_t)(blockIdx.x % nslots) * 2 * C;      // (TR_CS_SLOTS copies: k_tr_col_sums)
  auto dx_in = [&](int64_t i) -> float {
    if constexpr (NS == 0) {
      return dx[i];
    } else {
      float t[NS];
#pragma unroll
      for (int z = 0; z < NS; ++z) t[z] = part[(int64_t)z * total + i];
      float a = 0.f;
#pragma unroll
      for (int z = 0; z < NS; ++z) a += t[z];      // slice order, as k_tg_reduce
      return a;
    }
  };
  if (256 % C != 0) {
    // channel counts that do not divide the workgroup: a thread meets every channel, so the channel sums are built in LDS
    // (C <= 256 doubles per array) with one LDS atomic pair per element, then added to the global sums
    for (int c = threadIdx.x; c < C; c += 256) { s1[c] = 0; s2[c] = 0; }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
      const int c = (int)(i % C);
      const float yh = (y[i] - mean[c]) * inv[c];
      const float act = yh * gamma[c] + beta[c];
      float g = dropout_keep_u32(seed, step, 1u, (uint32_t)i + ioff, thr) ? dx_in(i) * keep_scale : 0.f;
      if (!(act > 0.f)) g = 0.f;
      dx[i] = g;
      atomicAdd(&s1[c], (double)g);
      atomicAdd(&s2[c], (double)g * yh);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
      atomicAdd(&sums[c], s1[c]);
      atomicAdd(&sums[C + c], s2[c]);
    }
    return;
  }
  double a1 = 0, a2 = 0;
  // grid-stride: 256 % C == 0, so a thread stays on one channel and the channel sums are built in registers
  const int64_t st = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)(i % C);
  const float mc = mean[c], ic = inv[c], gc = gamma[c], bc = beta[c];
  for (; i + 3 * st < total; i += 4 * st) {          // four load pairs in flight (one at a time: 20 dependent round trips, 40 us)
    float yv[4], dv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { yv[u] = y[i + u * st]; dv[u] = dx_in(i + u * st); }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float yh = (yv[u] - mc) * ic;
      const float act = yh * gc + bc;
      float g = dropout_keep_u32(seed, step, 1u, (uint32_t)(i + u * st) + ioff, thr) ? dv[u] * keep_scale : 0.f;
      if (!(act > 0.f)) g = 0.f;
      dx[i + u * st] = g;
      a1 += g;
      a2 += (double)g * yh;
    }
  }
  for (; i < total; i += st) {
    const float yh = (y[i] - mc) * ic;
    const float act = yh * gc + bc;
    float g = dropout_keep_u32(seed, step, 1u, (uint32_t)i + ioff, thr) ? dx_in(i) * keep_scale : 0.f;
    if (!(act > 0.f)) g = 0.f;
    dx[i] = g;
    a1 += g;
    a2 += (double)g * yh;
  }
  // 256 % C == 0 here: threads with the same (threadIdx.x % C) share a channel
  s1[threadIdx.x] = a1; s2[threadIdx.x] = a2;
  __syncthreads();
  for (int o = 128; o >= C; o >>= 1) {
    if ((int)threadIdx.x < o) { s1[threadIdx.x] += s1[threadIdx.x + o]; s2[threadIdx.x] += s2[threadIdx.x + o]; }
    __syncthreads();
  }
  if ((int)threadIdx.x < C) {
    const int c = (int)(((int64_t)blockIdx.x * 256 + threadIdx.x) % C);
    atomicAdd(&sums[c], s1[threadIdx.x]);
    atomicAdd(&sums[C + c], s2[threadIdx.x]);
  }
}

// pass 2: dy = gamma*inv*(g - S1/n - yhat*S2/n) (batch statistics) or gamma*inv*g; in place on dx
// sums: S1 | S2 over the n positions the statistics were taken over;  own: the sums of this launch's rows, the gamma / beta gradients
// (one buffer for both but in a step whose statistics span several ranks, DESIGN 6.13: the ranks' gradients are added afterwards)
__global__ __launch_bounds__(256) void k_tr_bn1_bwd_apply(float* __restrict__ dx, const float* __restrict__ y,
                                                          const float* __restrict__ mean, const float* __restrict__ inv,
                                                          const float* __restrict__ gamma, const double* __restrict__ sums,
                                                          const double* __restrict__ own, int C,
                                                          int64_t total, double n, int use_batch, float* __restrict__ dgamma,
                                                          float* __restrict__ dbeta) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < C) { dbeta[i] = (float)own[i]; dgamma[i] = (float)own[C + i]; }
  if (i >= total) return;
  const int c = (int)(i % C);
  const float g = dx[i];
  if (use_batch) {
    const float yh = (y[i] - mean[c]) * inv[c];
    dx[i] = (float)((double)gamma[c] * inv[c] * ((double)g - sums[c] / n - (double)yh * sums[C + c] / n));
  } else {
    dx[i] = gamma[c] * inv[c] * g;
  }
}

// conv backward, one workgroup per query: the query's filter / bias gradients dK_ps[b], dkb_ps[b] (reduced by the caller: through the
// generators / tables, or -- static filters -- by column sums), d(img) -> rows of dE / drel_emb
// DET: d(img) is STORED per query at dE[b][isz] (a workspace, not the gradient); k_tr_rows_by_key_det adds the rows per entity / relation
template <bool DET>
__global__ __launch_bounds__(256) void k_tr_conv_bwd(const float* __restrict__ dy, const float* __restrict__ img_all,
                                                     const float* __restrict__ K, const int64_t* __restrict__ e1,
                                                     const int64_t* __restrict__ rel, int64_t E, int64_t R, int d, int r,
                                                     int in_h, int in_w, int stacked, int C, int Ho, int Wo,
                                                     float* __restrict__ dE, float* __restrict__ drel,
                                                     const float* __restrict__ K_ps, float* __restrict__ dK_ps,
                                                     float* __restrict__ dkb_ps, int fh, int fw) {
  extern __shared__ float lds[];  // img[isz] | g[P][C + 1] | taps[fh*fw*C]
  // (round 6: a pixel's C gradients are C + 1 words apart -- the image-gradient loop below has every lane on another PIXEL and the
  //  same channel: with a stride of C = 32 words all 64 lanes sat on one LDS bank, 45 of this kernel's 60 us)
  const int isz = in_h * in_w, P = Ho * Wo, nt = fh * fw, CS = C + 1;
  float* img = lds;
  float* g = img + isz;
  float* taps = g + P * CS;
  const int64_t b = blockIdx.x;
  for (int t = threadIdx.x; t < isz; t += 256) img[t] = img_all[b * isz + t];
  for (int t = threadIdx.x; t < P * C; t += 256) g[(t / C) * CS + (t % C)] = dy[b * (int64_t)P * C + t];
  const float* Ksrc = K_ps ? K_ps + b * (int64_t)nt * C : K;
  for (int t = threadIdx.x; t < nt * C; t += 256) taps[t] = Ksrc[t];
  __syncthreads();
  // filter and bias gradients: entry (tap, c) = sum_p img[p + tap offset] * g[p, c]
  for (int idx = threadIdx.x; idx < (nt + 1) * C; idx += 256) {
    const int cc = idx % C, tap = idx / C;
    float a = 0.f;
    if (tap < nt) {
      const int u = tap / fw, v = tap % fw;
      // (the trip counts are run-time values: without the unrolls every iteration waits out its own two LDS reads -- with two
      //  waves per SIMD this kernel was LDS latency end to end, 31 us)
      for (int i = 0; i < Ho; ++i) {
        const float* ir = img + (i + u) * in_w + v;
        const float* gr = g + (i * Wo) * CS + cc;
#pragma unroll 6
        for (int j = 0; j < Wo; ++j) a = fmaf(ir[j], gr[j * CS], a);
      }
      dK_ps[b * (int64_t)nt * C + tap * C + cc] = a;
    } else {
#pragma unroll 8
      for (int p = 0; p < P; ++p) a += g[p * CS + cc];
      dkb_ps[b * C + cc] = a;
    }
  }
  // image gradient (full correlation), scattered to the embedding rows
  int64_t row = e1[b];
  if (row < 0 || row >= E) row = 0;
  int64_t rid = rel[b];
  if (rid < 0 || rid >= R) rid = 0;
  for (int t = threadIdx.x; t < isz; t += 256) {
    const int ii = t / in_w, jj = t - ii * in_w;
    float a = 0.f;
    for (int u = 0; u < fh; ++u) {
      const int i = ii - u;
      if (i < 0 || i >= Ho) continue;
      for (int v = 0; v < fw; ++v) {
        const int j = jj - v;
        if (j < 0 || j >= Wo) continue;
        const float* gp = g + (i * Wo + j) * CS;
        const float* tp = taps + (u * fw + v) * C;
#pragma unroll 8
        for (int cc = 0; cc < C; ++cc) a = fmaf(gp[cc], tp[cc], a);
      }
    }
    if constexpr (DET) dE[b * isz + t] = a;
    else {
    if (t < d) atomicAdd(&dE[row * d + t], a);
    else if (stacked) atomicAdd(&drel[rid * r + (t - d)], a);
    }
  }
}

// out[b, :] = table[rel[b], :]   (relation rows; also the per-sample conv filters of g_lookup)
__global__ __launch_bounds__(256) void k_tr_gather_rows(const float* __restrict__ table, const int64_t* __restrict__ rel, int64_t R, int n,
                                                        int64_t total, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  int64_t rid = rel[i / n];
  if (rid < 0 || rid >= R) rid = 0;
  out[i] = table[rid * n + i % n];
}

// concat_rel (models.py:406-407): xc[b] = [x[b] | c[b]], after the hidden dropout
__global__ __launch_bounds__(256) void k_tr_concat(const float* __restrict__ x, const float* __restrict__ c, int64_t Fc, int r, int64_t total,
                                                   float* __restrict__ xc) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t b = i / (Fc + r), f = i - b * (Fc + r);
  xc[i] = f < Fc ? x[b * Fc + f] : c[b * r + (f - Fc)];
}

// ... and back: dx[b] = dxc[b, :Fc];  drel_emb[rel[b], :] += dxc[b, Fc:]   (DET: the second half by k_tr_rows_by_key_det)
template <bool DET>
__global__ __launch_bounds__(256) void k_tr_split(const float* __restrict__ dxc, const int64_t* __restrict__ rel, int64_t R, int64_t Fc, int r,
                                                  int64_t total, float* __restrict__ dx, float* __restrict__ drel) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t b = i / (Fc + r), f = i - b * (Fc + r);
  if (f < Fc) { dx[b * Fc + f] = dxc[i]; return; }
  if constexpr (DET) return;
  int64_t rid = rel[b];
  if (rid < 0 || rid >= R) rid = 0;
  atomicAdd(&drel[rid * r + (f - Fc)], dxc[i]);
}

// drel_emb[rel[b], :] += dc[b, :]
__global__ __launch_bounds__(256) void k_tr_scatter_rows(const float* __restrict__ dc, const int64_t* __restrict__ rel, int64_t R,
                                                         int r, int64_t total, float* __restrict__ drel) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  int64_t rid = rel[i / r];
  if (rid < 0 || rid >= R) rid = 0;
  atomicAdd(&drel[rid * r + i % r], dc[i]);
}

// every trainable tensor in one launch (blockIdx.y = tensor): the small ones would otherwise cost a launch each
struct TrainTensors {
  float* p[TR_MAX_PARAMS];
  float* g[TR_MAX_PARAMS];
  float* m[TR_MAX_PARAMS];
  float* v[TR_MAX_PARAMS];
  float* vh[TR_MAX_PARAMS];
  int64_t n[TR_MAX_PARAMS];
  // tensors whose gradient rows exist only for keys present in the batch (g_lookup tables): row length and the
  // per-key count; a row with count 0 has gradient 0 whatever the buffer holds
  int64_t rowlen[TR_MAX_PARAMS];
  const int32_t* rowcnt[TR_MAX_PARAMS];
  unsigned* wmax;     // TG_MAX_SLOTS slots for max |p_new| of tensor wmax_of (-1: none)
  int wmax_of;
};

// DET: workgroup (x, y) STORES its sum at acc[y * gridDim.x + x] (a slab; k_tr_fold_det adds them into slot 0 of the squared-norm slots)
template <bool DET>
__global__ __launch_bounds__(256) void k_tr_sumsq(TrainTensors tt, int skip, double* __restrict__ acc) {
  __shared__ double part[256];
  if ((int)blockIdx.y == skip) return;   // the GEMM that produced this gradient already added its squares
  const float* g = tt.g[blockIdx.y];
  const int64_t n = tt.n[blockIdx.y];
  double a = 0;
  const int32_t* rc = tt.rowcnt[blockIdx.y];
  const int64_t rl = tt.rowlen[blockIdx.y];
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (!rc && ((uintptr_t)g & 15) == 0) {
    // 16-byte loads, four in flight per thread; the scalar loop below takes what is left
    const int64_t n4 = n >> 2;
    const float4* g4 = (const float4*)g;
    int64_t j = i;
    for (; j + 3 * stride < n4; j += 4 * stride) {
      const float4 v0 = g4[j], v1 = g4[j + stride], v2 = g4[j + 2 * stride], v3 = g4[j + 3 * stride];
      a += (double)v0.x * v0.x + (double)v0.y * v0.y + (double)v0.z * v0.z + (double)v0.w * v0.w;
      a += (double)v1.x * v1.x + (double)v1.y * v1.y + (double)v1.z * v1.z + (double)v1.w * v1.w;
      a += (double)v2.x * v2.x + (double)v2.y * v2.y + (double)v2.z * v2.z + (double)v2.w * v2.w;
      a += (double)v3.x * v3.x + (double)v3.y * v3.y + (double)v3.z * v3.z + (double)v3.w * v3.w;
    }
    for (; j < n4; j += stride) {
      const float4 v0 = g4[j];
      a += (double)v0.x * v0.x + (double)v0.y * v0.y + (double)v0.z * v0.z + (double)v0.w * v0.w;
    }
    i += n4 * 4;   // the scalar loop: elements [4 n4, n)
  } else if (!rc) {
    for (; i + 3 * stride < n; i += 4 * stride) {   // four independent loads in flight
      const float g0 = g[i], g1 = g[i + stride], g2 = g[i + 2 * stride], g3 = g[i + 3 * stride];
      a += (double)g0 * g0 + (double)g1 * g1 + (double)g2 * g2 + (double)g3 * g3;
    }
  }
  for (; i < n; i += stride) {
    if (rc && rc[i / rl] == 0) continue;
    a += (double)g[i] * g[i];
  }
  part[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if constexpr (DET) {
    if (threadIdx.x == 0) acc[blockIdx.x + (size_t)blockIdx.y * gridDim.x] = part[0];
    return;
  }
  if (threadIdx.x == 0 && part[0] != 0.0) atomicAdd(acc + (blockIdx.x + blockIdx.y * gridDim.x) % TG_SUMSQ_SLOTS, part[0]);
}

// tf.clip_by_global_norm + AMSGrad (amsgrad.py:130-159), all in one pass over the parameters
// gs (coper_train_apply's `scale`): the gradient applied is gs * g, its norm |gs| * |g|; the element factor gs * clip / max(norm, clip)
// is formed once, in double -- gs == 1 (the fused step) multiplies by an exact 1 and leaves the factor's bits what they were
__global__ __launch_bounds__(256) void k_tr_amsgrad(TrainTensors tt, const double* __restrict__ ssq, double* __restrict__ total,
                                                    float clip, float lr_t, float b1, float b2, float eps, double gs) {
  float* p = tt.p[blockIdx.y];
  const float* g = tt.g[blockIdx.y];
  float* m = tt.m[blockIdx.y];
  float* v = tt.v[blockIdx.y];
  float* vh = tt.vh[blockIdx.y];
  const int64_t n = tt.n[blockIdx.y];
  double ss = 0;   // the slots in index order: every thread of every workgroup forms the same sum
  for (int i = 0; i < TG_SUMSQ_SLOTS; ++i) ss += ssq[i];
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *total = ss * gs * gs;   // what coper_train_grad reports
  const double gn = fabs(gs) * sqrt(ss);
  const float scale = (float)(gs * (double)clip / (gn > (double)clip ? gn : (double)clip));
  const int32_t* rc = tt.rowcnt[blockIdx.y];
  const int64_t rl = tt.rowlen[blockIdx.y];
  // dense tensors (every gradient row exists): four elements per thread and step as 16-byte accesses -- nine streams of 4 bytes
  // per element, 1.17 GB per step at the FB15k-237 shapes; element by element (and an int64 division per element for the
  // row-count test that only the looked-up tables need) the pass ran at 5.4 TB/s
  if (!rc && (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)vh) & 15) == 0) {
    const int64_t n4 = n >> 2;
    unsigned pmx = 0u;       // the largest |p_new| this thread wrote (bit pattern): the next step's packs take their power of two from it
    auto upd4 = [&](const float4& g4, float4& m4, float4& v4, float4& h4, float4& p4) {
      float* gm = (float*)&m4; float* gv = (float*)&v4; float* gh = (float*)&h4; float* gp = (float*)&p4; const float* gg = (const float*)&g4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gi = gg[j] * scale;
        const float mi = b1 * gm[j] + (1.f - b1) * gi;
        const float vi = b2 * gv[j] + (1.f - b2) * gi * gi;
        const float vhi = fmaxf(gh[j], vi);
        gm[j] = mi; gv[j] = vi; gh[j] = vhi;
        gp[j] -= lr_t * mi / (sqrtf(vhi) + eps);
        const unsigned pb = __float_as_uint(gp[j]) & 0x7fffffffu;
        pmx = pb > pmx ? pb : pmx;
      }
    };
    const int64_t st = (int64_t)gridDim.x * 256;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    // two elements-of-four per thread and trip: ten 16-byte loads in flight (round 6: five reached 4.9 TB/s on the 1.17 GB of a step)
    // the three slot streams (m, v, v_hat: read once and written once per step, 0.78 GB of the 1.17) with the non-temporal policy:
    // they pass the caches without displacing the gradient the products just wrote and the parameter the packs read next
    // (round 6 A/B, three workloads: - 25 ... - 35 us per step)
#ifndef COPER_DBG_AMSGRAD_NO_NT
    typedef float f4v __attribute__((ext_vector_type(4)));
#define AMS_LD(p_, i_) ([&] { const f4v t = __builtin_nontemporal_load((const f4v*)(p_) + (i_)); return make_float4(t.x, t.y, t.z, t.w); }())
#define AMS_ST(p_, i_, v_) __builtin_nontemporal_store(f4v{(v_).x, (v_).y, (v_).z, (v_).w}, (f4v*)(p_) + (i_))
#else
#define AMS_LD(p_, i_) (((const float4*)(p_))[i_])
#define AMS_ST(p_, i_, v_) (((float4*)(p_))[i_] = (v_))
#endif
    for (; i + st < n4; i += 2 * st) {
      const float4 ga = ((const float4*)g)[i], gb = ((const float4*)g)[i + st];
      float4 ma = AMS_LD(m, i), va = AMS_LD(v, i), ha = AMS_LD(vh, i), pa = ((const float4*)p)[i];
      float4 mb = AMS_LD(m, i + st), vb = AMS_LD(v, i + st), hb = AMS_LD(vh, i + st), pb4 = ((const float4*)p)[i + st];
      upd4(ga, ma, va, ha, pa);
      upd4(gb, mb, vb, hb, pb4);
      AMS_ST(m, i, ma); AMS_ST(v, i, va); AMS_ST(vh, i, ha); ((float4*)p)[i] = pa;
      AMS_ST(m, i + st, mb); AMS_ST(v, i + st, vb); AMS_ST(vh, i + st, hb); ((float4*)p)[i + st] = pb4;
    }
#undef AMS_LD
#undef AMS_ST
    for (; i < n4; i += st) {
      const float4 g4 = ((const float4*)g)[i];
      float4 m4 = ((const float4*)m)[i], v4 = ((const float4*)v)[i], h4 = ((const float4*)vh)[i], p4 = ((const float4*)p)[i];
      upd4(g4, m4, v4, h4, p4);
      ((float4*)m)[i] = m4; ((float4*)v)[i] = v4; ((float4*)vh)[i] = h4; ((float4*)p)[i] = p4;
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
      const float gi = g[i] * scale;
      const float mi = b1 * m[i] + (1.f - b1) * gi;
      const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
      const float vhi = fmaxf(vh[i], vi);
      m[i] = mi; v[i] = vi; vh[i] = vhi;
      const float pn = p[i] - lr_t * mi / (sqrtf(vhi) + eps);
      p[i] = pn;
      const unsigned pb = __float_as_uint(pn) & 0x7fffffffu;
      pmx = pb > pmx ? pb : pmx;
    }
    if (tt.wmax && tt.wmax_of == (int)blockIdx.y) {     // one atomic per wave, spread over the slots (8 per slot at 2,048 workgroups)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { const unsigned u = __shfl_xor(pmx, o, 64); pmx = u > pmx ? u : pmx; }
      if ((threadIdx.x & 63) == 0 && pmx) atomicMax(tt.wmax + ((blockIdx.x * 4 + (threadIdx.x >> 6)) & (TG_MAX_SLOTS - 1)), pmx);
    }
    return;
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float gi = (rc && rc[i / rl] == 0) ? 0.f : g[i] * scale;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    const float vhi = fmaxf(vh[i], vi);
    m[i] = mi; v[i] = vi; vh[i] = vhi;
    p[i] -= lr_t * mi / (sqrtf(vhi) + eps);
  }
}

__global__ void k_tr_store_loss(const double* __restrict__ acc, double inv_BL, float* __restrict__ out) { out[0] = (float)(acc[0] * inv_BL); }

// logits of the train-mode forward for coper_train_forward: the fma chain of k_tr_score_loss (sampled) / S + bias (1-vs-all)
__global__ __launch_bounds__(256) void k_tr_scores_out(const float* __restrict__ hv, const float* __restrict__ ent,
                                                       const float* __restrict__ pred_bias, const int32_t* __restrict__ lookup,
                                                       int64_t E, int d, int64_t L, float* __restrict__ out) {
  const int64_t b = blockIdx.x;
  for (int64_t l = threadIdx.x; l < L; l += 256) {
    int64_t row = lookup[b * L + l];
    if (row < 0 || row >= E) row = 0;
    const float* er = ent + row * d;
    float s = 0.f;
    for (int k = 0; k < d; ++k) s = fmaf(hv[b * d + k], er[k], s);
    out[b * L + l] = s + pred_bias[row];
  }
}
// The SHARD form for the forward-only sharded call: the same chain for the entries (b, l) whose clamped id lies in
// [sh_lo, sh_lo + sh_n), from the handle's own rows; an exact +0.f at every other entry -- so every element of [B, L] has one non-zero
// addend over the ranks and their sum is exact.  CURRENT: k_tr_score_loss's comment.
template <bool CURRENT>
__global__ __launch_bounds__(256) void k_tr_scores_out_shard(const float* __restrict__ hv, const float* __restrict__ ent,
                                                             const float* __restrict__ pred_bias, const int32_t* __restrict__ lookup,
                                                             int64_t E, int d, int64_t L, float* __restrict__ out, int64_t sh_lo, int64_t sh_n,
                                                             RowTables rt, RowCatchUp cu) {
  const int64_t b = blockIdx.x;
  const int64_t Lw = (L + 255) / 256 * 256;      // (CURRENT: the waves make every trip whole)
  for (int64_t l = threadIdx.x; l < Lw; l += 256) {
    bool own = l < L;
    int64_t row = 0;
    if (own) {
      row = lookup[b * L + l];
      row = ((row < 0 || row >= E) ? 0 : row) - sh_lo;
      own = row >= 0 && row < sh_n;
    }
    [[maybe_unused]] double Cs = 0.0;
    [[maybe_unused]] bool behind = false;
    if constexpr (CURRENT) {
      const int gap = own ? cu.now - rt.word[row] : 0;
      behind = gap > 0;
      Cs = rows_wave_C(cu, gap, (int)(threadIdx.x & 63));
    }
    if (l >= L) continue;
    float s = 0.f;
    if (own) {
      const float* er = ent + row * d;
      const float* hb = hv + b * d;
      if ((d & 3) == 0) {   // 16-byte loads of the row (and of its slots); the fma chain keeps its order
        for (int k4 = 0; k4 < d / 4; ++k4) {
          float4 e = ((const float4*)er)[k4];
          if constexpr (CURRENT) { if (behind) e = rows_current4(rt, cu, row * d + 4 * k4, e, Cs); }
          const float4 h4 = ((const float4*)hb)[k4];
          s = fmaf(h4.x, e.x, s); s = fmaf(h4.y, e.y, s); s = fmaf(h4.z, e.z, s); s = fmaf(h4.w, e.w, s);
        }
      } else
      for (int k = 0; k < d; ++k) {
        float e = er[k];
        if constexpr (CURRENT) { if (behind) e = rows_current1(rt, cu, row * d + k, e, Cs); }
        s = fmaf(hb[k], e, s);
      }
      float pb = pred_bias[row];
      if constexpr (CURRENT) { if (behind) pb = rows_current_bias(rt, cu, row, pb, Cs); }
      s += pb;
    }
    out[b * L + l] = s;
  }
}
__global__ __launch_bounds__(256) void k_tr_add_bias_out(const float* __restrict__ S, const float* __restrict__ pred_bias, int64_t E,
                                                         int64_t total, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total) out[i] = S[i] + pred_bias[i % E];
}
// coper_train_grad on a looked-up table: rows of relations the last batch did not hold are never written by the step (the optimizer and
// the global norm skip them by their count) -- the copy handed out shows them as the zeros they are
__global__ __launch_bounds__(256) void k_tr_zero_absent_rows(float* __restrict__ out, const int32_t* __restrict__ rowcnt, int64_t rowlen, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    if (rowcnt[i / rowlen] == 0) out[i] = 0.f;
}

// coper_train_grads_export: every trainable leaf's gradient into its slice of the flat gradient vector, one launch (blockIdx.y = leaf).
// flat[off + i] = g[i], or += g[i] (ACC); the pad behind a leaf (up to the next multiple of 64 floats) is written as 0.  One thread
// owns an element: no atomics, one defined order in either form.  The looked-up dense table (leaf `table`) hands out the rows of
// relations absent from the batch as zeros by the step's relation counts (ACC: they add nothing) -- the only leaf that pays the
// row test.  16-byte accesses, four of them in flight per thread; the scalar loop takes a leaf's last n % 4 elements and the pad.
struct ExportList {
  const float* g[TR_MAX_PARAMS];
  int64_t off[TR_MAX_PARAMS];    // multiples of 64 floats: a 16-byte aligned `flat` keeps every slice 16-byte aligned
  int64_t n[TR_MAX_PARAMS];
  int64_t span[TR_MAX_PARAMS];   // n rounded up to a multiple of 64: the slice with its pad
  int table;                     // -1: none
  int64_t rowlen;
  const int32_t* rowcnt;
};
template <bool ACC>
__global__ __launch_bounds__(256) void k_tr_grads_export(ExportList el, float* __restrict__ flat) {
  const int y = blockIdx.y;
  const float* __restrict__ g = el.g[y];
  float* __restrict__ out = flat + el.off[y];
  const int64_t n = el.n[y], span = el.span[y];
  const int64_t st = (int64_t)gridDim.x * 256, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n4 = ((uintptr_t)g & 15) == 0 ? n >> 2 : 0;
  const float4* g4 = (const float4*)g;
  float4* o4 = (float4*)out;
  auto put = [&](int64_t j, const float4& v) {
    if constexpr (ACC) { const float4 o = o4[j]; o4[j] = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w); }
    else o4[j] = v;
  };
  if (y == el.table) {
    const int64_t rl = el.rowlen;
    const int32_t* __restrict__ rc = el.rowcnt;
    for (int64_t j = i; j < n4; j += st) {
      const int64_t e = j * 4, row = e / rl, rem = e - row * rl;
      if (rem + 3 < rl) {      // the four elements lie in one row
        if (rc[row] != 0) put(j, g4[j]);
        else if (!ACC) o4[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {                 // a row boundary inside: element by element
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const bool present = rc[(e + u) / rl] != 0;
          if constexpr (ACC) { if (present) out[e + u] += g[e + u]; }
          else out[e + u] = present ? g[e + u] : 0.f;
        }
      }
    }
  } else {
    int64_t j = i;
    for (; j + 3 * st < n4; j += 4 * st) {
      const float4 v0 = g4[j], v1 = g4[j + st], v2 = g4[j + 2 * st], v3 = g4[j + 3 * st];
      if constexpr (ACC) {
        const float4 a0 = o4[j], a1 = o4[j + st], a2 = o4[j + 2 * st], a3 = o4[j + 3 * st];
        o4[j] = make_float4(a0.x + v0.x, a0.y + v0.y, a0.z + v0.z, a0.w + v0.w);
        o4[j + st] = make_float4(a1.x + v1.x, a1.y + v1.y, a1.z + v1.z, a1.w + v1.w);
        o4[j + 2 * st] = make_float4(a2.x + v2.x, a2.y + v2.y, a2.z + v2.z, a2.w + v2.w);
        o4[j + 3 * st] = make_float4(a3.x + v3.x, a3.y + v3.y, a3.z + v3.z, a3.w + v3.w);
      } else {
        o4[j] = v0; o4[j + st] = v1; o4[j + 2 * st] = v2; o4[j + 3 * st] = v3;
      }
    }
    for (; j < n4; j += st) put(j, g4[j]);
  }
  for (int64_t e = 4 * n4 + i; e < span; e += st) {
    if (e >= n) { out[e] = 0.f; continue; }      // the pad
    const bool present = y != el.table || el.rowcnt[e / el.rowlen] != 0;
    if constexpr (ACC) { if (present) out[e] += g[e]; }
    else out[e] = present ? g[e] : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------
// deterministic mode (coper_train_config.deterministic): the kernels that only this mode launches
// ------------------------------------------------------------------------------------------------
// The fold of a slab [nslots][n] that the workgroups of a reducing launch stored (workgroup w: slot w): a workgroup per column j,
// thread t adds slots t, t + 256, ... in ascending order, the 256 thread sums meet in a fixed LDS tree.  The order depends on
// (n, nslots) alone -- the reducing launch's grid, which this mode sizes by the problem shape.  accumulate: onto what out[j] holds.
__global__ __launch_bounds__(256) void k_tr_fold_det(const double* __restrict__ slab, int n, int64_t nslots, double* __restrict__ out,
                                                     int accumulate) {
  __shared__ double sh[256];
  const int j = blockIdx.x;
  double a = 0;
  for (int64_t z = threadIdx.x; z < nslots; z += 256) a += slab[z * n + j];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[j] = accumulate ? out[j] + sh[0] : sh[0];
}

// out[e] = slab[0][e] + slab[1][e] + ... in ascending z: the row stretches of k_tr_col_sums_add<true> / k_tr_wsum_rows_add<true>
__global__ __launch_bounds__(256) void k_tr_fold_f32_det(const float* __restrict__ slab, int64_t n, int nz, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  float a = 0.f;
  for (int z = 0; z < nz; ++z) a += slab[(size_t)z * n + e];
  out[e] = a;
}

// k_tr_bn1_bwd_sums for any C <= 256 without an LDS atomic: k_tr_col_sums' layout -- thread (row lane, channel), a workgroup's row
// lanes added in lane order -- over the [B P, C] gradient; workgroup w stores its 2 C sums at slab[w]
__global__ __launch_bounds__(256) void k_tr_bn1_bwd_sums_det(float* __restrict__ dx, const float* __restrict__ y, const float* __restrict__ mean,
                                                             const float* __restrict__ inv, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, int C, int64_t rows, uint32_t seed, uint32_t step, uint32_t ioff,
                                                             uint32_t thr, float keep_scale, double* __restrict__ slab) {
  __shared__ double s1[256], s2[256];
  double* const out = slab + (size_t)blockIdx.x * 2 * C;
  const int cpt = 256 / C, c = threadIdx.x % C, rl = threadIdx.x / C;
  double a1 = 0, a2 = 0;
  if (rl < cpt) {
    const float mc = mean[c], ic = inv[c], gc = gamma[c], bc = beta[c];
    for (int64_t rr = (int64_t)blockIdx.x * cpt + rl; rr < rows; rr += (int64_t)gridDim.x * cpt) {
      const int64_t i = rr * C + c;
      const float yh = (y[i] - mc) * ic;
      const float act = yh * gc + bc;
      float g = dropout_keep_u32(seed, step, 1u, (uint32_t)i + ioff, thr) ? dx[i] * keep_scale : 0.f;
      if (!(act > 0.f)) g = 0.f;
      dx[i] = g;
      a1 += g;
      a2 += (double)g * yh;
    }
  }
  s1[threadIdx.x] = a1; s2[threadIdx.x] = a2;
  __syncthreads();
  if ((int)threadIdx.x < C) {
    for (int l = 1; l < cpt; ++l) { a1 += s1[threadIdx.x + l * C]; a2 += s2[threadIdx.x + l * C]; }
    out[c] = a1;
    out[C + c] = a2;
  }
}

// Row scatter with ONE WRITER PER DESTINATION ROW: dst[key[b], 0 .. n) += src[b, col0 .. col0 + n) over the samples b of a key in
// ASCENDING b, onto what dst holds.  A workgroup per sample: the one of a key's FIRST sample (a leader scan over the ids in front of
// it) is the key's writer and walks the rest of the batch, 256 ids at a time through LDS; the others leave.  B^2 / 2 id compares per
// launch, no sort, no workspace, any B.  Keys outside [0, K) count as 0, as everywhere in the step.
__global__ __launch_bounds__(256) void k_tr_rows_by_key_det(const float* __restrict__ src, int64_t stride, int64_t col0, int n,
                                                            const int64_t* __restrict__ keys, int64_t K, int64_t B, float* __restrict__ dst) {
  __shared__ int64_t kc[256];
  const int64_t b = blockIdx.x;
  auto key = [&](int64_t i) { const int64_t k = keys[i]; return (k < 0 || k >= K) ? (int64_t)0 : k; };
  const int64_t k = key(b);
  int earlier = 0;
  for (int64_t i = threadIdx.x; i < b; i += 256) earlier |= key(i) == k ? 1 : 0;
  if (__syncthreads_or(earlier)) return;      // (uniform)
  for (int t0 = 0; t0 < n; t0 += 256) {
    const int t = t0 + threadIdx.x;
    float a = t < n ? dst[k * n + t] : 0.f;
    for (int64_t i0 = b; i0 < B; i0 += 256) {
      __syncthreads();
      kc[threadIdx.x] = i0 + threadIdx.x < B ? key(i0 + threadIdx.x) : (int64_t)-1;
      __syncthreads();
      const int m = (int)(B - i0 < 256 ? B - i0 : 256);
      if (t < n)
        for (int u = 0; u < m; ++u)
          if (kc[u] == k) a += src[(i0 + u) * stride + col0 + t];
    }
    if (t < n) dst[k * n + t] = a;
  }
}

// k_tr_build_S with the duplicate ids of a row added in ASCENDING l: rounds over a stretch of TR_SDET_CHUNK columns in LDS -- in
// every round the lowest not yet placed l of a column wins an integer atomicMin (order-free) and is that column's only adder; the
// rounds end when nothing is left: 1 + the largest multiplicity of an id in the row.
constexpr int TR_SDET_CHUNK = 4096;
__global__ __launch_bounds__(256) void k_tr_build_S_det(const int32_t* __restrict__ lookup, const float* __restrict__ ds, int64_t E, int64_t L,
                                                        float* __restrict__ S, unsigned* __restrict__ max_slots) {
  __shared__ float s_row[TR_SDET_CHUNK];
  __shared__ int placed[TR_SDET_CHUNK], nxt[TR_SDET_CHUNK];
  const int64_t b = blockIdx.x;
  const int32_t* lk = lookup + b * L;
  const float* g = ds + b * L;
  float mx = 0.f;
  for (int64_t c0 = 0; c0 < E; c0 += TR_SDET_CHUNK) {
    const int n = (int)(E - c0 < TR_SDET_CHUNK ? E - c0 : TR_SDET_CHUNK);
    for (int i = threadIdx.x; i < n; i += 256) { s_row[i] = 0.f; placed[i] = -1; }
    for (;;) {
      for (int i = threadIdx.x; i < n; i += 256) nxt[i] = 0x7fffffff;
      __syncthreads();
      int any = 0;
      for (int64_t l = threadIdx.x; l < L; l += 256) {
        int64_t row = lk[l];
        if (row < 0 || row >= E) row = 0;
        if (row >= c0 && row < c0 + n && (int)l > placed[row - c0]) { atomicMin(&nxt[row - c0], (int)l); any = 1; }
      }
      if (!__syncthreads_or(any)) break;      // (uniform)
      for (int64_t l = threadIdx.x; l < L; l += 256) {
        int64_t row = lk[l];
        if (row < 0 || row >= E) row = 0;
        if (row >= c0 && row < c0 + n && nxt[row - c0] == (int)l) { s_row[row - c0] += g[l]; placed[row - c0] = (int)l; }
      }
      __syncthreads();
    }
    float* out = S + b * E + c0;
    for (int i = threadIdx.x; i < n; i += 256) {
      const float v = s_row[i];
      out[i] = v;
      mx = fmaxf(mx, fabsf(v));
    }
    __syncthreads();
  }
  tr_block_max_to_slot(mx, max_slots);
}

// the samples of every relation group (perm / offset / count of the handle's grouping, whose order inside a group is arrival order) in
// ASCENDING sample index -> out, by rank: a workgroup per relation, count^2 / 256 compares per thread.  The grouping itself is not touched.
__global__ __launch_bounds__(256) void k_tr_sort_groups_det(const int32_t* __restrict__ perm, const int32_t* __restrict__ offset,
                                                            const int32_t* __restrict__ count, int32_t* __restrict__ out) {
  const int n = count[blockIdx.x], off = offset[blockIdx.x];
  for (int i = threadIdx.x; i < n; i += 256) {
    const int32_t p = perm[off + i];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += perm[off + j] < p ? 1 : 0;
    out[off + rank] = p;
  }
}

}  // namespace
}  // namespace coper
