// COPER_DENSE_FACTORED (coper_config.dense_mode): the generated dense layer at inference WITHOUT the per-relation weight cache.
//
//   h_pre[b, k] = sum_rho ctx[rel_b, rho] * ( sum_f x[b, f] * P[rho, f d + k] )  +  fc_b_rel[rel_b, k]
//   h[b, k]     = relu( fc_scale[k] h_pre[b, k] + fc_shift[k] )
//
// ctx [R, K] is the context of the fc_weights generator (rel_emb for g_linear, the last hidden activation for g_MLP: kept by
// coper_prepare), P [K, F d] its last projection, packed ONCE at prepare into the split-fp16 operand planes of train_gemm.h (rows
// (rho, k), contraction index f).  A chunk of queries takes three launches:
//   1. k_fac_x       conv + folded-in Conv1BN + ReLU (+ the concat_rel tail) of 32 queries per workgroup, written straight into the
//                    x operand planes (TgPlanes fragment order, rows = queries of the chunk) as x 2^e_x hi + lo -- e_x is the
//                    HANDLE's power of two (compute_x_exp: from a bound on x), never the batch's maximum; x never exists in fp32
//   2. tg_gemm_nt    T[b, (rho, k)] = sum_f x P on the 16-bit matrix cores (3 MFMAs per product), K slices and kernel variant
//                    pinned at prepare; the slices stay in the partial-sum buffer
//   3. k_fac_finish  the slices added in slice order, the contraction over rho (ascending, one fp32 fma chain), bias, folded FCBN,
//                    ReLU -> h rows
// Every element of h[b] is summed in an order that depends on the configuration only: h[b] is the same bits whatever batch, chunk or
// position computes it.  Nothing is grouped by relation (a query's relation enters as K scalars in step 3), so the grouping launches
// of the cached path do not run; ids out of range are clamped and counted by step 1 into the counter coper_check_ids reads.
#include "coper_internal.h"
#include "split16.h"
#include "train_gemm.h"

namespace coper {

struct FacXArgs {
  const int64_t* e1; const int64_t* rel; const float* e1_rows;     // the chunk's first query
  const float* ent; int64_t shard_lo, n_local, E, R;
  const float* rel_emb; const float* conv_w; const float* conv_b; int per_rel_conv;
  const float* scale; const float* shift;
  int d, r, in_w, fh, fw, C, Wo, img_stride, x_exp, KS16, KST;
  int64_t F_conv, F, M;                                             // M: queries of the chunk
  uint4* hi; uint4* lo; int32_t* bad;
};

constexpr int FAC_X_KSB = 32;     // k-steps (of 16 values of f) per workgroup: 8 per wave

// Workgroup (k-step range, 32-query row block): the 32 images in LDS (row stride odd: the 32 rows of a wave read 32 banks), then every
// wave takes whole (row block, k-step) fragment blocks -- lane l holds row l & 31, values f = 16 ks + 8 (l >> 5) + j -- and stores
// 1 KiB per plane per block, contiguous.  C8: C is a multiple of 8, so the 8 values of a lane are 8 channels of ONE pixel (the window
// is read once, the taps as 16-byte loads); otherwise every value decodes its own (pixel, channel).
template <bool C8>
__global__ __launch_bounds__(256) void k_fac_x(FacXArgs A) {
  extern __shared__ float lds[];     // img[32][img_stride]
  __shared__ int s_rid[32];
  const int t = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.y * 32;
  if (t < 32) {
    const int64_t q = q0 + t;
    int rid = 0;
    if (q < A.M) {
      const int64_t v = A.rel[q];
      const bool ok = v >= 0 && v < A.R;
      rid = ok ? (int)v : 0;
      int nbad = ok ? 0 : 1;
      if (!A.e1_rows) { const int64_t e = A.e1[q]; nbad += (e < 0 || e >= A.E) ? 1 : 0; }
      if (nbad && blockIdx.x == 0) atomicAdd(A.bad, nbad);        // clamped, and reported by coper_check_ids
    }
    s_rid[t] = rid;
  }
  for (int i = t; i < 32 * A.d; i += 256) {
    const int row = i / A.d, k = i - row * A.d;
    const int64_t q = q0 + row;
    float v = 0.f;
    if (q < A.M) {
      if (A.e1_rows) {
        v = A.e1_rows[q * A.d + k];
      } else {
        const int64_t er = A.e1[q] - A.shard_lo;
        if (er >= 0 && er < A.n_local) v = A.ent[er * A.d + k];
      }
    }
    lds[row * A.img_stride + k] = v;
  }
  __syncthreads();
  const int wave = t >> 6, lane = t & 63, row = lane & 31, half = lane >> 5;
  const bool live = q0 + row < A.M;
  const int rid = s_rid[row];
  const float* img = lds + row * A.img_stride;
  const float* wsrc = A.per_rel_conv ? A.conv_w + (int64_t)rid * (A.fh * A.fw * A.C) : A.conv_w;
  const float* bsrc = A.per_rel_conv ? A.conv_b + (int64_t)rid * A.C : A.conv_b;
  const int ks_end = min((int)(blockIdx.x + 1) * FAC_X_KSB, A.KS16);
  for (int ks = blockIdx.x * FAC_X_KSB + wave; ks < ks_end; ks += 4) {
    const int64_t f0 = (int64_t)ks * 16 + 8 * half;
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = 0.f;
    if (live) {
      if (C8 && f0 < A.F_conv) {
        const int pix = (int)(f0 / A.C), c0 = (int)(f0 - (int64_t)pix * A.C);
        const int oh = pix / A.Wo, ow = pix - oh * A.Wo;
        for (int u = 0; u < A.fh; ++u)
          for (int v = 0; v < A.fw; ++v) {
            const float w = img[(oh + u) * A.in_w + ow + v];
            const float4 ta = *(const float4*)(wsrc + (u * A.fw + v) * A.C + c0), tb = *(const float4*)(wsrc + (u * A.fw + v) * A.C + c0 + 4);
            y[0] = fmaf(w, ta.x, y[0]); y[1] = fmaf(w, ta.y, y[1]); y[2] = fmaf(w, ta.z, y[2]); y[3] = fmaf(w, ta.w, y[3]);
            y[4] = fmaf(w, tb.x, y[4]); y[5] = fmaf(w, tb.y, y[5]); y[6] = fmaf(w, tb.z, y[6]); y[7] = fmaf(w, tb.w, y[7]);
          }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float a = fmaf(y[j] + bsrc[c0 + j], A.scale[c0 + j], A.shift[c0 + j]);
          y[j] = x3_scale(fmaxf(a, 0.f), A.x_exp);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int64_t f = f0 + j;
          if (f < A.F_conv) {
            const int pix = (int)(f / A.C), c = (int)(f - (int64_t)pix * A.C);
            const int oh = pix / A.Wo, ow = pix - oh * A.Wo;
            float a = 0.f;
            for (int u = 0; u < A.fh; ++u)
              for (int v = 0; v < A.fw; ++v) a = fmaf(img[(oh + u) * A.in_w + ow + v], wsrc[(u * A.fw + v) * A.C + c], a);
            a = fmaf(a + bsrc[c], A.scale[c], A.shift[c]);
            y[j] = x3_scale(fmaxf(a, 0.f), A.x_exp);
          } else if (f < A.F) {       // concat_rel: the relation embedding behind the conv features (models.py:406)
            y[j] = x3_scale(A.rel_emb[(int64_t)rid * A.r + (f - A.F_conv)], A.x_exp);
          }
        }
      }
    }
    uint4 h4, l4;
    split8_s16(y, h4, l4);
    const int64_t o = ((int64_t)blockIdx.y * A.KST + ks) * 64 + lane;
    A.hi[o] = h4;
    A.lo[o] = l4;
  }
}

// h rows from the K slices of T: one thread per (query, feature k).  part: [NS][M][N] with N = K_ctx * d, column rho d + k.
__global__ __launch_bounds__(256) void k_fac_finish(const float* __restrict__ part, int ns, int64_t M, int Kc, int d,
                                                    const int64_t* __restrict__ rel, int64_t R, const float* __restrict__ ctx,
                                                    const float* __restrict__ fc_b, const float* __restrict__ scale,
                                                    const float* __restrict__ shift, float* __restrict__ h_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * d) return;
  const int64_t b = i / d;
  const int k = (int)(i - b * d);
  int64_t rid = rel[b];
  if (rid < 0 || rid >= R) rid = 0;
  const int64_t N = (int64_t)Kc * d, MN = M * N;
  const float* p = part + b * N + k;
  const float* cw = ctx + rid * Kc;
  float v = 0.f;
#pragma unroll 4
  for (int rho = 0; rho < Kc; ++rho) {
    float a = p[(int64_t)rho * d];
    for (int z = 1; z < ns; ++z) a += p[(int64_t)z * MN + (int64_t)rho * d];     // slice order
    v = fmaf(cw[rho], a, v);
  }
  v += fc_b[rid * d + k];
  v = fmaf(v, scale[k], shift[k]);
  h_out[i] = fmaxf(v, 0.f);
}

__global__ void k_fac_set_exp(int32_t* dst, int e) { *dst = e; }

// what coper_prepare builds for a factored handle: the context of the fc_weights generator (copied out of the generator scratch), the
// planes of its last projection, the device word of e_x, and the plan (chunk, K slices, GEMM variant) -- all from the configuration
int factored_prepare(coper_handle* h, const float* ctx, int Kc, const float* P_last, hipStream_t s) {
  const Dims& dm = h->dm;
  int rc;
  const int64_t N = (int64_t)Kc * dm.d, F = dm.F;
  h->fac_K = Kc;
  if ((rc = h->fac_ctx.alloc(h, (size_t)dm.R * Kc, "factored context")) || (rc = h->fac_exp.alloc(h, 4, "factored exponents")) ||
      (rc = h->fac_P_hi.alloc(h, tg_plane_elems(N, F), "factored projection planes")) ||
      (rc = h->fac_P_lo.alloc(h, tg_plane_elems(N, F), "factored projection planes")))
    return rc;
  COPER_HIP_TRY(h, hipMemcpyAsync(h->fac_ctx, ctx, sizeof(float) * (size_t)dm.R * Kc, hipMemcpyDeviceToDevice, s));
  COPER_HIP_TRY(h, hipMemsetAsync(h->fac_exp, 0, 4 * sizeof(int32_t), s));     // [0] e_P, [1] e_x, [2..3] tg_pack's scratch (zero between packs)
  TgPlanes pl;
  pl.hi = h->fac_P_hi; pl.lo = h->fac_P_lo; pl.exp = h->fac_exp;
  // rows (rho, k) of P [K][F][d], contracted over f (the view the training forward packs)
  if ((rc = tg_pack(h, P_last, tg_idx2(dm.d, F * (int64_t)dm.d, 1), tg_idx(dm.d), N, F, tg_rows_pad(N), true, pl, s,
                    (unsigned*)(h->fac_exp.get() + 2))))
    return rc;
  hipLaunchKernelGGL(k_fac_set_exp, dim3(1), dim3(1), 0, s, h->fac_exp.get() + 1, h->x_exp);
  COPER_HIP_TRY(h, hipGetLastError());
  // The plan.  K slices: two when the contraction is long (half the time of a batch that fills a fraction of the chip, twice the
  // partial sums), one otherwise; the chunk: as many queries (a multiple of 128, at most 4,096) as keep the slices of T within 256 MB;
  // the variant: what the GEMM would choose for a full chunk.
  const int ks16 = (int)((F + 15) / 16);
  int ns = ks16 >= 64 ? 2 : 1;
  if (const char* e = getenv("COPER_FACTORED_NSPLIT")) { const int v = atoi(e); if (v >= 1 && v <= 8 && v <= ks16) ns = v; }   // A/B switch
  int64_t chunk = ((int64_t)256 << 20) / ((int64_t)ns * N * 4) / 128 * 128;
  if (chunk > 4096) chunk = 4096;
  if (const char* e = getenv("COPER_FACTORED_CHUNK")) { const int64_t v = atoll(e) / 128 * 128; if (v >= 128 && v < chunk) chunk = v; }   // tests: several chunks
  if (chunk < 128) chunk = 128;
  h->fac_nsplit = ns;
  h->fac_chunk = chunk;
  h->fac_variant = (int)tg_variant_for(chunk, N, F);
  return COPER_OK;
}

// the chunk workspaces for batches of up to `cap` queries
bool factored_workspace_short(const coper_handle* h, int64_t cap) {
  const Dims& dm = h->dm;
  const int64_t rows = cap < h->fac_chunk ? cap : h->fac_chunk, N = (int64_t)h->fac_K * dm.d;
  return h->fac_x_hi.size() < tg_plane_elems(rows, dm.F) || h->fac_x_lo.size() < tg_plane_elems(rows, dm.F) ||
         h->fac_T.size() < (size_t)h->fac_nsplit * rows * N;
}
int factored_workspace(coper_handle* h, int64_t cap) {
  const Dims& dm = h->dm;
  const int64_t rows = cap < h->fac_chunk ? cap : h->fac_chunk, N = (int64_t)h->fac_K * dm.d;
  int rc;
  if ((rc = h->fac_x_hi.ensure(h, tg_plane_elems(rows, dm.F), "factored x planes")) ||
      (rc = h->fac_x_lo.ensure(h, tg_plane_elems(rows, dm.F), "factored x planes")) ||
      (rc = h->fac_T.ensure(h, (size_t)h->fac_nsplit * rows * N, "factored product")))
    return rc;
  return COPER_OK;
}

int launch_dense_factored(coper_handle* h, const int64_t* e1, const int64_t* rel, const float* e1_rows, int64_t B, float* h_out, hipStream_t s) {
  const Dims& dm = h->dm;
  const int Kc = h->fac_K;
  const int64_t N = (int64_t)Kc * dm.d;
  int32_t* bad = h->gset[0].rel_count + dm.R + 1;
  COPER_HIP_TRY(h, hipMemsetAsync(bad, 0, sizeof(int32_t), s));
  FacXArgs A;
  A.ent = h->lv.ent_emb->ptr; A.shard_lo = h->cfg.shard_lo; A.n_local = dm.n_local; A.E = dm.E; A.R = dm.R;
  A.rel_emb = h->lv.rel_emb->ptr;
  A.conv_w = conv_w(h);
  A.conv_b = conv_b(h);
  A.per_rel_conv = dm.gen_conv ? 1 : 0;
  A.scale = h->conv_scale; A.shift = h->conv_shift;
  A.d = dm.d; A.r = dm.r; A.in_w = dm.in_w; A.fh = dm.fh; A.fw = dm.fw; A.C = dm.C; A.Wo = dm.Wo;
  A.img_stride = dm.d | 1; A.x_exp = h->x_exp;
  A.KS16 = (int)((dm.F + 15) / 16); A.KST = (int)tg_ks_stride(dm.F);
  A.F_conv = dm.F_conv; A.F = dm.F;
  A.hi = h->fac_x_hi; A.lo = h->fac_x_lo; A.bad = bad;
  const bool c8 = dm.C % 8 == 0 && (((uintptr_t)A.conv_w) & 15) == 0;
  const size_t lds = sizeof(float) * 32 * (size_t)A.img_stride;
  TgPlanes X, Y;
  X.hi = h->fac_x_hi; X.lo = h->fac_x_lo; X.exp = h->fac_exp.get() + 1;
  Y.hi = h->fac_P_hi; Y.lo = h->fac_P_lo; Y.exp = h->fac_exp.get();
  const float* fcb = h->fc_b_rel;
  for (int64_t q0 = 0; q0 < B; q0 += h->fac_chunk) {
    const int64_t M = B - q0 < h->fac_chunk ? B - q0 : h->fac_chunk;
    A.e1 = e1 ? e1 + q0 : nullptr; A.rel = rel + q0; A.e1_rows = e1_rows ? e1_rows + q0 * dm.d : nullptr; A.M = M;
    // every row block of the 128-row tiles the GEMM reads is written (rows beyond M as zeros)
    const dim3 grid((unsigned)((A.KS16 + FAC_X_KSB - 1) / FAC_X_KSB), (unsigned)(tg_rows_pad(M) / 32));
    {
      ScopedKernelTimer t(h, "conv", s);
      if (c8) hipLaunchKernelGGL(k_fac_x<true>, grid, dim3(256), lds, s, A);
      else hipLaunchKernelGGL(k_fac_x<false>, grid, dim3(256), lds, s, A);
      COPER_HIP_TRY(h, hipGetLastError());
    }
    COPER_DBG_SYNC(h, s, "factored x");
    ScopedKernelTimer t(h, "dense", s);
    int rc;
    if ((rc = tg_gemm_nt(h, X, M, Y, N, dm.F, h->fac_T, tg_idx(N), tg_idx(1), s, h->fac_nsplit, h->fac_T, nullptr, true,
                         (TgVariant)h->fac_variant)))
      return rc;
    COPER_DBG_SYNC(h, s, "factored gemm");
    hipLaunchKernelGGL(k_fac_finish, dim3((unsigned)((M * dm.d + 255) / 256)), dim3(256), 0, s, h->fac_T.get(), h->fac_nsplit, M, Kc, dm.d,
                       rel + q0, dm.R, h->fac_ctx.get(), fcb, h->fc_scale.get(), h->fc_shift.get(), h_out + q0 * dm.d);
    COPER_HIP_TRY(h, hipGetLastError());
    COPER_DBG_SYNC(h, s, "factored finish");
  }
  return COPER_OK;
}

}  // namespace coper
