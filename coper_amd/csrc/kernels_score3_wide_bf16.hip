// k_score_count3_wide_bf16x3 -- the count kernel of the bf16x3 mode for ent_emb_size beyond 320 (KS16 = 21 .. 40).
//
// k_score_count3_bf16x3 (kernels_score3_bf16.hip) keeps the f3 fragments of its 128-query tile in LDS for the whole launch:
// 16 KiB per step (a pair of k-steps), the CU's 160 KiB at KS16 = 20.  This kernel keeps the SAME tile -- 128 queries, the
// same f3 images on both sides, the same band mask / summary / block-maxima layouts, so that everything around the count
// launch (k_rows_to_frag_bf16, k_band_setup, k_band_exact, the top-k threshold and re-scoring) serves a wide handle unchanged
// and there is one tile width in the library -- and holds it in LDS in TWO HALVES OF K: a workgroup's row (4 waves x 2 blocks
// of 64 entities against the tile) runs steps [0, SCH) of both blocks of every wave from the first half, the workgroup
// swaps the second half in, and the 256 accumulators of a lane are carried across.  A half is re-read from L2 once per row
// per workgroup.  Measured (profiles/wide_d.json): 209 - 229 TFLOP/s algorithmic at d = 400 .. 640 against 512 for
// the pipelined kernel at d = 320 and 101 - 105 for the f32 wide kernel -- the compiler's schedule and the per-row fixed costs, not yet
// taken apart.
//
// Arithmetic: bf16x3_chain.h.  Per accumulator the instructions are those of sc3_mfmas in the same order -- step s:
// (e.reg0, q.reg1), (e.reg1, q.reg0), (e.reg1, q.reg1); the tail step of an odd KS16: the first two -- starting from
// pred_bias 2^(e_E + e_h): the one order of the mode (by construction; the kernel exports no logit a test could compare).  The step count is a run-time
// argument (one instantiation per block-maxima form, not one per KS16), the schedule is the compiler's: entity fragments are
// requested one step ahead, the epilogue of a row follows its last instruction.  The register-level pipeline of the narrow
// kernel is instantiated per KS16 and tuned at d = 200 / 256; it is not touched.
#include "bf16x3_chain.h"
#include "coper_internal.h"

namespace coper {

#if defined(COPER_SC3_MB) && COPER_SC3_MB != 4
#error "the wide count kernel is written for 64-entity blocks (COPER_SC3_MB = 4)"
#endif

namespace {
constexpr int W3_MB = 4;              // 16-row blocks per entity block of a wave (SC3_MB)
constexpr int W3_NB = X3_TILE_Q / 16; // 16-query column blocks of the tile
static_assert(W3_NB == 8, "a mask word holds 32 values = two column blocks of 4 MB");

struct W3Frag { uint4 a0[W3_MB], a1[W3_MB]; };

// block `blk` (64 entities), step s: registers ((m2 NS + s) 2 + w) 64 + lane of the block's W3_MB NS 2 registers
__device__ __forceinline__ void w3_load(W3Frag& f, const uint4* __restrict__ Ef3, const int64_t blk, const int NS, const int s, const int lane) {
  const uint4* p = Ef3 + blk * ((int64_t)W3_MB * NS * 2 * 64) + lane;
#pragma unroll
  for (int m2 = 0; m2 < W3_MB; ++m2) {
    f.a0[m2] = p[((m2 * NS + s) * 2 + 0) * 64];
    f.a1[m2] = p[((m2 * NS + s) * 2 + 1) * 64];
  }
}
}  // namespace

// Ef3 / Hf3 / tband / mask / summ / gmax: as k_score_count3_bf16x3.  NS steps, the first NP of them pairs; SCH: steps per half.
template <int GM>
__global__ __launch_bounds__(256, 1) void k_score_count3_wide_bf16x3(const uint4* __restrict__ Ef3, const float* __restrict__ bias_pad,
                                                                      const uint4* __restrict__ Hf3, const float2* __restrict__ tband,
                                                                      int64_t B, int NS, int NP, int SCH, int64_t rows_per_tile,
                                                                      int64_t total_rows, int32_t* __restrict__ ng, uint4* __restrict__ mask,
                                                                      unsigned long long* __restrict__ summ, float* __restrict__ gmax,
                                                                      int64_t gm_stride, const int32_t* __restrict__ x3s) {
  constexpr int MB = W3_MB, NB = W3_NB;
  extern __shared__ uint4 hlw[];      // [NB][SCH][2][64]
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int64_t r_begin = total_rows * blockIdx.x / gridDim.x, r_end = total_rows * (blockIdx.x + 1) / gridDim.x;
  const int sexp = __builtin_amdgcn_readfirstlane(x3s[1]);
  constexpr int64_t MW = 64 * (MB / 2);      // 16-byte mask pieces of one row of a wave
  for (int64_t r = r_begin; r < r_end; ++r) {
    const int64_t tile = r / rows_per_tile, row = r % rows_per_tile;
    const int64_t eb = (row * 4 + wave) * 2;           // the wave's first entity block
    const uint4* ht = Hf3 + tile * ((int64_t)NB * NS * 2 * 64);
    f32x4 acc[2][MB][NB];
#pragma unroll
    for (int M = 0; M < 2; ++M)
#pragma unroll
      for (int m2 = 0; m2 < MB; ++m2) {
        const float4 bv = *(const float4*)(bias_pad + (eb + M) * (16 * MB) + 16 * m2 + 4 * (lane >> 4));
        const f32x4 c = {x3_scale(bv.x, sexp), x3_scale(bv.y, sexp), x3_scale(bv.z, sexp), x3_scale(bv.w, sexp)};
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[M][m2][b] = c;
      }
    W3Frag cur, nxt;
    w3_load(cur, Ef3, eb, NS, 0, lane);
    for (int s0 = 0; s0 < NS; s0 += SCH) {             // workgroup-uniform
      const int ns = NS - s0 < SCH ? NS - s0 : SCH;
      __syncthreads();                                 // every wave has read the previous half
      for (int j = threadIdx.x; j < NB * ns * 128; j += 256) {
        const int b = j / (ns * 128), o = j - b * (ns * 128);
        hlw[b * (SCH * 128) + o] = ht[(b * NS + s0) * 128 + o];
      }
      __syncthreads();
#pragma unroll
      for (int M = 0; M < 2; ++M) {
        for (int sl = 0; sl < ns; ++sl) {
          const int s = s0 + sl;
          // the fragments of the step that follows: this block's next step; at the end of a half the other block's first step of
          // the half (M = 0) or block 0's first step of the next half (M = 1); the row's last request re-reads its own step
          {
            int64_t nblk = eb + M;
            int nstep = s + 1;
            if (sl + 1 == ns) {
              if (M == 0) { nblk = eb + 1; nstep = s0; }
              else if (s0 + ns < NS) { nblk = eb; nstep = s0 + ns; }
              else nstep = s;
            }
            w3_load(nxt, Ef3, nblk, NS, nstep, lane);
          }
          const bool pair = s < NP;
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            const uint4 q0 = hlw[((b * SCH + sl) * 2 + 0) * 64 + lane], q1 = hlw[((b * SCH + sl) * 2 + 1) * 64 + lane];
#pragma unroll
            for (int m2 = 0; m2 < MB; ++m2) acc[M][m2][b] = BX3_MFMA16(cur.a0[m2], q1, acc[M][m2][b]);
#pragma unroll
            for (int m2 = 0; m2 < MB; ++m2) acc[M][m2][b] = BX3_MFMA16(cur.a1[m2], q0, acc[M][m2][b]);
            if (pair) {
#pragma unroll
              for (int m2 = 0; m2 < MB; ++m2) acc[M][m2][b] = BX3_MFMA16(cur.a1[m2], q1, acc[M][m2][b]);
            }
          }
          cur = nxt;
        }
      }
    }
    // ---- epilogue of the row: value V = 4 MB b + 4 m2 + j of block M is entity row 16 m2 + 4 (lane >> 4) + j of the block,
    // query 16 b + (lane & 15) of the tile; its band bit is bit 31 - (V & 31) of word MB M + (V >> 5) (k_band_exact decodes it)
    unsigned mk[2 * MB];
#pragma unroll
    for (int i = 0; i < 2 * MB; ++i) mk[i] = 0u;
    const int64_t unit = (tile * rows_per_tile + row) * 4 + wave;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int64_t q = tile * X3_TILE_Q + b * 16 + (lane & 15);
      float2 tb = make_float2(INFINITY, INFINITY);      // queries beyond the batch: nothing counts, nothing is marked
      if (q < B) tb = tband[q];
      int cg = 0;
#pragma unroll
      for (int M = 0; M < 2; ++M) {
#pragma unroll
        for (int m2 = 0; m2 < MB; ++m2) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int V = 4 * MB * b + 4 * m2 + j;
            const float sc = acc[M][m2][b][j];
            const bool gt = sc > tb.y, ge = sc >= tb.x;
            cg += gt ? 1 : 0;
            if (ge && !gt) mk[MB * M + (V >> 5)] |= 1u << (31 - (V & 31));
          }
        }
        if constexpr (GM) {
          // block maxima per (32 entities, query): the eight values of two consecutive 16-row blocks, over the four row groups
          // of the lanes (lane >> 4)
#pragma unroll
          for (int g = 0; g < MB / 2; ++g) {
            float mx = -INFINITY;
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
              for (int j = 0; j < 4; ++j) mx = fmaxf(mx, acc[M][2 * g + u][b][j]);
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            if (lane < 16) gmax[((eb + M) * (MB / 2) + g) * gm_stride + tile * X3_TILE_Q + b * 16 + lane] = mx;
          }
        }
      }
      int g = cg + __shfl_xor(cg, 16);
      g += __shfl_xor(g, 32);
      if (lane < 16 && q < B && g) atomicAdd(&ng[q], g);
    }
    unsigned any = 0u;
#pragma unroll
    for (int i = 0; i < 2 * MB; ++i) any |= mk[i];
    const bool nz = any != 0u;
    const unsigned long long which = __ballot(nz);
    if (nz) {
#pragma unroll
      for (int i = 0; i < MB / 2; ++i) mask[unit * MW + lane * (MB / 2) + i] = make_uint4(mk[4 * i], mk[4 * i + 1], mk[4 * i + 2], mk[4 * i + 3]);
    }
    if (lane == 0) summ[unit] = which;
  }
}

// at prepare, per handle (as score_kernels_init does for the f32 mode): both forms may ask for the CU's whole LDS on this device
int score_count3_wide_init(coper_handle* h) {
  COPER_HIP_TRY(h, hipFuncSetAttribute((const void*)k_score_count3_wide_bf16x3<0>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  COPER_HIP_TRY(h, hipFuncSetAttribute((const void*)k_score_count3_wide_bf16x3<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  return COPER_OK;
}

// the count launch over queries [q0, q0 + Bc) of the packed batch (arguments: sc3_go, kernels_score3_bf16.hip)
int score_count3_wide_launch(coper_handle* h, int64_t q0, int64_t Bc, int32_t* ng, uint4* mask, unsigned long long* summ, float* gmax,
                             int64_t gm_stride, hipStream_t s) {
  const Dims& dm = h->dm;
  if (dm.KS16 <= X3_KS16_LDS || dm.KS16 > 2 * X3_KS16_LDS) return fail(h, COPER_EUNSUPPORTED, "score_count3 (wide): ent_emb_size not in 321 .. 640");
  if (topk_expand(h) != 1) return fail(h, COPER_ESTATE, "score_count3 (wide): 64-entity block maxima are not generated");
  const int NS = f3_steps(dm.KS16), NP = dm.KS16 / 2, SCH = (NS + 1) / 2;
  const int64_t q_tiles = (Bc + X3_TILE_Q - 1) / X3_TILE_Q;
  const int64_t rows_per_tile = dm.n_eblk * 2 / W3_MB / 8;    // a row: 4 waves x 2 entity blocks of 16 MB rows
  const int64_t total_rows = q_tiles * rows_per_tile;
  int64_t grid = h->num_cus;
  if (grid > total_rows) grid = total_rows;
  const size_t lds = (size_t)W3_NB * SCH * 2 * 64 * sizeof(uint4);
  if (lds > (size_t)160 * 1024) return fail(h, COPER_EUNSUPPORTED, "score_count3 (wide): query half-tile beyond LDS");
  const uint4* hf3 = (const uint4*)h->hf3_ws + (q0 / 16) * NS * 2 * 64;
#define W3_LAUNCH(GM_)                                                                                                                       \
  hipLaunchKernelGGL((k_score_count3_wide_bf16x3<GM_>), dim3((unsigned)grid), dim3(256), lds, s, (const uint4*)h->Ef3, h->bias_pad, hf3,      \
                     (const float2*)h->tband_ws + q0, Bc, NS, NP, SCH, rows_per_tile, total_rows, ng + q0, mask, summ, gmax, gm_stride, h->x3s)
  if (gmax) W3_LAUNCH(1); else W3_LAUNCH(0);
#undef W3_LAUNCH
  COPER_HIP_TRY(h, hipGetLastError());
  return COPER_OK;
}

}  // namespace coper
