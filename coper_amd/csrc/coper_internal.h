// Internal declarations shared by the libcoper_hip.so translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <stdint.h>
#include <deque>
#include <map>
#include <string>
#include <vector>

#include "../../include/coper_hip.h"

// ---- build switches (round 6: pruned) -------------------------------------------------------------------------------------------
// The kernels keep ONE family of compile-time switches: the ablation / clock-stamp set COPER_DBG_* that the measurements of
// DESIGN_LOG.md were made with (a stage removed, a clock stamped per workgroup).  They exist in DIAGNOSTIC builds only: without
// -DCOPER_DIAG every one of them is undefined here, whatever the command line says, so the product library is one program.
// (tools/ab_build.py passes -DCOPER_DIAG with them.)  The variant builds that rounds 2 - 5 measured and rejected -- the bf16 split,
// the fp32-FMA conv of the fused encoder, loads inside the count kernel's asm blocks, buffer loads, the 8-bit second term, the
// old grid layouts ... -- are gone from the sources; their numbers are in DESIGN_LOG.md.  What remains besides are named tunables
// with ONE shipped value (`#ifndef X / #define X value`: COPER_SC3_MB, COPER_TL_WAVES, COPER_FUSED_PBUDGET, ...).
#ifndef COPER_DIAG
#undef COPER_DBG_AMSGRAD_NO_NT
#undef COPER_DBG_BL_CLOCK
#undef COPER_DBG_CLOCK
#undef COPER_DBG_DENSE_NO_DMA
#undef COPER_DBG_DENSE_NO_MFMA
#undef COPER_DBG_FUSED_CLOCK
#undef COPER_DBG_FUSED_EXIT
#undef COPER_DBG_FUSED_NO_CONV
#undef COPER_DBG_FUSED_NO_IMG
#undef COPER_DBG_FUSED_NO_MFMA
#undef COPER_DBG_FUSED_NO_STORE
#undef COPER_DBG_FUSED_NO_W
#undef COPER_DBG_FUSED_NO_XREAD
#undef COPER_DBG_GROUP_CLK
#undef COPER_DBG_NO_EPILOGUE
#undef COPER_DBG_NO_GLOADS
#undef COPER_DBG_NO_GROUP_CHK
#undef COPER_DBG_NO_LDS
#undef COPER_DBG_REG_NO_BAR
#undef COPER_DBG_REG_NO_MFMA
#undef COPER_DBG_REG_NO_X
#undef COPER_DBG_SC3_DUMMY_LDS
#undef COPER_DBG_SC3_EPI_R0
#undef COPER_DBG_SC3_HALF_LDS
#undef COPER_DBG_SC3_LOADS_FIRST
#undef COPER_DBG_SC3_NO_BAND
#undef COPER_DBG_SC3_NO_EPI
#undef COPER_DBG_SC3_ONE_LDS
#undef COPER_DBG_SC3_SKIP_GL
#undef COPER_DBG_SC3_SKIP_LDS
#undef COPER_DBG_TK_OVER
#undef COPER_DBG_TL_CLOCK
#undef COPER_DBG_TL_NOGATHER
#undef COPER_DBG_W128_NO_EPI
#undef COPER_DBG_W128_NO_LOADS
#endif

namespace coper {

// every device allocation of the library goes through these two: a process-wide ledger (pointer -> bytes) behind
// coper_live_device_bytes(), so that a leak shows up as a number and not as a guess from hipMemGetInfo (which also moves with
// the runtime's own scratch and pool decisions)
hipError_t tracked_malloc_impl(void** p, size_t bytes);
hipError_t tracked_free(void* p);
// tracked_malloc_impl of `bytes` for a DevBuf: on failure *p is null, the sticky HIP error is cleared and the handle's error says
// what failed (COPER_ENOMEM)
int devbuf_malloc(coper_handle* h, void** p, size_t bytes, const char* what);

// The owner of one device buffer: a pointer and its capacity in elements, freed when the owner is.  Empty (null, capacity 0) until
// allocated, after reset() and after a failed allocation.  Reads as T* (launch code takes it as the pointer it was before); an
// explicit cast gives the other pointer types the byte planes are read as.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
    return *this;
  }
  ~DevBuf() { reset(); }
  // exactly n elements (at least one), replacing the contents: the old buffer is freed first
  int alloc(coper_handle* h, size_t n, const char* what) {
    reset();
    if (n == 0) n = 1;
    void* p = nullptr;
    if (int rc = devbuf_malloc(h, &p, n * sizeof(T), what)) return rc;
    p_ = (T*)p;
    n_ = n;
    return COPER_OK;
  }
  // at least n elements: nothing happens when they are there
  int ensure(coper_handle* h, size_t n, const char* what) { return n <= n_ ? COPER_OK : alloc(h, n, what); }
  void reset() {
    if (p_) (void)tracked_free(p_);
    p_ = nullptr;
    n_ = 0;
  }
  size_t size() const { return n_; }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  template <typename U>
  explicit operator U*() const { return (U*)p_; }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};


// One parameter of the configuration: what coper_param_spec reports (name, spec_shape) and what coper_set_param registered.
struct Leaf {
  std::string name;
  std::vector<int64_t> spec_shape;
  const float* ptr = nullptr;
  std::vector<int64_t> shape;
  bool set = false;
};

// The leaves of a handle by role, resolved once (enumerate_leaves in coper_abi.hip, at coper_create): launch code reads
// h->lv.<leaf>->ptr and never looks a name up.  A leaf the configuration does not have is null.
struct Leaves {
  struct Bn { Leaf *gamma = nullptr, *beta = nullptr, *moving_mean = nullptr, *moving_variance = nullptr; };
  struct Gen {              // a g_MLP generator: proj[0 .. n_hidden], the last one multiplies the context; bn[i] behind proj[i], i < n_hidden
    int n_hidden = 0;
    Leaf* proj[COPER_MAX_CTX + 1] = {};
    Bn bn[COPER_MAX_CTX];
  };
  Leaf *ent_emb = nullptr, *pred_bias = nullptr, *rel_emb = nullptr /* none under g_lookup */;
  Leaf *conv1_weights = nullptr, *conv1_bias = nullptr;   // static filters or g_lookup tables (none where they are generated)
  Leaf *fc_weights = nullptr, *fc_bias = nullptr;         // static dense layer or g_lookup tables (none where it is generated)
  Bn Conv1BN, FCBN;
  Gen gen[4];               // GenId; empty where the parameter is not generated by a g_MLP
};
enum GenId { GEN_FC_WEIGHTS = 0, GEN_FC_BIAS = 1, GEN_CONV1_WEIGHTS = 2, GEN_CONV1_BIAS = 3 };

// Derived sizes, exactly as ConvE._create_variables derives them (models.py:261-271).
struct Dims {
  int64_t E = 0, R = 0;
  int d = 0, r = 0, emb_h = 0, emb_w = 0;
  int fh = 3, fw = 3, C = 32;
  bool concat_rel = false, lookup = false, gen_conv = false, gen_fc = false, stacked = false, ctx_bn = false;
  int in_h = 0, in_w = 0, Ho = 0, Wo = 0;
  int64_t F_conv = 0, F = 0;
  // padded sizes used by the MFMA layouts
  int64_t F_pad = 0;   // F rounded up to 32 (two 16x16x4 f32 super-steps = one 16x16x32 bf16 k-step)
  int d_pad16 = 0;     // d rounded up to 16 (feature blocks of the dense layer)
  int nfb = 0;         // d_pad16 / 16
  int d_pad8 = 0;      // d rounded up to 8 (k-steps of the score kernels)
  int KS = 0;          // d_pad8 / 8
  int KS16 = 0;        // ceil(d / 16): k-steps of the bf16 MFMA
  int x3_tail = 0;     // how the x3 mode sums the last k-step of an odd KS16 (bf16x3_chain.h: bx3_tail_kind), recorded at coper_create
  int f3_rb = 0;       // registers per 16-row block of the count kernel's images (f3_regs)
  int64_t n_local = 0; // shard rows
  int64_t n_eblk = 0;  // 32-row entity blocks (padded to a multiple of EBLK_ALIGN)
};

// half-width of the exact band of the x3 ranker, relative to |h_q| max|E_e| + max|bias| (per logit; a comparison of two
// logits gets twice that).  The largest error of the mode's logits against the fp32 chain measured over 3e8 logits of the
// FB15k-237-shaped pass (tools/rank_decomp.py): fp16 split 1.8e-7 |h_q||E_e| (rms 1.2e-8) -- the fp32 chain itself is
// 2.3e-7 from float64 --; round 2's bf16 split: 3.3e-6 (rms 3.1e-7).  The default keeps a factor 5 above
// the worst case seen, 80 (30) sigma.  coper_config.rank_band_kappa overrides them; the proven worst case of the split and
// of fp32 accumulation in any order is 3 * 2^-22 (2^-16) + 2 (3 * 16 KS16 + 1) 2^-24 ~ 7.5e-5 (1.2e-4) at d = 200.
constexpr float COPER_BAND_KAPPA_DEFAULT = 1e-6f;
constexpr int COPER_TOPK_PRUNED_MAX = 128;   // largest k served by the block-maxima top-k (bf16x3); above: logits chunks
constexpr int BAND_NCONST = 8;
// the check words of a grouping prepared ahead (group_body.h: the guard), 64-bit each
enum { GROUP_CHK_REL = 0, GROUP_CHK_E1 = 1, GROUP_CHK_PERM = 2, GROUP_CHK_LO = 3, GROUP_CHK_NLOCAL = 4, GROUP_CHK_RALL = 5,
       GROUP_CHK_STALE = 6, GROUP_CHK_WORDS = 8 };
constexpr int EBLK_ALIGN = 16;  // entity blocks consumed per workgroup iteration in score_count (8 waves x 2)
// what the build pass of the known-facts index counts (kernels_known.hip); coper_set_known_facts reports the tail_indptr kinds first
enum { KNOWN_BAD_ORDER = 0, KNOWN_BAD_DUP = 1, KNOWN_BAD_E1 = 2, KNOWN_BAD_REL = 3, KNOWN_BAD_TAIL = 4, KNOWN_BAD_ASC = 5,
       KNOWN_BAD_IP0 = 6, KNOWN_BAD_IP_DECR = 7, KNOWN_BAD_IPN = 8, KNOWN_BAD_KINDS = 9, KNOWN_BAD_WORDS = 16 };

// The workspaces of the pruned top-k, sized by a TopkPlan (below) and reserved by ensure() beside the launchers that use them
// (kernels_topk_bf16.hip).  The slot counts are the plan's: T64 = k_blocks * B + nnz candidate blocks, T of them as 32-entity slots.
struct TopkPlan;
struct TopkWs {
  DevBuf<float> gmax_ws;           // [Gm][query chunk]: block maxima written by the count pass
  size_t cand_cap = 0;             // the candidate slots T the group of four below holds (0 while any of it is missing)
  DevBuf<int32_t> cand_blk_ws;     // [list_len] candidate blocks, query q's at k_blocks*q + indptr[q]
  DevBuf<float> cand_val_ws;       // [T][32] their logits
  DevBuf<int32_t> cand_q_ws;       // [list_len] the query of every candidate slot
  DevBuf<int32_t> cand_sorted_ws;  // [sorted_cap] candidate slots grouped by entity block, 32-padded per block
  DevBuf<char> tk_coarse_ws;       // the threshold kernel's coarse level (coarse_bytes)
  DevBuf<uint32_t> cand_tau_ws;    // [B] selection threshold per query (ordered float bits; 0: none)
  DevBuf<int32_t> blk_cnt_ws;      // [2 GV] slots per (block, segment) | scatter cursors
  DevBuf<int32_t> blk_off_ws;      // [GV + 1] their offsets | the scan's chunk sums
  int ensure(coper_handle* h, const TopkPlan& p, hipStream_t s);
  bool holds(const TopkPlan& p) const;
};
// coper_predict_topk's own workspaces (kernels_topk_bf16.hip: the predict section)
struct PredictWs {
  DevBuf<int64_t> pred_ids_ws;     // [B] -1: "no target" for the kernels that exempt e2 from the filter | [B + 1] zeros: the raw call's CSR
  DevBuf<int32_t> pred_q_ws;       // [B] chain re-scores of the query (-1: unresolved) | [B] its audit ratio's float bits | [B] unresolved queries
  DevBuf<uint32_t> pred_stats;     // [8] since the last reset: [0] unresolved queries, [2] largest audit ratio (float bits), [4] unresolved of the
                                   //   running call, [6..7] chain re-scores (64 bit); zeroed when allocated
  DevBuf<float> pred_rows_ws;      // [workgroups][n_local] chain logits of the unresolved queries being served
  int64_t pred_queries = 0;        // queries answered since the last reset (host count)
  int ensure(coper_handle* h, int64_t B, hipStream_t s);
};

struct Timer {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  double total_ms = 0.0;
  int64_t launches = 0;
};

}  // namespace coper

struct coper_handle {
  coper_config cfg;
  coper::Dims dm;
  std::deque<coper::Leaf> leaves;    // one per parameter, in spec order; a deque: the elements (and the names handed out) never move
  coper::Leaves lv;                  // the same leaves by role
  std::string err;
  bool prepared = false;

  // ---- derived device buffers (owned) ----
  coper::DevBuf<float> conv_scale;  // [C]   folded Conv1BN
  coper::DevBuf<float> conv_shift;
  coper::DevBuf<float> fc_scale;    // [d]   folded FCBN
  coper::DevBuf<float> fc_shift;
  coper::DevBuf<float> conv_w_rel;  // [R, fh*fw, C] generated / looked-up conv filters (gen_conv)
  coper::DevBuf<float> conv_b_rel;  // [R, C]
  coper::DevBuf<float> fc_b_rel;    // [R, d]  (gen_fc)
  coper::DevBuf<float> Wf;          // dense weights, fragment-major: [Rw][nfb][F_pad/16][64] float4
  int64_t Rw = 0;                   // R when gen_fc else 1
  coper::DevBuf<float> Ef;          // entity table, fragment-major: [n_eblk][KS][64] float4
  coper::DevBuf<float> bias_pad;    // [n_eblk*32], -inf padded
  coper::DevBuf<uint4> Wf16_hi;     // COPER_SCORE_BF16X3: dense weights as hi / lo bf16 planes (16x16x32 fragment order)
  coper::DevBuf<uint4> Wf16_lo;
  bool enc_bf16 = false;            // encoder runs in bf16x3 (needs 3x3 filters, C % 8 == 0)
  coper::DevBuf<uint4> Ef16_hi;     // COPER_SCORE_BF16X3: entity table hi / lo bf16 planes, fragment-major
  coper::DevBuf<uint4> Ef16_lo;     //   [n_eblk][KS16][64] x 16 B
  coper::DevBuf<uint4> Erm16_hi;    //   row-major twins [n_eblk*32][KS16*16] bf16 (pair kernel gathers)
  coper::DevBuf<uint4> Erm16_lo;
  coper::DevBuf<uint4> Ef3;         //   the count kernel's image (bf16x3_chain.h): [2 n_eblk][NS][2][64] x 16 B, zero-filled first
  coper::DevBuf<unsigned> band_consts;   // [BAND_NCONST] float bits: [0] max |E_e|_2, [1] max |pred_bias| of the shard (exact band), [2] max |E element|,
                                     //   [3] the band audit's largest |x3 - chain| / (tau / 2), [4] its pair count (coper_band_audit)
  float band_kappa_mult = 1.f;       // coper_band_policy: a power of two on top of the configured kappa (kept across coper_prepare)
  unsigned band_launches = 0;        // count launches since prepare (which of them the band audit rides on: kernels_score3_bf16.hip)
  int img_exp = 0;                   // e_I: the fused encoder's image planes (compute_x_exp)
  int x3_ent_exp = 0;                // e_E: the entity planes hold E 2^e_E (split16.h; prepare)
  float x3_ent_absmax = 0.f;         //   the maximum it was chosen from (the shard's, or coper_config.x3_ent_absmax)
  // coper_group_next: grouping arrays in sets.  Set 0 is HOME (the owners in `home`: every pass that groups itself, and every captured
  // graph, uses it); sets 1 and 2 are written by the grouping role of a fused encoder launch for the NEXT pass while the running
  // pass reads its own.  grouping() is the set of the pass being enqueued.
  struct HomeSet {
    coper::DevBuf<int32_t> counts;   // [3 (R+2) + 4]: rel_count of set 0 | rel_count_acc() | rel_cursor() | group_done() (ensure_workspace)
    coper::DevBuf<int32_t> rel_offset, perm, inv_perm, sorted_row, sorted_rid, tiles, n_tiles;
    coper::DevBuf<float> x3m;        // [X3M_SLOTS] per-block maxima of the h rows being packed (bf16x3_chain.h; allocated by coper_prepare)
  } home;
  struct GroupSet {
    coper::DevBuf<int32_t> slab;     // sets 1, 2: one allocation; set 0: empty (its arrays are `home`)
    coper::DevBuf<char> fin;         // the set's FusedFinConst: the fused encoder's finalize constants (fused_fin_update)
    // views: into slab, or into `home` for set 0 (group_home_views)
    int32_t* rel_count = nullptr;    // [R+2] counts of the LAST grouping call (+ the out-of-range counter at R+1)
    int32_t* rel_offset = nullptr;   // [R+1]
    int32_t* perm = nullptr;         // [B] sorted position -> query
    int32_t* inv_perm = nullptr;     // [B] query -> sorted position
    int32_t* sorted_row = nullptr;   // [B] sorted position -> local entity row of e1 (or the e1_rows row), -1 = not on this shard
    int32_t* sorted_rid = nullptr;   // [B] sorted position -> validated relation id
    int32_t* tiles = nullptr;        // [T_max*4] (rel, start, n, pad)
    int32_t* n_tiles = nullptr;      // [2] #small tiles, #big 16-query blocks
    float* x3m = nullptr;
    const int32_t* fused_fin_perm = nullptr;   // the perm `fin` was written for (the workspace generation)
    int64_t* chk = nullptr;          // sets 1, 2: [GROUP_CHK_WORDS] what the grouping role sorted (group_body.h: the guard of a prepared grouping)
  } gset[3];
  int gcur = 0;                      // the set of the pass being enqueued
  const GroupSet& grouping() const { return gset[gcur]; }
  // views into home.counts (null until the workspace exists)
  int32_t* counts_part(int i) const { return home.counts ? home.counts.get() + i * (dm.R + 2) : nullptr; }
  int32_t* rel_count_acc() const { return counts_part(1); }   // [R+2] the accumulation buffer of k_rel_hist_scan (zero between calls)
  int32_t* rel_cursor() const { return counts_part(2); }      // [R]
  int32_t* group_done() const { return counts_part(3); }      // ticket counter of the histogram launch (its last block runs the scan)
  // The jobs a host registers for a LATER launch of this handle, and the grouping a launch prepared ahead: ONE owner, one
  // invalidation rule (the drop rules used to be spread over five places).
  //   stage  (coper_stage_ids_next): a batch to bring in beside the next fused encoder launch            n > 0: pending
  //   post   (coper_post_i32_next):  int32 results to copy out beside the next pass's first launch       n > 0: pending
  //   gnext  (coper_group_next):     id arrays of the pass AFTER the next one, to be sorted inside the next fused encoder launch
  //   gdone: a grouping launched ahead into set `set`; the pass that comes with exactly these pointers consumes it -- and CHECKS it
  //          on the device against the live ids (PassCtx::chk)
  // Lifetimes: stage / post name buffers the caller owns and stay pending until a launch carries them (an eager pass, or post_flush /
  // a launch of their own where no launch can carry them); gnext is for the NEXT encode / encode_rank call only; gdone is for the
  // call after that only.  invalidate_grouping() -- coper_prepare, a training step, a growing workspace, freed grouping sets -- drops
  // gnext and gdone together; nothing else does.
  struct PassPipeline {
    struct { const int32_t* src = nullptr; int64_t n = 0; int64_t* dst = nullptr; } stage;
    struct { const int32_t* src = nullptr; int64_t n = 0; int32_t* dst = nullptr; } post;
    struct { const int64_t* e1 = nullptr; const int64_t* rel = nullptr; int64_t B = 0; int rows = 0;
             bool pending = false; } gnext;   // pending: registered, not yet launched
    struct { const int64_t* e1 = nullptr; const int64_t* rel = nullptr; int64_t B = 0; int rows = 0;
             bool done = false; int set = 0; } gdone;
    void invalidate_grouping() { gnext.pending = false; gdone.done = false; }
    // the next call's view of a grouping prepared ahead: consumed (true) or dropped -- never kept for a later call
    bool take_prepared(const int64_t* e1, const int64_t* rel, int64_t B, int rows, int* set) {
      const bool hit = gdone.done && gdone.rel == rel && gdone.e1 == (rows ? nullptr : e1) && gdone.B == B && gdone.rows == rows;
      gdone.done = false;
      *set = hit ? gdone.set : 0;
      return hit;
    }
    int64_t take_stage() { const int64_t n = stage.n; stage.n = 0; return n; }
    int64_t take_post() { const int64_t n = post.n; post.n = 0; return n; }
  } pipe;
  int64_t stale_passes_host = 0;     // coper_stale_passes: what the device counter (group_done() + 2) held when a growing workspace replaced it
  coper::DevBuf<int32_t> w_exp;      // [R or 1] e_W per relation id: the dense-weight planes hold W_r 2^e_W (split16.h; prepare)
  int w_div = 1, w_rem = 0;          // coper_config.rel_mod_*: the weight planes hold the relations r with r % w_div == w_rem, relation r at slot r / w_div
  int x_exp = 0;                     // e_x: the conv activations enter the dense layer as x 2^e_x (from a bound; prepare)
  coper::DevBuf<int32_t> x3s;        // [4] the packed batch's exponents: [0] e_h, [1] e_E + e_h (bf16x3_chain.h)
  coper::DevBuf<float> ctx_tmp[2];   // generator hidden activations
  // ---- COPER_DENSE_FACTORED (kernels_dense_factored_bf16.hip): no W_r cache; built by coper_prepare from the configuration
  bool factored = false;             // coper_config.dense_mode == COPER_DENSE_FACTORED
  int fac_K = 0;                     // width of the fc_weights generator's context
  coper::DevBuf<float> fac_ctx;      // [R, fac_K] that context (rel_emb itself for g_linear)
  coper::DevBuf<uint4> fac_P_hi;     // the generator's last projection as GEMM operand planes: rows (rho, k), contraction f
  coper::DevBuf<uint4> fac_P_lo;
  coper::DevBuf<int32_t> fac_exp;    // [4] device words: [0] e_P, [1] e_x (= x_exp), [2..3] the pack's reduction scratch
  int64_t fac_chunk = 0;             // queries per GEMM (the slices of T stay within 256 MB)
  int fac_nsplit = 1;                // K slices of the product
  int fac_variant = 0;               // TgVariant of the product
  coper::DevBuf<uint4> fac_x_hi;     // workspace: the chunk's x operand planes
  coper::DevBuf<uint4> fac_x_lo;
  coper::DevBuf<float> fac_T;        // workspace: [fac_nsplit][chunk][fac_K d] the product's K slices

  // ---- workspace (owned, grown lazily) ----
  int64_t ws_queries = 0;         // the capacity of the workspace group of ensure_workspace: 0 while any of it is missing
  int64_t ws_nnz = 0;
  int ws_ksplit = 0;
  coper::DevBuf<int32_t> blk_off; // [R+1] exclusive scan of the big groups' block counts
  coper::DevBuf<float> x_sorted;  // [B, F_pad]
  coper::DevBuf<float> z_part;    // [ksplit, B, d_pad16]
  coper::DevBuf<float> tgt_ws;    // [B]
  coper::DevBuf<int32_t> cnt_ws;  // [2B]
  coper::DevBuf<float> h_ws;      // internal h of coper_encode_rank when the caller does not want it (fp32 mode)
  coper::DevBuf<float> logits_ws; // top-k path only: [chunk_rows, n_local]
  int64_t gmax_max_floats = (int64_t)1 << 28;   // most block maxima held at a time; set from the device memory size at prepare
  coper::TopkWs topk;                   // pruned top-k (k <= COPER_TOPK_PRUNED_MAX) and
  coper::PredictWs pred;                //   coper_predict_topk: reserved and used in kernels_topk_bf16.hip
  coper::DevBuf<uint4> hfrag16_hi;      // bf16x3: h hi / lo planes in fragment order
  coper::DevBuf<uint4> hfrag16_lo;
  coper::DevBuf<uint4> hrm16_hi;        //   row-major twins
  coper::DevBuf<uint4> hrm16_lo;
  coper::DevBuf<uint4> hf3_ws;          //   the count kernel's query image [ceil(B/128) * 8][NS][2][64] x 16 B (zero-filled at allocation)
  coper::DevBuf<float> tband_ws;        // [B] float2 {t_lo, t_hi}: the exact band around the mode's target logit
  coper::DevBuf<float> tgtx_ws;         // [B] exact-chain targets of the two-call flows
  coper::DevBuf<char> mask_ws;          // band bits of one count launch (kernels_score3_bf16.hip)
  coper::DevBuf<int32_t> row_of_ws;     // bf16x3: CSR entry -> query row [nnz]
  coper::DevBuf<int32_t> heavy_ws;      // fused tail: [0] number of listed blocks, [1] finished workgroups, [2..] 32-query blocks whose CSR entries
                                        //   exceed what their workgroup corrects itself (k_filter_excess_bf16x3); zero between passes
  coper::DevBuf<float> hfrag_ws;        // h re-packed in MFMA-fragment order [ceil(B/128)*4][KS][64] float4
  // ---- the known-facts index (coper_set_known_facts; kernels_known.hip): copies of the caller's arrays, no function of the
  // parameters -- coper_prepare, training steps and coper_reserve leave it alone
  int64_t known_n_keys = 0;             // rows of the index; 0: none set
  int64_t known_nnz = 0;
  bool known_wide = false;              // tails held as int64 (num_ent beyond int32) instead of int32
  coper::DevBuf<int64_t> known_keys;    // [n_keys] e1 * num_rel + rel, ascending
  coper::DevBuf<int64_t> known_indptr;  // [n_keys + 1]
  coper::DevBuf<char> known_tails;      // [nnz] int32 or int64 (known_wide) global ids, ascending within a row
  coper::DevBuf<int32_t> known_row_ws;  // [B] the index row of every query of the running lookup, -1: none
  coper::DevBuf<int64_t> known_ip_ws;   // [B + 1], [nnz]: the CSR the fused entry points (coper_predict_topk_known,
  coper::DevBuf<int64_t> known_ix_ws;   //   coper_encode_rank_known) look up and hand to the bodies of the explicit-CSR calls
  int num_cus = 256;
  void* train = nullptr;          // coper::TrainState (coper_train.hip)
  bool dense_attr_done = false;
  bool fused_attr_done = false;

  bool profile = false;
  std::map<std::string, coper::Timer> timers;
  std::vector<hipEvent_t> event_pool;   // recycled by coper_profile_read
};

namespace coper {

// what the encoder's launches read: the per-relation buffers coper_prepare derived where the parameter is generated or looked up,
// the registered tensor where it is static; rel_emb is null under g_lookup
inline const float* conv_w(const coper_handle* h) { return h->dm.gen_conv ? h->conv_w_rel.get() : h->lv.conv1_weights->ptr; }
inline const float* conv_b(const coper_handle* h) { return h->dm.gen_conv ? h->conv_b_rel.get() : h->lv.conv1_bias->ptr; }
inline const float* fc_b(const coper_handle* h) { return h->dm.gen_fc ? h->fc_b_rel.get() : h->lv.fc_bias->ptr; }
inline const float* rel_emb_or_null(const coper_handle* h) { return h->lv.rel_emb ? h->lv.rel_emb->ptr : nullptr; }

struct FilterArgs {         // the filter role's view of a pass (queries of one count launch: all pointers at its first query)
  const float* hvec; const uint4* Ehi; const uint4* Elo; const float* bias_pad; const int64_t* e2; const int64_t* indptr;
  const int64_t* idx; const float2* tband; int32_t* ranks; int32_t* heavy; const int32_t* x3s; int64_t B, n_local; int d;
};

// What the launches of one API call hand each other.  It lives on the entry point's stack and is passed to the launch helpers of
// the pass; a helper called outside a ranking pass gets a default one.  coper_handle holds only what outlives a call.
struct PassCtx {
  // coper_rank / coper_encode_rank: the pack launch presets the [B] rank counters cnt to base (and eq to 0), so n_greater
  // accumulates straight into `ranks` from 1; preset: they are, and the count pass on cnt skips its zeroing launch
  int32_t* cnt = nullptr;
  int32_t* eq = nullptr;
  int32_t base = 0;
  bool preset = false;
  // the target pass also writes row_of_ws for this CSR; expanded: it did, and the filter correction reads them
  const int64_t* csr = nullptr;
  bool expanded = false;
  // what the query planes were packed from in this call (the count pass of the same call reuses them)
  const float* packed_hvec = nullptr;
  int64_t packed_B = 0;
  // the filter-excess role, deferred to the next band launch (kernels_score3_bf16.hip)
  bool excess_pending = false;
  FilterArgs excess = {};
  // the fused tail left the whole filter correction to the look-up role of the band launches (filter_bits_supported): the count
  // launches of the pass store their gt plane
  bool gt_bits = false;
  // the pass runs on a grouping prepared ahead: the set's check words (its tiles compare the live ids with what was sorted; the
  // kernels that preset the rank counters read the verdict); nullptr: the pass grouped itself
  int64_t* chk = nullptr;
  bool post_here = false;    // pipe.post rides in the fused encoder launch (the pass was grouped ahead: no grouping launch carries it)
  bool gnext_ride = false;   // pipe.gnext rides in the fused encoder launch (sets 1, 2 are allocated)
};

int fail(coper_handle* h, int code, const std::string& msg);
void train_destroy(coper_handle* h);   // coper_train.hip
int train_params_changed(coper_handle* h, const char* leaf_name);   // coper_set_param: the training state resolves its variables again
// deferred rows (coper_train_defer_rows): every row of ent_emb / pred_bias and their slots current before a call reads or replaces the
// tables whole; device_wide: for a call without a stream (null stream between two device synchronisations).  No-op with the mode off.
int train_rows_sync(coper_handle* h, void* stream, bool device_wide);
int hip_fail(coper_handle* h, hipError_t e, const char* what);

#define COPER_HIP_TRY(h, expr)                                    \
  do {                                                            \
    hipError_t _e = (expr);                                       \
    if (_e != hipSuccess) return coper::hip_fail((h), _e, #expr); \
  } while (0)

// Growing buffers that launches already on the stream may read: the stream is synchronised once, before the first buffer that is
// replaced, and not at all when every buffer holds.  b gets max(need, rounded) elements when it has fewer than `need`.
struct StreamGrow {
  coper_handle* h; hipStream_t s; bool synced = false;
  int sync() { if (!synced) COPER_HIP_TRY(h, hipStreamSynchronize(s)); synced = true; return COPER_OK; }
  template <typename T> int operator()(DevBuf<T>& b, size_t need, const char* what, size_t rounded = 0) {
    if (need <= b.size()) return COPER_OK;
    if (int rc = sync()) return rc;
    return b.alloc(h, need > rounded ? need : rounded, what);
  }
};

// kernels_prepare.hip
int launch_fold_bn(coper_handle* h, const float* gamma, const float* beta, const float* mean, const float* var,
                   int n, float eps, float* scale, float* shift, hipStream_t s);
// out[rel, n] = act( sum_k ctx[rel,k] * P[k,n] ), optional BN+ReLU epilogue (generator hidden layers,
// conv filters/biases, dense bias): small N.
int launch_gen_small(coper_handle* h, const float* ctx, int64_t R, int K, const float* P, int64_t N,
                     const float* bn_scale, const float* bn_shift, bool relu, float* out, hipStream_t s);
// dense weights into fragment-major Wf.  mode 0: sum_k ctx[rel,k]*P[k, f*d+i]; mode 1: P[rel, f*d+i] (lookup
// and static: ctx == nullptr).
int launch_gen_dense_frag(coper_handle* h, const float* ctx, int64_t R, int K, const float* P, int mode,
                          float* Wf, hipStream_t s);
int launch_entity_frag(coper_handle* h, const float* ent, const float* bias, hipStream_t s);

// kernels_encode.hip
int launch_group_by_relation(coper_handle* h, const int64_t* e1, const int64_t* rel, bool have_e1_rows, int64_t B, int tq,
                             hipStream_t s);
int launch_conv(coper_handle* h, const int64_t* e1, const int64_t* rel, const float* e1_rows, int64_t B,
                hipStream_t s);
int launch_dense(coper_handle* h, const int64_t* rel, int64_t B, int tq, int ksplit, float* h_out, hipStream_t s);
int launch_copy_i32(coper_handle* h, const int32_t* src, int64_t n, int32_t* dst, hipStream_t s);
int launch_pack_owned_rows(coper_handle* h, const float* ent, const float* bias, const int64_t* loc, int64_t n, int64_t cap, float hdr0, float hdr1,
                           float* buf, hipStream_t s);
int launch_unpack_rows(coper_handle* h, const float* all, const int64_t* take1, const int64_t* take2, int64_t B, float* g1, float* g2, float* b2,
                       hipStream_t s);
int launch_pack_shard_record(coper_handle* h, const int32_t* ng, const int32_t* ne, const float* tv, const int64_t* ti, int64_t B, int k,
                             unsigned* audit, int reset, int64_t* rec, hipStream_t s);
int launch_merge_shard_records(coper_handle* h, const int64_t* all, int world, int64_t B, int k, int32_t* ranks, int32_t* ne, float* vals,
                               int64_t* ids, hipStream_t s);
int launch_copy_i32_audit(coper_handle* h, const int32_t* src, int64_t n, int32_t* dst, unsigned* audit, int reset, hipStream_t s);
int launch_widen_ids(coper_handle* h, const int32_t* src, int64_t n, int64_t* dst, hipStream_t s);
int launch_gather_entities(coper_handle* h, const int64_t* ids, int64_t B, float* out, hipStream_t s);

// kernels_score.hip
int launch_score_all(coper_handle* h, const float* hvec, int64_t B, float* logits, int64_t ld, hipStream_t s);
int launch_score_count(coper_handle* h, const float* hvec, const float* tgt, int64_t B, int32_t* ng, int32_t* ne,
                       hipStream_t s);
int launch_pair_targets(coper_handle* h, const float* hvec, const int64_t* e2, int64_t B, float* tgt, hipStream_t s);
int launch_filter_correct(coper_handle* h, const float* hvec, const float* tgt, const int64_t* e2,
                          const int64_t* indptr, const int64_t* idx, int64_t nnz, int64_t B, int32_t* ng,
                          int32_t* ne, hipStream_t s);
int launch_score_lookup(coper_handle* h, const float* hvec, const int32_t* lookup, int64_t B, int64_t L, float* out,
                        hipStream_t s);
int launch_finish_ranks(coper_handle* h, const int32_t* ng, int64_t B, int32_t* ranks, hipStream_t s);
int score_kernels_init(coper_handle* h);
// kernels_score_bf16.hip (COPER_SCORE_BF16X3)
int launch_rows_to_frag_bf16(coper_handle* h, PassCtx& ctx, const float* src, int64_t n_rows, int64_t n_blk, uint4* hi, uint4* lo,
                             uint4* rm_hi, uint4* rm_lo, uint4* f3, bool query_side, hipStream_t s);
int launch_pack_h_bf16(coper_handle* h, PassCtx& ctx, const float* hvec, int64_t B, hipStream_t s);
int launch_absmax_publish(coper_handle* h, const float* src, int64_t n, hipStream_t s);
int launch_score_count_bf16x3(coper_handle* h, PassCtx& ctx, const float* hvec, const float* tgt_x, const int64_t* e2, const int64_t* indptr,
                              const int64_t* idx, int64_t B, int32_t* ng, int32_t* ne, hipStream_t s);
int launch_score_all_bf16x3(coper_handle* h, const float* hvec, int64_t B, float* logits, int64_t ld, hipStream_t s);
int launch_pair_targets_bf16x3(coper_handle* h, PassCtx& ctx, const float* hvec, const int64_t* e2, int64_t B, float* tgt,
                               hipStream_t s);
int launch_score_lookup_bf16x3(coper_handle* h, const float* hvec, const int32_t* lookup, int64_t B, int64_t L,
                               float* out, hipStream_t s);
int launch_filter_correct_bf16x3(coper_handle* h, const PassCtx& ctx, const int64_t* e2, const int64_t* indptr, const int64_t* idx, int64_t nnz,
                                 int64_t B, int32_t* ng, hipStream_t s);
int score_bf16_kernels_init(coper_handle* h);
// queries whose block maxima are held at a time: at most `cap_floats` (1/32 of the device memory, at least 1 GiB;
// the threshold kernel runs one workgroup per 16 or 32 queries, so short chunks leave the chip idle) or one tile
inline int64_t topk_chunk_queries(int64_t n_eblk, int64_t B, int64_t cap_floats) {
  int64_t qc = cap_floats / n_eblk / 128 * 128;
  if (const char* e = getenv("COPER_TOPK_CHUNK_QUERIES")) qc = atoll(e) / 128 * 128;   // tests: force several chunks
  if (qc < 128) qc = 128;
  const int64_t Bpad = (B + 127) / 128 * 128;
  return qc > Bpad ? Bpad : qc;
}
// Geometry of the top-k threshold kernel (kernels_topk_bf16.hip): a workgroup of TK_THREADS threads per strip of 4 x QV queries
// (QV = 4 or 8), the block axis divided among TK_THREADS / QV sub-ranges.
constexpr int TK_THREADS = 512;
constexpr int tk_strip_queries(int QV) { return 4 * QV; }
constexpr int tk_sub_ranges(int QV) { return TK_THREADS / QV; }
inline int64_t tk_strips(int64_t qs, int QV) { return (qs + tk_strip_queries(QV) - 1) / tk_strip_queries(QV); }
// Its coarse level (round 5): one key per TK_GRP visits of a thread, i.e. 1/16 of the block maxima of a query chunk.
constexpr int TK_GRP = 16;
constexpr int64_t TK_COARSE_MIN_BLOCKS = 16384;       // below: the block axis is too short for the route to pay
inline int64_t tk_coarse_groups(int64_t G, int QV) {  // coarse keys a thread writes
  return ((G + tk_sub_ranges(QV) - 1) / tk_sub_ranges(QV) + TK_GRP - 1) / TK_GRP;
}
inline size_t tk_coarse_bytes(int64_t G, int64_t qs, int QV) {   // four keys (a thread's four queries) per thread, group and strip
  return (size_t)tk_strips(qs, QV) * tk_coarse_groups(G, QV) * TK_THREADS * sizeof(uint4);
}
// counters per block for the grouping of candidate slots: few blocks = many slots per block = contended atomics
inline int topk_nseg(int64_t n_eblk) { return n_eblk < 4096 ? 8 : 1; }
// Large tables: the x3 count kernel writes one block maximum per 64 entities instead of 32 (kernels_score3_bf16.hip: GM = 2),
// the threshold kernel selects 64-entity candidate blocks and k_topk_expand64 turns each into its two 32-entity halves for
// everything downstream -- half the bytes of the three threshold sweeps against twice the re-scoring.  Measured crossover
// between WN18RR's 41 K entities (equal) and a 1.25 M-row shard (-0.3 ms of 7.1): from 65,536 local rows on.
inline int topk_expand(const coper_handle* h) {
  const char* force = getenv("COPER_TOPK_EXPAND");             // A/B and tests: "1" / "2" (read per call; set it before the handle's first top-k call and keep it)
  if (h->cfg.score_mode == COPER_SCORE_F32) return 1;
#if defined(COPER_SC3_MB) && COPER_SC3_MB != 4
  return 1;                                                    // (A/B builds with another block count per wave: no 64-entity form generated)
#endif
  if (h->dm.KS16 != 13 && h->dm.KS16 != 16) return 1;          // (the 64-entity form is instantiated for d = 200 and 256 only: build time)
  if (force && (force[0] == '1' || force[0] == '2')) return force[0] - '0';
  return h->dm.n_local >= 65536 ? 2 : 1;
}
// The geometry of one pruned top-k call, computed once (topk_plan) and read by the reservation (TopkWs::ensure), the launchers and
// the entry points: no size of the top-k is written anywhere else.  The f32 mode is the same plan with XF == 1.
constexpr int TK_SCAN_CHUNK = 4096;   // counters per workgroup of the long block scan: 256 threads x 16
struct TopkPlan {
  int64_t B = 0;
  int k_blocks = 0;         // candidate blocks per query beside its filter entries: k (the ranker), k + PREDICT_SLACK (the x3 predictor)
  int XF = 1;               // 2: the count kernel writes 64-entity maxima (topk_expand), candidates are expanded to 32-entity slots
  int64_t G = 0, Gm = 0;    // 32-entity blocks | rows of gmax: G / XF (n_eblk is a multiple of 16)
  int nseg = 1;             // counters per block for the grouping of candidate slots (topk_nseg)
  int64_t GV = 0, qc = 0;   // (block, segment) counters: G * nseg | queries whose block maxima are held at a time
  int64_t T64 = 0, T = 0;   // candidate blocks: k_blocks + (filter entries) per query | ... as 32-entity slots: XF * T64
  size_t list_len = 0;      // cand_blk / cand_q: T (+ the 64-entity level's own lists, behind the expanded ones)
  size_t sorted_cap = 0;    // the block-grouped slot list: every (block, segment) with candidates is padded to a multiple of 32
  size_t coarse_bytes = 0;  // the coarse level for Gm blocks x qc queries, for either strip width; 0: no coarse route
  size_t cand_val_len = 0, gmax_floats = 0, blk_cnt_len = 0, blk_off_len = 0;
  int64_t scan_tmp_cap = 0; // chunk sums of the long block scan, behind blk_off
  bool fits = false;        // slot ids are int32
};
inline TopkPlan topk_plan(const coper_handle* h, int64_t B, int64_t k_blocks, int64_t filt_nnz) {
  TopkPlan p;
  p.B = B; p.k_blocks = (int)k_blocks; p.XF = topk_expand(h);
  p.G = h->dm.n_eblk; p.Gm = p.G / p.XF;
  p.nseg = topk_nseg(p.G); p.GV = p.G * p.nseg; p.qc = topk_chunk_queries(p.G, B, h->gmax_max_floats);
  p.T64 = k_blocks * B + filt_nnz; p.T = p.XF * p.T64;
  p.list_len = (size_t)(p.T + (p.XF > 1 ? p.T64 : 0));
  p.sorted_cap = (size_t)((p.T + 31 * (p.GV < p.T ? p.GV : p.T) + 31) / 32 * 32);
  p.cand_val_len = (size_t)(32 * p.T); p.gmax_floats = (size_t)(p.Gm * p.qc);
  if (p.Gm >= TK_COARSE_MIN_BLOCKS) p.coarse_bytes = std::max(tk_coarse_bytes(p.Gm, p.qc, 4), tk_coarse_bytes(p.Gm, p.qc, 8));
  p.scan_tmp_cap = p.GV / TK_SCAN_CHUNK + 2; p.blk_cnt_len = (size_t)(2 * p.GV); p.blk_off_len = (size_t)(p.GV + 1 + p.scan_tmp_cap);
  p.fits = p.T + 32 * p.GV < 0x7fffffffLL;
  return p;
}
void score_count_begin_bf16x3(const PassCtx& ctx, int64_t B, int32_t* ng, int32_t* ne, hipStream_t s);
// kernels_score3_bf16.hip: the count kernel (16x16x32, software-pipelined, one wave per SIMD) and the exact band
int score_count3_chunk_bf16x3(coper_handle* h, PassCtx& ctx, int64_t q0, int64_t Bc, const float* hvec, const float* tgt_x, const int64_t* e2,
                              const int64_t* indptr, const int64_t* idx, int32_t* ng, int32_t* ne, float* gmax, int64_t gm_stride,
                              hipStream_t s);
size_t score_count3_mask_bytes(const coper_handle* h, int64_t Bc);
size_t score_count3_mask_words_bytes(const coper_handle* h, int64_t Bc);     // one plane: a bit per logit of the launch
// The count kernels hold the fragments of a 128-query tile in the CU's 160 KiB of LDS: whole up to KS16 = 20 / KS = 40
// (ent_emb_size <= 320), in two halves of K beyond that (kernels_score3_wide_bf16.hip, k_score_count_wide_f32) -- up to
// ent_emb_size = 640, the bound coper_create enforces.
constexpr int X3_TILE_Q = 128;        // queries per tile of either count kernel
constexpr int X3_KS16_LDS = 20;       // k-steps of 16 whose f3 tile fits LDS (x3 mode)
constexpr int F32_KS_LDS = 40;        // k-steps of 8 whose fp32 tile fits LDS (f32 mode)
constexpr int COPER_MAX_ENT_EMB = 16 * 2 * X3_KS16_LDS;
int score_count3_wide_init(coper_handle* h);      // per handle, at prepare: the launch's dynamic-LDS limit on the handle's device
int score_count3_wide_launch(coper_handle* h, int64_t q0, int64_t Bc, int32_t* ng, uint4* mask, unsigned long long* summ, float* gmax,
                             int64_t gm_stride, hipStream_t s);
int launch_band_consts(coper_handle* h, const float* ent, const float* bias, hipStream_t s);
int launch_band_setup(coper_handle* h, const float* hvec, const float* tgt, int64_t B, hipStream_t s);
int launch_exact_targets(coper_handle* h, const float* hvec, const int64_t* e2, int64_t B, float* out, hipStream_t s);
int launch_exact_rows(coper_handle* h, const float* hvec, const float* rows, const float* bias, int64_t B, float* out, hipStream_t s);
float band_kappa(const coper_handle* h);
// kernels_tail_bf16.hip: finalize + targets + filter correction of a ranking pass in one launch
bool tail_fused_supported(const coper_handle* h);
// The filter correction of a ranks-only pass of B queries is read from the count kernel's own compare bits (the gt plane,
// kernels_score3_bf16.hip: SC3_GT) instead of being scored a second time by the tail kernel: where the fused tail serves the handle
// and the plane of the pass's longest count launch stays within FILTER_BITS_PLANE_CAP.  The ONE predicate of the path: the
// workspace (ensure_rank_workspace) and every launch of the pass decide by it.
constexpr size_t FILTER_BITS_PLANE_CAP = (size_t)64 << 20;
bool filter_bits_supported(const coper_handle* h, int64_t B);
size_t rank_mask_bytes(const coper_handle* h, int64_t B);     // mask_ws of a ranking pass of B queries: band words, gt plane if any, summaries
int launch_finalize_targets_filter_bf16x3(coper_handle* h, PassCtx& ctx, int64_t B, int ksplit, float* h_out, const int64_t* e2, const int64_t* indptr,
                                          const int64_t* idx, int64_t nnz, float* tgt, int32_t* ranks, hipStream_t s);
int launch_finalize_h_publish(coper_handle* h, int64_t B, int ksplit, float* h_out, hipStream_t s);
int launch_filter_excess_bf16x3(coper_handle* h, PassCtx& ctx, const float* hvec, const int64_t* e2, const int64_t* indptr, const int64_t* idx,
                                int64_t nnz, int64_t B, int32_t* ranks, bool defer, hipStream_t s);
void score_count_begin_f32(coper_handle* h, const float* hvec, int64_t B, int32_t* ng, int32_t* ne, hipStream_t s);
int score_count_chunk_f32(coper_handle* h, int64_t q0, int64_t Bc, const float* tgt, int32_t* ng, int32_t* ne, float* gmax,
                          int64_t gm_stride, hipStream_t s);
int launch_topk_score_blocks_f32(coper_handle* h, const float* hvec, int64_t T, const int64_t* e2, const int64_t* indptr,
                                 const int64_t* idx, hipStream_t s);
int score_count3_maxima_bf16x3(coper_handle* h, int64_t q0, int64_t Bc, int32_t* ng, float* gmax, int64_t gm_stride, hipStream_t s);
// kernels_topk_bf16.hip: the launchers of a plan whose workspaces h->topk (and h->pred) hold (ensure() first)
int launch_topk_pruned_f32(coper_handle* h, const TopkPlan& p, const float* hvec, const float* tgt, const int64_t* e2, const int64_t* indptr,
                           const int64_t* idx, int32_t* ng, int32_t* ne, float* topk_val, int64_t* topk_idx, hipStream_t s);
int launch_topk_pruned_bf16x3(coper_handle* h, PassCtx& ctx, const TopkPlan& p, const float* hvec, const float* tgt_x, const int64_t* e2,
                              const int64_t* indptr, const int64_t* idx, int32_t* ng, int32_t* ne, float* topk_val, int64_t* topk_idx, hipStream_t s);
// coper_predict_topk: blocks emitted beyond the k + (filter entries) that hold the x3 top-k, so that the chain's top-k provably sits in
// emitted blocks; the plan of the x3 predictor has k_blocks = k + PREDICT_SLACK
constexpr int PREDICT_SLACK = 4;
// "no target" for the kernels that exempt one from the filter; a raw call (no CSR given) also gets its empty one
int predict_filter_args(coper_handle* h, int64_t B, bool raw, const int64_t** no_target, const int64_t** indptr, const int64_t** idx, hipStream_t s);
int launch_predict_topk_bf16x3(coper_handle* h, const TopkPlan& p, const float* hvec, const int64_t* no_target, const int64_t* indptr,
                               const int64_t* idx, int k, float* topk_val, int64_t* topk_idx, hipStream_t s);
int predict_stats_read(coper_handle* h, bool reset, uint32_t v[8], hipStream_t s);   // pred_stats into v (untouched before the first x3 call)
// kernels_encode_bf16.hip
bool conv_bf16_supported(const Dims& dm);
int launch_wfrag_to_bf16(coper_handle* h, const float* Wf, int64_t Rw, void* hi, void* lo, int32_t* w_exp, hipStream_t s);
int compute_x_exp(coper_handle* h, unsigned* scratch, hipStream_t s);
// k-steps (of 32) between two feature blocks of the 16-bit dense-weight image Wf16_{hi,lo}: [rel * nfb + fb][stride][64] x 16 B.
// Round 5: ODD (F / 32 | 1: 145 for 144 at FB15k-237 shapes, +0.7 % memory).  The 26 streams of a workgroup and the 237 workgroups
// of a pass are all at the same k-step at the same time; with feature blocks 144 KiB and relations 1,872 KiB apart they all sat at
// the same offset inside every 4-KiB page of the image, i.e. on the same few memory channels.  Measured on the pass (same box,
// three alternating runs): fused encoder 0.1729 -> 0.1687 ms, pass 0.5115 -> 0.5064 ms.
__host__ __device__ inline int64_t w16_ks_stride_n(int64_t ks32n) {
  return ks32n | 1;
}
inline int64_t w16_ks_stride(const Dims& dm) { return w16_ks_stride_n(dm.F_pad / 32); }
int launch_conv_bf16(coper_handle* h, const int64_t* e1, const int64_t* rel, const float* e1_rows, int64_t B, hipStream_t s);
int launch_dense_bf16(coper_handle* h, int64_t B, int nslices, hipStream_t s);
bool dense_fused_supported(const coper_handle* h, int nslices);
int launch_dense_fused_bf16(coper_handle* h, PassCtx& ctx, const int64_t* e1, const int64_t* rel, const float* e1_rows, int64_t B,
                            int nslices, float* h_fin, hipStream_t s);
bool dense_fused_finalizes(const coper_handle* h, int nslices, const float* h_out);
int fused_fin_update(coper_handle* h, hipStream_t s);
// grouping sets (coper_group_next; coper_abi.hip)
void group_home_views(coper_handle* h);             // set 0's views, after the home arrays were (re)allocated
void group_sets_free(coper_handle* h);              // sets 1, 2 (back to home first)
int group_sets_ensure(coper_handle* h, hipStream_t s);
int launch_dense_finalize(coper_handle* h, const int64_t* rel, int64_t B, int ksplit, float* h_out, hipStream_t s);
// kernels_dense_factored_bf16.hip (COPER_DENSE_FACTORED)
int factored_prepare(coper_handle* h, const float* ctx, int Kc, const float* P_last, hipStream_t s);
bool factored_workspace_short(const coper_handle* h, int64_t cap);    // the chunk workspaces do not serve `cap` queries yet
int factored_workspace(coper_handle* h, int64_t cap);
int launch_dense_factored(coper_handle* h, const int64_t* e1, const int64_t* rel, const float* e1_rows, int64_t B, float* h_out, hipStream_t s);
int launch_dense_finalize_pack(coper_handle* h, PassCtx& ctx, int64_t B, int ksplit, float* h_out, hipStream_t s);
int launch_pair_targets_packed_bf16x3(coper_handle* h, PassCtx& ctx, const int64_t* e2, int64_t B, float* tgt, hipStream_t s);
int score_all_dispatch(coper_handle* h, const float* hvec, int64_t B, float* logits, int64_t ld, hipStream_t s);
int launch_bias_pad(coper_handle* h, const float* bias, hipStream_t s);
int launch_topk(coper_handle* h, const float* hvec, const int64_t* e2, const int64_t* indptr, const int64_t* idx,
                int64_t B, int k, float* topk_val, int64_t* topk_idx, float* logits_ws, int64_t chunk_rows,
                hipStream_t s);

// kernels_known.hip: the known-facts index
int launch_known_build(coper_handle* h, const int64_t* e1, const int64_t* rel, const int64_t* ip, const int64_t* ix, int64_t n_keys,
                       int64_t nnz, int64_t* keys, int64_t* ip_out, void* tails, bool wide, unsigned* viol, hipStream_t s);
int launch_known_find_scan(coper_handle* h, const int64_t* e1, const int64_t* rel, int64_t B, int32_t* row, int64_t* filt_indptr,
                           hipStream_t s);
int launch_known_gather(coper_handle* h, const int64_t* filt_indptr, const int32_t* row, int64_t B, int64_t total, int64_t* out,
                        hipStream_t s);

// COPER_DBG_SYNC=1 in the environment: synchronise after the launches that carry this hook and report the first failing one
// (localises a faulting kernel; read once per process)
int dbg_sync(coper_handle* h, hipStream_t s, const char* what);
#define COPER_DBG_SYNC(h, s, what) do { int _d = coper::dbg_sync((h), (s), (what)); if (_d) return _d; } while (0)

// profiling helpers (hipEvents on the launch stream)
struct ScopedKernelTimer {
  coper_handle* h;
  const char* name;
  hipStream_t s;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ScopedKernelTimer(coper_handle* h_, const char* n, hipStream_t s_);
  ~ScopedKernelTimer();
};

}  // namespace coper
