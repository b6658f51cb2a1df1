// Training step (include/coper_hip.h "Training step").  fp32 throughout.
//
//   forward (train mode, models.py:354-426,438-443):
//     c = rel_emb[rel]; generator chains (g_MLP: projection, BN with batch statistics, ReLU, dropout per hidden layer)
//     conv filters: static, generated per sample (c or chain output times the last projection) or looked up
//     img = ent_emb[e1] (+ rel_emb[rel] stacked below it for plain ConvE)            k_tr_conv_fwd
//     y   = conv3x3(img) + bias                             [B, P = Ho*Wo, C]          k_tr_conv_fwd
//     Conv1BN (batch statistics when batch_norm_train_stats), ReLU, dropout -> x [B, F]   k_tr_bn1_fwd
//     concat_rel: x = [x | c]                                                          k_tr_concat / k_tr_split
//     dense: static z0 = x W (one GEMM); generated z[b] = sum_rho ctx[b,rho] (x[b] P[rho]) -- the FACTORED form: r
//            independent [B,F]x[F,d] products (one strided-batched GEMM), the [B,F,d] weight tensor of
//            models.py:70,412 is never formed; g_lookup: one pass over the looked-up [F,d] rows  (k_tr_lookup_*)
//     + dense bias, dropout, FCBN, ReLU -> h [B, d]                                   k_tr_fc_post(_slices), k_tr_fcbn_fwd
//     sampled scorer s[b,l] = h[b] . ent_emb[lookup[b,l]] + pred_bias[...] and the loss: k_tr_score_loss_dh (round 6: with ds and
//     dh = sum_l ds E[lookup] from the same pass over the gathered rows; k_tr_score_loss where d % 4 != 0) or 1-vs-all (GEMM; from sparse labels
//     in chunks of entity columns, forward and backward per chunk: Step::score_csr)
//   backward: the transposes of the above (dense: dP[rho] = x^T (ctx[:,rho] . dz) batched, dA = dz P2^T one GEMM, then
//   the contraction with ctx / x); embedding-row gradients by float atomics or, when B*|E| is small, through a dense
//   d(loss)/d(logits) matrix and one GEMM.  Every GEMM is the split-fp16 MFMA kernel of train_gemm_bf16.hip (no library).
//   optimiser: tf.clip_by_global_norm + AMSGrad (amsgrad.py:130-159), one launch each over all tensors.
//   Schedule (round 6): the scorer's backward and the dP product run on two side streams of the training state, forked from and
//   joined to the caller's stream by events (SideJoin; the forks are where a stage begins, the joins in Step::join_sides at the end of a call); K slices of the few-tile products are added by the
//   kernels that consume them (k_tr_fc_post_slices, k_tr_bn1_bwd_sums<NS>), not by a launch of their own.
//   Deterministic mode (coper_train_config.deterministic): every atomic accumulation above has a second form with one defined
//   order -- per-workgroup partial sums in TrainState::det_slab folded by k_tr_fold_det, one writer per embedding / relation row
//   (k_tr_rows_by_key_det), S rows built in ascending lookup position (k_tr_build_S_det) -- chosen where the launch is made (`det`);
//   the step is one chain on the caller's stream there.  With the mode off every launch is the one it was.
//   Deferred rows (coper_train_defer_rows): the sampled step touches only the rows of ent_emb / pred_bias its batch names --
//   claim, catch up (the closed form of the skipped zero-gradient updates), norm and update over that list, the list before re-zeroed --
//   in phases of their own beside the ones above (Step::rows_*; kernels in train_rows.h); k_tr_zero_list, k_tr_sumsq and k_tr_amsgrad
//   leave the two tables out.  With the mode off every launch is the one it was.  The mode's split step (coper_train_rows_backward |
//   _export | _import | _apply) exchanges a small flat vector and row blocks: k_rows_export / k_rows_import (train_rows.h).
//   Ordered rows (coper_train_order_rows; a switch on a deterministic state): the sampled scorer's table gradient by a stable
//   sort of the batch's ids, their segment heads and one wave per segment (Step::order_rows / bwd_scorer; kernels in train_order.h) at any
//   num_ent; the heads are the deferred-rows mode's row list, in ascending id, and its norm goes through the slab.  Off: nothing changes.
//   Entity-sharded 1-vs-all (coper_train_init_sharded): the handle holds rows [shard_lo, shard_hi) of the two tables with their
//   gradients and slots; the step is four calls -- coper_train_shard_forward | _score_csr or _score_lookup (sampled labels, DESIGN 6.8:
//   the sampled scorer below over the handle's row range) | _backward | _apply -- three ranges of the stage list and the update,
//   with the caller's exchanges between them (input rows, the shards' shares of dh and the loss, their squared norms).  A deterministic
//   state only; kernels of its own in train_shard.h.  Every other entry point behaves as it did.
//   Deferred rows on a shard: coper_train_defer_rows on such a state, between steps; the row state is per LOCAL row.  The
//   four calls branch on the mode in the host code below: the gather returns rows as of the current update (k_shard_gather_current), the
//   forward call re-zeroes the list of the step before, the sampled score call sorts first, takes the owned run of the heads as its list
//   (k_shard_list_owned) and catches it up, the backward call's squared norm and the apply call's table update run over that list.  With
//   the mode off a sharded step launches what it launched.
//   Synchronised batch statistics (coper_train_sync_begin | _next): the backward of a data-parallel rank whose Conv1BN / FCBN
//   statistics span every rank's shard of one batch -- the stage list is cut where a batch-wide sum is needed (behind Bn1Sums, FcbnSums,
//   FcbnBwdSums, Bn1BwdSums: kSyncCuts), five calls with the caller's all-gathers between them, the ranks' shares added in ascending
//   rank (k_tr_fold_parts).  Every other entry point runs the halves back to back, as one launch list.
// This file is the host side: the training state, the GEMM helpers, init / destroy, the step and the small entry points.  The kernels
// are in train_kernels.h.
//   The schedule is written ONCE: enum class Stage lists the stages of a step in execution order -- ConvFilters, Bn1Sums, Bn1, Dense,
//   FcbnSums, Fcbn, Score | ScorerBwd, FcbnBwdSums, FcbnBwd, DenseBwd, ChainsBwd, Bn1BwdSums, Bn1Bwd, ConvBwd, ConvFiltersBwd -- and
//   Step::run(from, to) executes a range of it; nothing else calls a stage.  Every entry point is its preamble (refusals, workspaces,
//   the zero list, the row lists) and ranges: the fused calls [ConvFilters, End) or, forward only, [ConvFilters, ScorerBwd) in
//   train_step_impl; the sharded calls [ConvFilters, Score) | [Score, FcbnBwdSums) | [FcbnBwdSums, End); the synchronised step
//   [ConvFilters, Bn1) and the four rows of kSyncCuts.  A step that stays open between calls is ONE record, TrainState::open (OpenStep:
//   the arguments, the StepCarry, the phase), resumed by open_resume and suspended by `open.carry = st`.
//   What a call is (StepKind) and which route its scorer takes (ScorerPlan: label form, table-gradient route, dh route, the owned row
//   range) are decided ONCE per call -- plan_scorer, and ScorerPlan::resolve_dh behind the workspaces -- and read everywhere else: the
//   refusals, the workspace sizes and the launches cannot disagree.  Every update ends in the same tail: a tensor table from
//   train_tensors, the launches, finish_update for the host's bookkeeping.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "coper_internal.h"
#include "train_common.h"
#include "train_gemm.h"
#include "train_kernels.h"
#include "train_rows.h"
#include "train_order.h"
#include "train_shard.h"

namespace coper {

namespace {

struct TrainParam {
  std::string name;
  float* p = nullptr;   // the caller's variable, updated in place
  int64_t n = 0;
  DevBuf<float> g;      // gradient of the last step
  int64_t flat_off = 0; // where the leaf starts in the flat gradient vector (coper_train_grads_layout)
  int64_t small_off = -1; // ... and in the small flat vector of the deferred-rows split step (coper_train_rows_layout; -1: ent_emb, pred_bias)
  DevBuf<float> m;      // AMSGrad slots
  DevBuf<float> v;
  DevBuf<float> vh;
};

// What the forward stages of a step hand to its backward stages (a base of struct Step).  A step held open between calls keeps it on
// the state (OpenStep, below struct StepArgs): one assignment each way.
struct StepCarry {
  const unsigned* w_slots = nullptr;  // the dense weights' maximum as the last step's optimizer pass left it, when it describes them
  const unsigned* x_slots = nullptr;  // the dense input's, as k_tr_bn1_fwd wrote it
  const float *ccw = nullptr, *ccb = nullptr;   // contexts of the conv generators [B, rc_cw], [B, rc_cb]
  const float *cw = nullptr, *cbv = nullptr;    // contexts of the dense generators [B, rc_w], [B, rc_b]
  const float* xin = nullptr;         // the dense layer's input [B, F] and its gradient
  float* dxin = nullptr;
  const TrainParam* W = nullptr;      // the dense weights: row-major [rc_w * F, d] (generated), [F, d] (static) or the table (looked up)
  bool p3_packed = false;        // the projection's second view (rows f) was packed with its first
  // ordered rows: the sorted entry indices, and the batch's unique rows with their segment offsets (Step::order_rows; null until it ran)
  const int32_t *ord_vals = nullptr, *ord_rows = nullptr, *ord_rows_count = nullptr;
};

// 1-vs-all labels as id lists (include/coper_hip.h, coper_train_step_csr); indptr == nullptr: the dense-label call
struct CsrLabels {
  const int64_t *indptr = nullptr, *idx = nullptr, *row = nullptr;
  int64_t n_rows = 0;
};

// What a call of the step is: coper_train_forward; coper_train_step; coper_train_backward (everything but the optimizer);
// coper_train_rows_backward (the same in the deferred-rows mode)
enum class StepKind { Forward, Step, Backward, RowsBackward };
inline bool differentiates(StepKind k) { return k != StepKind::Forward; }
inline bool runs_optimizer(StepKind k) { return k == StepKind::Step; }
inline bool keeps_moving_stats(StepKind k) { return k == StepKind::Forward; }      // (k_tr_bn_finish leaves the moving statistics alone)

// ---- the scorer's routes, decided once per call
// the dense d(loss)/d(logits) matrix S [B, |E|] fits: 1-vs-all trains through it, the sampled scorer's backward is a GEMM on it
inline bool dense_S_fits(int64_t B, int64_t E) { return (double)B * (double)E * 4.0 <= 512.0 * 1024 * 1024 && E <= 0x7fffffff; }
enum class LabelForm { Dense, Csr, Sampled };      // labels [B, |E|] (or none: a sharded call that scores nothing); id lists; [B, L] with a lookup
// d(ent_emb) / d(pred_bias): one GEMM on the S of 1-vs-all; per chunk of entity columns (Step::score_csr); the dense S built from the
// lookup and one GEMM; sorted segments, one writer per row (ordered rows, a sharded state); float atomics
enum class TableGrad { OvaGemm, CsrChunks, DenseS, Ordered, Atomics };
// dh [B, d]: a GEMM on S (1-vs-all); from the pass that formed the scores (k_tr_score_loss_dh); k_tr_dh_gather4; k_tr_score_bwd
enum class DhRoute { Gemm, Fused, Gather4, ScoreBwd };
struct ScorerPlan {
  LabelForm labels = LabelForm::Dense;
  TableGrad table = TableGrad::OvaGemm;
  DhRoute dh = DhRoute::Gemm;
  size_t lds_fused = 0;         // k_tr_score_loss_dh's dynamic LDS (DhRoute::Fused)
  bool shard = false;           // an entity-sharded state: the tables are rows [lo, lo + n) of num_ent, the sampled kernels
  int64_t lo = 0, n = 0;        //   take their SHARD forms; otherwise [0, num_ent)
  bool current = false;         // (with shard) the forward-only sharded call in the deferred-rows mode: the sampled kernels take
                                //   their CURRENT forms -- every owned row as of the current update in registers, nothing written
  bool sampled() const { return labels == LabelForm::Sampled; }
  bool ordered() const { return table == TableGrad::Ordered; }
  // The part that looks at pointers, once the workspaces exist (ent is the caller's: nothing here follows from an allocator).
  void resolve_dh(int d, int64_t L, const float* ent, const float* dh_ws, const float* hv_ws) {
    if (!sampled()) return;
    dh = DhRoute::ScoreBwd;
    if (table == TableGrad::Atomics) return;      // (k_tr_score_bwd<true>: dh beside its atomics)
    // the gather: 16-byte rows; fused with the scores: a training step whose dE goes through S or the segments takes scores, loss, ds
    // and dh from one pass over the rows (coper_train_forward takes the same kernel: its loss is the step's, bit for bit)
    if (!((d & 3) == 0 && d >= 16 && d <= 1024 && (((uintptr_t)ent | (uintptr_t)dh_ws) & 15) == 0)) return;
    dh = DhRoute::Gather4;
    if (!(L >= 1 && L <= SF_MAX_L && ((uintptr_t)hv_ws & 15) == 0)) return;
    dh = DhRoute::Fused;
    const int d4 = d >> 2, slots = 256 / d4 > 256 / SF_U ? 256 / SF_U : 256 / d4, RB = SF_U * slots;
    // (SHARD: the compacted entries' positions, int [L] more)
    lds_fused = sizeof(float4) * (size_t)slots * d4 + sizeof(float) * (size_t)RB * (d4 + 2) + (shard ? 2 : 1) * sizeof(int) * (size_t)L;
    // (CURRENT: every compacted entry's C and whether it is behind, double [L] and a byte [L] more -- where that passes the 160 KB of a
    //  workgroup the launch is refused by the caller, never served by another route: the route decides the bits)
    if (current) lds_fused += (sizeof(double) + 1) * (size_t)L;
  }
};

// One call of the step: the arguments, and what they and the configuration decide once (struct Step: the stages over them).
struct StepArgs {
  StepKind kind = StepKind::Step;
  hipStream_t s = nullptr;
  const int64_t *e1 = nullptr, *rel = nullptr;
  const int32_t* lookup = nullptr;
  const float* labels = nullptr;
  int64_t B = 0, L = 0;
  float *loss_out = nullptr, *pred_out = nullptr, *h_out = nullptr;
  CsrLabels csr;                    // the sparse-label 1-vs-all step: `labels` is null, the scorer runs in chunks (score_csr)
  const float* img_rows = nullptr;  // the entity-sharded step: the input images are the rows of img_rows [B, d] (the gathered e1 rows), never the table's
  ScorerPlan plan;                  // plan_scorer of the same call; its dh route once grow_workspaces has run
  // synchronised batch statistics: the batch is rows [sample_offset, sample_offset + B) of a batch of B_stat samples that
  // the BN statistics are taken over (0: the batch is its own) -- the dropout masks are drawn by the position in THAT batch
  int64_t B_stat = 0, sample_offset = 0;
};
// A step held open between calls: the synchronised step (coper_train_sync_begin | _next) and the entity-sharded step
// (coper_train_shard_forward | _score_* | _backward | _apply) -- a state runs one or the other.  `args`: the arguments of the
// call that opened it (the begin call's: the caller keeps the batch's buffers as they are until the step is complete or abandoned; the
// sharded forward call's, over the state's own copy of the ids, amended by the score call with its labels).  `carry`: what the stages
// that ran hand to the ones to come.  `phase`: 0 no step open; a synchronised step: 1..4, the exchange the state waits for; a sharded
// state: the call expected next (ShardPhase).  Every later call resumes it (open_resume) and suspends it again (`open.carry = st`).
struct OpenStep {
  StepArgs args;
  StepCarry carry;
  int phase = 0;
};

// the owner of one operand plane set of the split-16 GEMMs; the GEMM helpers take the TgPlanes it hands out
struct PlaneSet {
  DevBuf<uint4> hi, lo;
  int32_t* exp = nullptr;   // view: its word in TrainState::tg_exps
  operator TgPlanes() const { return TgPlanes{hi, lo, exp}; }
};

// What the step reads and writes: the handle's leaves (coper::Leaves, h->lv) as the step sees them, resolved ONCE (resolve_leaves: at
// coper_train_init and behind every coper_set_param).  Trainable leaves by their TrainParam, BN moving statistics by where they are
// registered now.
struct TrainLeaves {
  TrainParam *ent_emb = nullptr, *rel_emb = nullptr /* none under g_lookup */, *pred_bias = nullptr;
  TrainParam *conv1_weights = nullptr, *conv1_bias = nullptr;   // static filters or g_lookup tables (none where they are generated)
  TrainParam *fc_weights = nullptr, *fc_bias = nullptr;         // static dense layer or g_lookup tables (none where it is generated)
  struct Bn { TrainParam *gamma = nullptr, *beta = nullptr; float *mov_mean = nullptr, *mov_var = nullptr; } bn1, fcbn;   // Conv1BN, FCBN
  struct Gen {              // generator chain g: proj[0 .. nh], the last one multiplies the context; bn[i] behind proj[i], i < nh
    TrainParam* proj[COPER_MAX_CTX + 1] = {};
    Bn bn[COPER_MAX_CTX];
  } gen[4];                 // GenId
};

// The one description of TrainState::red, the step's reduction scratch in double (zeroed whole by the step's zero list): [0] loss,
// [1] squared global gradient norm (written by the optimizer kernel), TR_COLSUM_SLICES slices of 2 mx column sums (sum | sum of squares),
// TG_SUMSQ_SLOTS partial sums of the squared gradient norm, then two slices in TR_CS_SLOTS copies each (CsSlots).  mx: the widest BN layer.
struct RedLayout {
  double* base;
  size_t mx;
  size_t slice_at(int i) const { return 2 + (size_t)i * 2 * mx; }
  size_t slots_at(int j) const { return slice_at(TR_COLSUM_SLICES) + TG_SUMSQ_SLOTS + (size_t)j * TR_CS_SLOTS * 2 * mx; }
  size_t doubles() const { return slots_at(2); }
  double* loss() const { return base; }
  double* total_sumsq() const { return base + 1; }
  double* colsum_slice(int i) const { return base + slice_at(i); }      // i: ColsumSlice / cs_chain(g, i)
  double* sumsq_slots() const { return base + slice_at(TR_COLSUM_SLICES); }
  double* cs_slots(int j) const { return base + slots_at(j); }          // j: CsSlots
};
// the rows of TrainState::bnst, mx floats each: mean and 1 / std of Conv1BN and FCBN as the forward pass used them
enum BnRow { BN1_MEAN, BN1_INV, FCBN_MEAN, FCBN_INV, BN_ROWS };

}  // namespace

struct TrainState {
  coper_train_config cfg;
  std::vector<TrainParam> tp;
  double b1p = 0, b2p = 0;
  uint32_t step = 0;
  int64_t capB = 0, capL = 0;  // the batch and lookup sizes the workspaces hold (0 while any of them is missing)
  // workspaces
  DevBuf<float> img, y, x, c;
  DevBuf<float> xc, dxc;       // concat_rel: [B, F_conv + r] input of the dense layer and its gradient
  // g_MLP generator chains (models.py:56-70), one for fc_weights (0) and one for fc_bias (1):
  //   v[0] = c;  u[i] = v[i] P_i;  a[i] = relu(BN_i(u[i]));  v[i+1] = dropout(a[i]);  context = v[nh]
  struct Chain {
    int dims[COPER_MAX_CTX + 1];
    DevBuf<float> v[COPER_MAX_CTX + 1];  // v[1..]; v[0] is TrainState::c (left empty here)
    DevBuf<float> u[COPER_MAX_CTX];
    DevBuf<float> a[COPER_MAX_CTX];
    DevBuf<float> dv[COPER_MAX_CTX + 1]; // gradient w.r.t. v[i]
    DevBuf<float> du[COPER_MAX_CTX];
    DevBuf<float> st[COPER_MAX_CTX];     // [2][n]: mean | inv_std
  } chain[4];                 // 0 fc_weights, 1 fc_bias, 2 conv1_weights, 3 conv1_bias
  int nh = 0;                 // hidden layers of the dense-layer generators
  int nhc = 0;                // hidden layers of the conv generators
  DevBuf<float> Kt, Kbv, dKs, dkbs;   // per-sample conv filters / biases and their gradients
  DevBuf<float> Sd;          // [B, |E|] dense d(loss)/d(logits) when it fits (scorer backward by GEMM)
  DevBuf<float> A;           // generated dense: T[r][B][d] (forward partials) | dT[r][B][d]
  // generated dense, split-bf16 GEMMs (train_gemm_bf16.hip): operand planes
  PlaneSet pX, pXt, pP1, pP3, pTn, pTb;   // x rows b | x rows f | P rows (rho,k) | P rows f | dT rows (rho,k) | dT rows b
  // the other products (static dense layer, 1-vs-all scorer, dE of the dense scorer backward): two operand plane sets and
  // the split-K partial sums, grown on demand
  PlaneSet mmX, mmY;
  DevBuf<int32_t> tg_exps;       // [10 + TR_EXP_CACHE] the exponents of the ten plane sets (train_gemm.h), in the order pX pXt pP1 pP3 pTn pTb mmX mmY mmX2 mmY2,
                                 //   then the words tg_matmul hands out per operand tensor within a step (exp_cache)
  // the largest |W| of the dense weights (the last projection of the fc_weights generator / the static fc_weights), as the OPTIMIZER
  // left it: k_tr_amsgrad folds |p_new| of that leaf into TG_MAX_SLOTS slots while it writes it, the packs of the next step reduce
  // the slots -- the 118 MB pass that used to find the maximum (53 us of a 1.25 ms step) is gone.  Two sets: a step reads [wmax_cur],
  // its optimizer pass writes [wmax_cur ^ 1] (zeroed by the step's zero list).  Valid only from one train step to the next of this
  // handle with no coper_set_param in between (the tensors are the caller's: include/coper_hip.h, coper_train_step)
  DevBuf<unsigned> xmax;         // TG_MAX_SLOTS: max x as k_tr_bn1_fwd wrote it;  dtmax: max |dT| as k_tr_scale_rows wrote it (zeroed per step)
  DevBuf<unsigned> dtmax;
  DevBuf<unsigned> smax;         // TG_MAX_SLOTS: max |S| as k_tr_build_S wrote it
  DevBuf<unsigned> wmax[2];
  int wmax_cur = 0;
  bool wmax_valid = false;
  // looked-up dense table: the relation counts of the last step's batch (R + 1), copied out of the grouping workspace behind the
  // step's grouping -- coper_train_grad hands out the rows of absent relations as zeros by them, whatever has been grouped since
  DevBuf<int32_t> step_rel_count;
  DevBuf<int32_t> all_rel_count;    // R + 1 ones: every row present (coper_train_apply from a flat vector)
  // the split step (coper_train_backward / _grads_export / _apply): the flat gradient vector's length, and whether the gradient
  // buffers hold a backward pass that no update has consumed and nothing has zeroed since
  int64_t flat_total = 0;
  bool pending = false;
  // tg_matmul: the exponent of an operand tensor packed earlier in THIS step (x, the static W, dz and S are each packed for two
  // products): (tensor, its word).  Cleared at the start of a step and where a kernel rewrites a tensor in place.
  std::vector<std::pair<const float*, int32_t*>> exp_cache;
  DevBuf<unsigned> tg_scratch;      // [2] the absmax reduction of tg_pack (zero between packs); [2..3]: the side stream's
  // round 6: a step is not one chain -- the projection's packs do not need the conv, the scorer's backward does not need the dense
  // layer's.  Those stretches run on a side stream of the state's own, forked from and joined to the caller's stream by events
  // (under capture they become branches of the graph).  side[0]: the packs in front, the scorer's backward; side[1]: the dP product.
  hipStream_t side[2] = {nullptr, nullptr};
  hipEvent_t ev_fork[3] = {nullptr, nullptr, nullptr}, ev_join[3] = {nullptr, nullptr, nullptr};
  PlaneSet mmX2, mmY2;               // tg_matmul's operand planes on the side stream (TrainState::side[0])
  DevBuf<float> mmP;
  DevBuf<float> z0, z1, hv, dh, dz, ds, dx, dc;
  DevBuf<float> dhc;         // [B, d] a later chunk's share of dh (the 1-vs-all step from sparse labels, Step::score_csr)
  DevBuf<double> red;        // the reduction scratch in double (RedLayout)
  // deterministic mode (coper_train_config.deterministic): no side streams; every reducing launch stores per-workgroup
  // partial sums in det_slab (one use at a time, in stream order; sized by Step::grow_workspaces from the problem shape) and a fold
  // launch adds them; the conv backward leaves d(img) per query in dimg [B, in_h in_w]; det_perm: the relation groups in ascending sample order
  bool det = false;
  DevBuf<double> det_slab;
  DevBuf<float> dimg;
  DevBuf<int32_t> det_perm;
  DevBuf<float> bnst;        // [BN_ROWS][mx]: Conv1BN's and FCBN's statistics of the forward pass (BnRow)
  int mx = 0;                // the widest BN layer: both are sized by it
  RedLayout red_layout() const { return RedLayout{red, (size_t)mx}; }
  float* bn_row(BnRow k) const { return bnst + (size_t)k * mx; }
  TrainLeaves lv;            // where the variables are (resolve_leaves)
  // deferred rows (coper_train_defer_rows; kernels in train_rows.h).  rows_word[e]: row e of ent_emb / pred_bias and their
  // slots is current as of update number rows_word[e] of rows_now (updates since the mode was enabled); rows_claim: a bit per row, set
  // while the row is on a list; rows_list[rows_prev]: the rows of the call before (their gradient rows are the only non-zero ones of
  // the two buffers, their claim bits the only ones set), rows_list[rows_prev ^ 1]: free for the next call; rows_count: their lengths
  bool rows_deferred = false;
  int32_t rows_now = 0;
  double rows_l2b1p = 0, rows_l2b2p = 0;   // log2 of b1p / b2p, advanced by addition: a catch-up divides the powers by beta^gap (train_rows.h, RowCatchUp)
  int rows_prev = 0;
  int64_t rows_cap = 0;
  DevBuf<int32_t> rows_word, rows_list[2], rows_count;
  DevBuf<unsigned> rows_claim;
  DevBuf<unsigned long long> rows_stats;
  // the step in calls in the mode (coper_train_rows_*).  small_total: the small flat vector's length.  rows_pending_small:
  // the gradient buffers of every leaf but the two tables hold a coper_train_rows_backward that nothing has consumed or zeroed;
  // rows_pending_table: rows_list[rows_prev] and the listed rows of d(ent_emb) / d(pred_bias) hold such a backward, or the imports since
  // the last `first`; rows_bound: what the host knows about that list's length (min(B (L + 1), E); min(E, entries imported))
  int64_t small_total = 0;
  bool rows_pending_small = false, rows_pending_table = false;
  int64_t rows_bound = 0;
  void rows_pending_clear() { rows_pending_small = rows_pending_table = false; rows_bound = 0; }
  // ordered rows (coper_train_order_rows; kernels in train_order.h): the sort's ping-pong buffers ord_key / ord_val and the
  // segment offsets ord_seg hold ord_cap = B (L + 1) entries (+ 1), ord_hist 256 words per sort tile (+ the tiles' head counts behind
  // them), ord_scan their exclusive scan; ord_list / ord_count: the unique rows of a step with deferred rows off (with it on they are rows_list / rows_count).
  // rows_list_unsorted: imports appended to the pending list since it was last in ascending id (sorted before the norm and an export).
  bool rows_ordered = false;
  int64_t ord_cap = 0;
  DevBuf<int32_t> ord_key[2], ord_val[2], ord_seg, ord_hist, ord_scan, ord_list, ord_count;
  bool rows_list_unsorted = false;
  // entity-sharded 1-vs-all (coper_train_init_sharded).  sh_e1 / sh_rel: the batch's ids as the forward call saw them (the
  // open step's arguments name them: the later calls have no id arguments); sh_iota: 0 .. B - 1, the row numbers of the gathered input
  // rows.  Deferred rows on a shard: the row state above is per LOCAL row.
  bool sharded = false;
  int64_t sh_cap = 0;
  bool sh_stepped = false;     // a sharded step has begun on this state: the deferred-rows mode is no longer ENABLED on it (it is chosen before the first step)
  DevBuf<int64_t> sh_e1, sh_rel, sh_iota;
  // the step held open between calls: a synchronised step, or on a sharded state the step of the four calls (OpenStep)
  OpenStep open;
  int sync_phase() const { return sharded ? 0 : open.phase; }      // the exchange an open synchronised step waits for (0: none is open)
  // synchronised batch statistics (coper_train_sync_*): [2][2 mx] doubles -- the backward sums of the whole batch as the
  // last fold left them | this rank's FCBN backward sums (Conv1BN's own stay in their slice of `red`)
  DevBuf<double> sync_sums;
  TrainParam* find(const char* name) {
    for (auto& t : tp)
      if (t.name == name) return &t;
    return nullptr;
  }
};

namespace {

// GEMM on planes packed by the caller, K cut into slices when the output has few tiles (the partial-sum pool grows on demand)
// slices_left: when not null and K was cut, the partial sums stay in T->mmP ([*slices_left][M][N]) for the caller's next kernel and C is
// not written (*slices_left = 1: C holds the product)
static int tg_gemm_split(coper_handle* h, TrainState* T, hipStream_t s, TgPlanes X, int64_t M, TgPlanes Y, int64_t N, int64_t K, float* C,
                         TgIdx ci, TgIdx cj, int* slices_left = nullptr) {
  int rc;
  const int nsplit = tg_split_k(M, N, K);
  if (slices_left) *slices_left = nsplit > 1 && nsplit <= 8 ? nsplit : 1;
  const size_t np = nsplit > 1 ? (size_t)nsplit * M * N : 0;
  if (np > T->mmP.size()) {
    COPER_HIP_TRY(h, hipStreamSynchronize(s));
    if ((rc = T->mmP.alloc(h, np, "split-K partial sums"))) return rc;
  }
  return tg_gemm_nt(h, X, M, Y, N, K, C, ci, cj, s, nsplit, T->mmP, nullptr, slices_left && *slices_left > 1);
}

// C(i, j) = sum_k X(i, k) Y(j, k) for two strided fp32 views, on the split-bf16 GEMM of train_gemm_bf16.hip: packs both
// operands into the state's plane sets (grown on demand), cuts K into slices when the output has few tiles.
struct MmView {
  const float* p;
  TgIdx ri, ki;
  bool rows_fast;   // consecutive rows contiguous in memory (else consecutive k)
};
static int tg_matmul(coper_handle* h, TrainState* T, hipStream_t s, const MmView& X, int64_t M, const MmView& Y, int64_t N, int64_t K,
                     float* C, TgIdx ci, TgIdx cj, double* sumsq = nullptr, const unsigned* x_slots = nullptr, const unsigned* y_slots = nullptr) {
  int rc;
  const size_t nx = tg_plane_elems(M, K), ny = tg_plane_elems(N, K);
  const int nsplit = tg_split_k(M, N, K);
  const size_t np = nsplit > 1 ? (size_t)nsplit * M * N : 0;
  const bool on_side = T->side[0] && s == T->side[0];      // (the caller made sure that no K slices are needed there: one partial-sum pool)
  PlaneSet& MX = on_side ? T->mmX2 : T->mmX;
  PlaneSet& MY = on_side ? T->mmY2 : T->mmY;
  if (on_side && nsplit > 1) return fail(h, COPER_ESTATE, "tg_matmul: a product with K slices on the side stream");
  if (nx > MX.hi.size() || nx > MX.lo.size() || ny > MY.hi.size() || ny > MY.lo.size() || np > T->mmP.size()) {
    COPER_HIP_TRY(h, hipStreamSynchronize(s));
    if ((rc = MX.hi.ensure(h, nx, "GEMM operand planes")) || (rc = MX.lo.ensure(h, nx, "GEMM operand planes")) ||
        (rc = MY.hi.ensure(h, ny, "GEMM operand planes")) || (rc = MY.lo.ensure(h, ny, "GEMM operand planes")) ||
        (rc = T->mmP.ensure(h, np, "split-K partial sums")))
      return rc;
  }
  // an operand tensor packed earlier in this step keeps its power of two (its own word from the pool behind the plane sets' eight):
  // no second pass for the maximum.  A tensor with producer-side maxima (slots) needs no pass at all.
  TgPlanes px = MX, py = MY;
  unsigned* const scratch = on_side ? T->tg_scratch + 2 : T->tg_scratch;
  auto pack = [&](const MmView& V, int64_t rows, TgPlanes& pl, const unsigned* slots) -> int {
    const int32_t* from = nullptr;
    for (auto& e : T->exp_cache)
      if (e.first == V.p) from = e.second;
    if (from) {
      pl.exp = const_cast<int32_t*>(from);
      return tg_pack(h, V.p, V.ri, V.ki, rows, K, tg_rows_pad(rows), V.rows_fast, pl, s, scratch, from);
    }
    if ((int)T->exp_cache.size() < TR_EXP_CACHE) {
      pl.exp = T->tg_exps + 10 + T->exp_cache.size();
      T->exp_cache.emplace_back(V.p, pl.exp);
    }
    return tg_pack(h, V.p, V.ri, V.ki, rows, K, tg_rows_pad(rows), V.rows_fast, pl, s, scratch, nullptr, slots);
  };
  if ((rc = pack(X, M, px, x_slots)) || (rc = pack(Y, N, py, y_slots))) return rc;
  return tg_gemm_nt(h, px, M, py, N, K, C, ci, cj, s, nsplit, T->mmP, sumsq);
}

// Fills TrainState::lv from the handle's leaves (h->lv, which spells the names): the only place that asks where a variable lives.
// `create` (coper_train_init): the trainable leaves become the TrainParams of T->tp (the optimizer's tensor table follows their order:
// the order of the calls here); otherwise each is found again.
static int resolve_leaves(coper_handle* h, TrainState* T, bool create) {
  const Leaves& hl = h->lv;
  TrainLeaves& lv = T->lv;
  lv = TrainLeaves();
  int rc = COPER_OK;
  // where a registered BN moving statistic lives now
  auto stat = [&](const Leaf* lf) -> float* {
    if (lf && lf->set) return const_cast<float*>(lf->ptr);
    if (!rc) rc = fail(h, COPER_EINVAL, "coper_train: missing parameter " + (lf ? lf->name : std::string("(not of this configuration)")));
    return nullptr;
  };
  // a trainable leaf: its TrainParam (created at init), pointed at where the variable lives now
  auto leaf = [&](const Leaf* lf) -> TrainParam* {
    float* const p = stat(lf);
    if (!p) return nullptr;
    TrainParam* t = T->find(lf->name.c_str());
    if (!t && create && (int)T->tp.size() < TR_MAX_PARAMS) {      // (T->tp is reserved: the TrainParams handed out stay where they are)
      T->tp.emplace_back();
      t = &T->tp.back();
      t->name = lf->name;
      t->n = 1;
      for (int64_t s : lf->shape) t->n *= s;
    }
    if (t) t->p = p;
    else if (!rc) rc = create ? fail(h, COPER_EUNSUPPORTED, "coper_train_init: too many trainable tensors")
                              : fail(h, COPER_EINVAL, "coper_train: not a trainable leaf: " + lf->name);
    return t;
  };
  auto bn = [&](const Leaves::Bn& b) {
    TrainParam *const gamma = leaf(b.gamma), *const beta = leaf(b.beta);
    return TrainLeaves::Bn{gamma, beta, stat(b.moving_mean), stat(b.moving_variance)};
  };
  auto chain = [&](int g) {
    const Leaves::Gen& hg = hl.gen[g];
    for (int i = 0; i <= hg.n_hidden; ++i) {
      lv.gen[g].proj[i] = leaf(hg.proj[i]);
      if (i < hg.n_hidden && h->dm.ctx_bn) lv.gen[g].bn[i] = bn(hg.bn[i]);
    }
  };
  lv.ent_emb = leaf(hl.ent_emb);
  lv.pred_bias = leaf(hl.pred_bias);
  lv.bn1 = bn(hl.Conv1BN);
  lv.fcbn = bn(hl.FCBN);
  if (hl.rel_emb) lv.rel_emb = leaf(hl.rel_emb);      // g_lookup has no relation embedding (models.py:210)
  if (hl.conv1_weights) {
    lv.conv1_weights = leaf(hl.conv1_weights);   // static [3,3,1,C], or the [R, 9C] table of g_lookup
    lv.conv1_bias = leaf(hl.conv1_bias);
  } else {
    for (int g : {GEN_CONV1_WEIGHTS, GEN_CONV1_BIAS}) chain(g);
  }
  if (hl.fc_weights) {
    lv.fc_weights = leaf(hl.fc_weights);   // static [F, d], or the [R, F*d] table of g_lookup
    lv.fc_bias = leaf(hl.fc_bias);         // [d], or the [R, d] table
  } else {
    for (int g : {GEN_FC_WEIGHTS, GEN_FC_BIAS}) chain(g);
  }
  return rc;
}

}  // namespace

// coper_set_param: whatever the optimizer's last pass knew about the parameters (TrainState::wmax) no longer describes them, and a
// variable may now live at another address (a checkpoint loaded between steps): the variables are the registered tensors
// (a BN moving statistic is no trainable leaf and says nothing about the dense weights: registering one again -- a data-parallel
// trainer writes the ranks' average into it between steps -- leaves the carried maximum alone)
int train_params_changed(coper_handle* h, const char* leaf_name) {
  TrainState* T = (TrainState*)h->train;
  if (!T) return COPER_OK;
  if (!leaf_name || T->find(leaf_name)) T->wmax_valid = false;
  return resolve_leaves(h, T, false);
}

void train_destroy(coper_handle* h) {
  TrainState* T = (TrainState*)h->train;
  if (!T) return;
  for (hipStream_t& st : T->side)
    if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); st = nullptr; }
  for (int i = 0; i < 3; ++i) {
    if (T->ev_fork[i]) (void)hipEventDestroy(T->ev_fork[i]);
    if (T->ev_join[i]) (void)hipEventDestroy(T->ev_join[i]);
  }
  delete T;
  h->train = nullptr;
}

}  // namespace coper

using namespace coper;

// coper_train_init, and coper_train_init_sharded (`sharded`: any [shard_lo, shard_hi); the leaves ent_emb / pred_bias are the handle's own
// rows, so their gradients and slots below are too)
static int train_init_impl(coper_handle* h, const coper_train_config* cfg, const bool sharded) {
  if (!h || !cfg) return COPER_EINVAL;
  if (cfg->abi_version != COPER_ABI_VERSION) return fail(h, COPER_EINVAL, "coper_train_init: ABI version mismatch");
  if (h->cfg.role != COPER_ROLE_BOTH) return fail(h, COPER_ESTATE, "coper_train_init: training needs a COPER_ROLE_BOTH handle");
  const Dims& dm = h->dm;
  if (!sharded && (h->cfg.shard_lo != 0 || h->cfg.shard_hi != dm.E))
    return fail(h, COPER_EUNSUPPORTED, "coper_train_init: training needs the whole entity table on the handle");
  if (sharded && cfg->deterministic != 1)
    return fail(h, COPER_EUNSUPPORTED, "coper_train_init_sharded: needs deterministic = 1 (the replicated encoders stay equal only because the mode makes "
                                       "every small-leaf gradient a function of its inputs; the default mode would need an all-reduce of them)");
  if (dm.C > 256)
    return fail(h, COPER_EUNSUPPORTED, "coper_train_init: at most 256 conv channels");
  if (!(cfg->learning_rate > 0) || cfg->hidden_dropout < 0 || cfg->hidden_dropout >= 1 || cfg->output_dropout < 0 ||
      cfg->output_dropout >= 1)
    return fail(h, COPER_EINVAL, "coper_train_init: bad hyper-parameter");
  if (cfg->one_vs_all_chunk < 0) return fail(h, COPER_EINVAL, "coper_train_init: one_vs_all_chunk is negative");
  if (cfg->deterministic != 0 && cfg->deterministic != 1) return fail(h, COPER_EINVAL, "coper_train_init: deterministic is 0 or 1");
  for (const Leaf& lf : h->leaves)
    if (!lf.set) return fail(h, COPER_EINVAL, "coper_train_init: parameter not set: " + lf.name);
  COPER_HIP_TRY(h, hipSetDevice(h->cfg.device));
  train_destroy(h);
  TrainState* T = new TrainState();
  h->train = T;
  T->cfg = *cfg;
  T->det = cfg->deterministic == 1;
  T->sharded = sharded;
  T->b1p = cfg->beta1;   // the beta powers start at beta (amsgrad.py:108-113)
  T->b2p = cfg->beta2;
  T->nh = (dm.gen_fc && !dm.lookup) ? h->cfg.n_ctx_out : 0;
  T->nhc = (dm.gen_conv && !dm.lookup) ? h->cfg.n_ctx_conv : 0;
  for (int g = 0; g < 4; ++g) {
    const int nhx = g < 2 ? T->nh : T->nhc;
    T->chain[g].dims[0] = dm.r;
    for (int i = 0; i < nhx; ++i) T->chain[g].dims[i + 1] = g < 2 ? h->cfg.ctx_out[i] : h->cfg.ctx_conv[i];
  }
  T->tp.reserve(TR_MAX_PARAMS);
  int rc;
  if ((rc = resolve_leaves(h, T, true))) return rc;
  for (TrainParam& tp : T->tp) {
    if ((rc = tp.g.alloc(h, (size_t)tp.n, "gradient")) || (rc = tp.m.alloc(h, (size_t)tp.n, "AMSGrad slot")) ||
        (rc = tp.v.alloc(h, (size_t)tp.n, "AMSGrad slot")) || (rc = tp.vh.alloc(h, (size_t)tp.n, "AMSGrad slot")))
      return rc;
    COPER_HIP_TRY(h, hipMemset(tp.m, 0, sizeof(float) * tp.n));
    COPER_HIP_TRY(h, hipMemset(tp.v, 0, sizeof(float) * tp.n));
    COPER_HIP_TRY(h, hipMemset(tp.vh, 0, sizeof(float) * tp.n));
    COPER_HIP_TRY(h, hipMemset(tp.g, 0, sizeof(float) * tp.n));
  }
  // the flat gradient vector: the trainable leaves in coper_param_spec order, each at a multiple of 64 floats
  for (const Leaf& lf : h->leaves)
    if (TrainParam* t = T->find(lf.name.c_str())) {
      t->flat_off = T->flat_total;
      T->flat_total += (t->n + 63) / 64 * 64;
      if (t != T->lv.ent_emb && t != T->lv.pred_bias) {      // the small flat vector: the same rules without the two tables
        t->small_off = T->small_total;
        T->small_total += (t->n + 63) / 64 * 64;
      }
    }
  T->mx = dm.C > dm.d ? dm.C : dm.d;
  for (int i = 0; i < T->nh; ++i) T->mx = h->cfg.ctx_out[i] > T->mx ? h->cfg.ctx_out[i] : T->mx;
  for (int i = 0; i < T->nhc; ++i) T->mx = h->cfg.ctx_conv[i] > T->mx ? h->cfg.ctx_conv[i] : T->mx;
  if ((rc = T->bnst.alloc(h, (size_t)BN_ROWS * T->mx, "BN statistics")) || (rc = T->red.alloc(h, T->red_layout().doubles(), "reductions")) ||
      (rc = T->tg_exps.alloc(h, (size_t)(10 + TR_EXP_CACHE), "plane exponents")) || (rc = T->tg_scratch.alloc(h, 4, "pack scratch")) ||
      (rc = T->wmax[0].alloc(h, TG_MAX_SLOTS, "max slots")) || (rc = T->wmax[1].alloc(h, TG_MAX_SLOTS, "max slots")) ||
      (rc = T->xmax.alloc(h, TG_MAX_SLOTS, "max slots")) || (rc = T->dtmax.alloc(h, TG_MAX_SLOTS, "max slots")) ||
      (rc = T->smax.alloc(h, TG_MAX_SLOTS, "max slots")) ||
      (dm.lookup && dm.gen_fc && ((rc = T->step_rel_count.alloc(h, (size_t)dm.R + 1, "relation counts")) ||
                                  (rc = T->all_rel_count.alloc(h, (size_t)dm.R + 1, "relation counts")))))
    return rc;
  COPER_HIP_TRY(h, hipMemset(T->tg_exps, 0, (10 + TR_EXP_CACHE) * sizeof(int32_t)));
  COPER_HIP_TRY(h, hipMemset(T->wmax[0], 0, TG_MAX_SLOTS * sizeof(unsigned)));
  COPER_HIP_TRY(h, hipMemset(T->wmax[1], 0, TG_MAX_SLOTS * sizeof(unsigned)));
  COPER_HIP_TRY(h, hipMemset(T->tg_scratch, 0, 4 * sizeof(unsigned)));
  if (T->step_rel_count) COPER_HIP_TRY(h, hipMemset(T->step_rel_count, 0, T->step_rel_count.size() * sizeof(int32_t)));
  if (T->all_rel_count) {
    const std::vector<int32_t> ones((size_t)dm.R + 1, 1);
    COPER_HIP_TRY(h, hipMemcpy(T->all_rel_count, ones.data(), ones.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  PlaneSet* sets[10] = {&T->pX, &T->pXt, &T->pP1, &T->pP3, &T->pTn, &T->pTb, &T->mmX, &T->mmY, &T->mmX2, &T->mmY2};
  for (int i = 0; i < 10; ++i) sets[i]->exp = T->tg_exps + i;
  static const bool one_stream = getenv("COPER_TRAIN_ONE_STREAM") != nullptr;   // A/B switch: the step as one chain
  if (!one_stream && !T->det) {      // (deterministic mode: one chain, one slab in use at a time)
    for (hipStream_t& st : T->side) COPER_HIP_TRY(h, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (int i = 0; i < 3; ++i) {
      COPER_HIP_TRY(h, hipEventCreateWithFlags(&T->ev_fork[i], hipEventDisableTiming));
      COPER_HIP_TRY(h, hipEventCreateWithFlags(&T->ev_join[i], hipEventDisableTiming));
    }
  }
  return COPER_OK;
}

extern "C" {

COPER_API int coper_train_init(coper_handle* h, const coper_train_config* cfg) { return train_init_impl(h, cfg, false); }

COPER_API int coper_train_init_sharded(coper_handle* h, const coper_train_config* cfg) { return train_init_impl(h, cfg, true); }

}  // extern "C"

namespace {

inline dim3 grid1d(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// the entity-sharded step's state machine (OpenStep::phase on a sharded state): the call expected next
enum ShardPhase { SHP_FORWARD = 0, SHP_SCORE = 1, SHP_BACKWARD = 2, SHP_APPLY = 3 };
const char* const kShardCall[4] = {"coper_train_shard_forward", "coper_train_shard_score_csr or coper_train_shard_score_lookup",
                                   "coper_train_shard_backward", "coper_train_shard_apply"};

constexpr int64_t TR_OVA_GRAIN = 128;                            // a chunk of entity columns is rows of a GEMM operand plane: TG_ROW_PAD
constexpr int64_t TR_OVA_WS_BYTES = 256LL * 1024 * 1024;         // the [B, chunk] logits of the library's own choice (as coper_rank_counts')
// entity columns per chunk of the sparse-label step: the request rounded up to the grain, or the widest multiple of it within the bound
inline int64_t ova_chunk(int64_t B, int64_t E, int32_t request) {
  int64_t c = request > 0 ? (request + TR_OVA_GRAIN - 1) / TR_OVA_GRAIN * TR_OVA_GRAIN : TR_OVA_WS_BYTES / 4 / B / TR_OVA_GRAIN * TR_OVA_GRAIN;
  if (c < TR_OVA_GRAIN) c = TR_OVA_GRAIN;
  return c < E ? c : E;
}

// The plan of a call's scorer (ScorerPlan, above the training state)
// (deferred rows: the atomic route at every |E| -- the GEMM writes all of dE;  ordered rows: the sorted-segment route at every |E| --
//  one arithmetic for every table size;  a sharded state's sampled score call, DESIGN 6.8: always that route)
static ScorerPlan plan_scorer(const coper_handle* h, const TrainState* T, const int32_t* lookup, const CsrLabels& csr, int64_t B) {
  ScorerPlan p;
  p.shard = T->sharded;
  p.lo = p.shard ? (int64_t)h->cfg.shard_lo : 0;
  p.n = p.shard ? (int64_t)h->dm.n_local : (int64_t)h->dm.E;
  if (csr.indptr) { p.labels = LabelForm::Csr; p.table = TableGrad::CsrChunks; }
  else if (lookup) {
    p.labels = LabelForm::Sampled;
    p.table = (T->rows_ordered || p.shard) ? TableGrad::Ordered
            : (!T->rows_deferred && dense_S_fits(B, h->dm.E)) ? TableGrad::DenseS : TableGrad::Atomics;
  }
  return p;
}

// the side streams (TrainState::side): fork(i, k) lets side[k] start behind everything queued on s so far, join(i) lets s go on
// behind what side[k] was given since.  Whatever leaves the step early joins what it forked.
struct SideJoin {
  TrainState* T; hipStream_t s; int on[3] = {-1, -1, -1};
  hipError_t err = hipSuccess;      // the first failure of an event call (checked where the step ends)
  void note(hipError_t e) { if (e != hipSuccess && err == hipSuccess) err = e; }
  void fork(int i, int k) {
    note(hipEventRecord(T->ev_fork[i], s));
    note(hipStreamWaitEvent(T->side[k], T->ev_fork[i], 0));
    on[i] = k;
  }
  void join(int i) {
    if (on[i] < 0) return;
    note(hipEventRecord(T->ev_join[i], T->side[on[i]]));
    note(hipStreamWaitEvent(s, T->ev_join[i], 0));
    on[i] = -1;
  }
  ~SideJoin() { for (int i = 0; i < 3; ++i) join(i); }
};

// ---- deferred rows: what the row kernels take (train_rows.h)
// the rows of ent_emb / pred_bias the state holds: num_ent, or the shard's own (the mode's state is per LOCAL row there)
inline int64_t rows_held(const coper_handle* h, const TrainState* T) { return T->sharded ? (int64_t)h->dm.n_local : (int64_t)h->dm.E; }
static RowTables row_tables(const coper_handle* h, const TrainState* T) {
  const TrainParam &e = *T->lv.ent_emb, &b = *T->lv.pred_bias;
  RowTables t;
  t.p = e.p; t.g = e.g; t.m = e.m; t.v = e.v; t.vh = e.vh;
  t.bp = b.p; t.bg = b.g; t.bm = b.m; t.bv = b.v; t.bvh = b.vh;
  t.word = T->rows_word;
  t.E = rows_held(h, T);
  t.d = h->dm.d;
  t.vec = (h->dm.d & 3) == 0 && ((((uintptr_t)t.p) | ((uintptr_t)t.g) | ((uintptr_t)t.m) | ((uintptr_t)t.v) | ((uintptr_t)t.vh)) & 15) == 0;
  return t;
}
// terms of C = sum_j lr(.) beta1^j worth keeping: lr(t) <= lr / (1 - beta1) and the first term is >= lr beta1 sqrt(1 - beta2) -- so
// everything beyond j, at most lr beta1^j / (1 - beta1)^2, is below 2^-53 of the sum once beta1^(j-1) < 2^-53 (1 - beta1)^2 sqrt(1 - beta2)
static int32_t rows_jmax(double b1, double b2) {
  if (!(b1 > 0.0) || !(b1 < 1.0)) return 1;      // (beta1 = 0: every term is 0)
  const double j = 1.0 + (53.0 * std::log(2.0) - 2.0 * std::log(1.0 - b1) - 0.5 * std::log(b2 < 1.0 ? 1.0 - b2 : 1.0)) / -std::log(b1);
  return j < 1.0 ? 1 : j > 1e9 ? 1000000000 : (int32_t)std::ceil(j);
}
static RowCatchUp row_catch_up_args(const TrainState* T) {
  const coper_train_config& tc = T->cfg;
  RowCatchUp cu;
  cu.lr = tc.learning_rate; cu.b1 = tc.beta1; cu.b2 = tc.beta2; cu.eps = tc.epsilon;
  cu.l2b1 = cu.b1 > 0.0 ? std::log2(cu.b1) : 0.0; cu.l2b2 = cu.b2 > 0.0 ? std::log2(cu.b2) : 0.0;   // (a beta of 0: its powers are 0 at every gap)
  cu.l2b1p = T->rows_l2b1p; cu.l2b2p = T->rows_l2b2p;
  cu.b2f = tc.beta2;
  cu.now = T->rows_now;
  cu.jmax = rows_jmax(cu.b1, cu.b2);
  return cu;
}
// Ordered rows, behind an update's advance of the powers and of their log2: the log2 a catch-up reads is that of the power itself for
// as long as the power is a normal double -- a function of the powers (what coper_train_powers restores), not of how many additions
// led there, so handles with different histories catch rows up to the same bits.  Once a power has underflowed the sum carries on.
static void rows_log2_from_powers(TrainState* T) {
  if (!T->rows_ordered && !T->sharded) return;      // (a sharded state's sampled call is always ordered: the same rule, so a shard [0, num_ent) is that handle)
  if (T->b1p >= 1e-290) T->rows_l2b1p = std::log2(T->b1p);
  if (T->b2p >= 1e-290) T->rows_l2b2p = std::log2(T->b2p);
}
// a wave per row, four per workgroup, at most 8,192 workgroups (the kernels stride)
inline dim3 rows_grid(int64_t rows) { return dim3((unsigned)std::min<int64_t>(std::max<int64_t>((rows + 3) / 4, 1), 8192)); }
// coper_profile_read of the training step's structure (counts, no times -- as "band_lookup"): "train.zero.<leaf>" per whole-buffer zeroing
// of a leaf's gradient, "train.sumsq.leaves" / "train.amsgrad.leaves" the tensors k_tr_sumsq / k_tr_amsgrad were launched over,
// "train.rows.<kernel>" per launch of a row kernel
inline void prof_count(coper_handle* h, const std::string& what, int64_t n = 1) { if (h->profile) h->timers[what].launches += n; }

// One pass over E (a shard: its own rows): every row of ent_emb / pred_bias and their slots current (k_rows_sync; a row with gap 0 is not written).
static int rows_sync_launch(coper_handle* h, TrainState* T, hipStream_t s) {
  hipLaunchKernelGGL(k_rows_sync, rows_grid(rows_held(h, T)), dim3(256), 0, s, row_tables(h, T), row_catch_up_args(T));
  prof_count(h, "train.rows.sync");
  COPER_HIP_TRY(h, hipGetLastError());
  return COPER_OK;
}
// the step words are int32: close to the end, start counting again from a table that is current (every word 0 = rows_now)
static int rows_wrap_guard(coper_handle* h, TrainState* T, hipStream_t s) {
  if (T->rows_now < 0x7ffffff0) return COPER_OK;
  if (int rc = rows_sync_launch(h, T, s)) return rc;
  COPER_HIP_TRY(h, hipMemsetAsync(T->rows_word, 0, sizeof(int32_t) * (size_t)rows_held(h, T), s));
  T->rows_now = 0;
  return COPER_OK;
}
// the rows of the call before: their gradient rows, their claim bits; the other list's count (a claim or an import appends from 0)
static void rows_rezero_launch(coper_handle* h, TrainState* T, hipStream_t s) {
  const int pv = T->rows_prev;
  hipLaunchKernelGGL(k_rows_rezero, rows_grid(T->rows_cap), dim3(256), 0, s, row_tables(h, T), T->rows_list[pv].get(), T->rows_count + pv,
                     T->rows_claim.get(), T->rows_count + (pv ^ 1));
  prof_count(h, "train.rows.rezero");
}

// ---- ordered rows (kernels in train_order.h)
inline int64_t ord_tiles(int64_t n) { return std::max<int64_t>((n + ORD_TILE - 1) / ORD_TILE, 1); }
// 8-bit digit passes that cover the ids of [0, E)
inline int ord_passes(int64_t E) {
  int bits = 0;
  while (bits < 32 && ((int64_t)1 << bits) < E) ++bits;
  return std::max((bits + 7) / 8, 1);
}
// the sort's workspace at `n` entries or more (a host synchronisation of `s` when it grows, as every workspace of the step)
static int ord_grow(coper_handle* h, TrainState* T, int64_t n, hipStream_t s) {
  if (n <= T->ord_cap) return COPER_OK;
  int rc;
  COPER_HIP_TRY(h, hipStreamSynchronize(s));
  T->ord_cap = 0;
  for (int i = 0; i < 2; ++i)
    if ((rc = T->ord_key[i].alloc(h, (size_t)n, "ordered-rows sort")) || (rc = T->ord_val[i].alloc(h, (size_t)n, "ordered-rows sort"))) return rc;
  if ((rc = T->ord_seg.alloc(h, (size_t)n + 1, "ordered-rows segments")) || (rc = T->ord_list.alloc(h, (size_t)n, "ordered-rows list")) ||
      (rc = T->ord_hist.alloc(h, (size_t)257 * ord_tiles(n), "ordered-rows histograms")) ||
      (rc = T->ord_scan.alloc(h, (size_t)256 * ord_tiles(n), "ordered-rows histograms")) || (rc = T->ord_count.ensure(h, 1, "ordered-rows count")))
    return rc;
  T->ord_cap = n;
  return COPER_OK;
}
// The stable LSD sort of `n` entries (n_dev, when given: the device-side count, at most n) by key.  src: the first pass's input
// (OrdSrc).  with_vals: carry the entry indices.  Returns which of ord_key[] / ord_val[] holds the result.
static int ord_sort_launch(coper_handle* h, TrainState* T, hipStream_t s, OrdSrc src, const int32_t* n_dev, int64_t n, bool with_vals) {
  const int passes = ord_passes(h->dm.E);
  const unsigned tiles = (unsigned)ord_tiles(n);
  int cur = 0;
  for (int p = 0; p < passes; ++p) {
    cur = p & 1;
    hipLaunchKernelGGL(k_ord_hist, dim3(tiles), dim3(256), 0, s, src, n_dev, n, 8 * p, T->ord_hist.get());
    hipLaunchKernelGGL(k_ord_scan, dim3(256), dim3(256), 0, s, (const int32_t*)T->ord_hist.get(), (int)tiles, T->ord_scan.get());
    hipLaunchKernelGGL(k_ord_scatter, dim3(tiles), dim3(256), 0, s, src, n_dev, n, 8 * p, (const int32_t*)T->ord_scan.get(), T->ord_key[cur].get(),
                       with_vals ? T->ord_val[cur].get() : nullptr);
    prof_count(h, "train.order.sort", 3);
    src.keys = T->ord_key[cur];
    src.vals = with_vals ? T->ord_val[cur].get() : nullptr;
  }
  return cur;
}
// The pending list of the deferred-rows mode in ascending id again, after imports appended to it (k_rows_import: wave-arrival order):
// a keys-only sort of the listed ids, copied back.  In front of what reads the list in order: the norm of coper_train_rows_apply,
// coper_train_rows_export.
static int ord_sort_pending_list(coper_handle* h, TrainState* T, hipStream_t s) {
  if (!T->rows_ordered || !T->rows_list_unsorted) return COPER_OK;
  const int64_t n = T->rows_bound;
  if (n > 0) {
    if (int rc = ord_grow(h, T, n, s)) return rc;
    const int pv = T->rows_prev;
    OrdSrc src{T->rows_list[pv].get(), nullptr, nullptr, nullptr, 0, (int64_t)h->dm.E};
    const int at = ord_sort_launch(h, T, s, src, T->rows_count + pv, n, false);
    // (entries behind the count are whatever the buffers held: nothing reads them)
    COPER_HIP_TRY(h, hipMemcpyAsync(T->rows_list[pv], T->ord_key[at], sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, s));
    COPER_HIP_TRY(h, hipGetLastError());
  }
  T->rows_list_unsorted = false;
  return COPER_OK;
}

// ---- the update: the tensor table of k_tr_sumsq / k_tr_amsgrad, their launches, the host's bookkeeping behind them
enum class LeafSet { All, Small /* every leaf but ent_emb and pred_bias */, Tables /* those two */ };
enum class GradSrc { Buffers /* TrainParam::g */, FlatVector /* `vec` at each leaf's flat_off */, SmallVector /* ... at its small_off */ };
// Fills `tt` with the leaves of `which` in T->tp order and returns how many.  table_counts: the relation counts that say which rows of
// the looked-up dense table exist.  carry_wmax: the table hands k_tr_amsgrad wmax[wmax_cur ^ 1] for the dense weights' largest |p_new|
// (the next step's packs read it) -- on its 16-byte path only: it is the one that carries it.  found: where `find` sits in the table.
static int train_tensors(const coper_handle* h, TrainState* T, LeafSet which, GradSrc src, const float* vec, const int32_t* table_counts,
                         bool carry_wmax, TrainTensors& tt, const TrainParam* find = nullptr, int* found = nullptr) {
  const Dims& dm = h->dm;
  const TrainLeaves& lv = T->lv;
  const bool lk = dm.lookup && dm.gen_fc, gen = dm.gen_fc && !dm.lookup;
  const TrainParam* const W = gen ? lv.gen[0].proj[T->nh] : lv.fc_weights;
  int np = 0;
  tt.wmax = nullptr; tt.wmax_of = -1;
  for (const TrainParam& t : T->tp) {
    const bool is_table = &t == lv.ent_emb || &t == lv.pred_bias;
    if (which != LeafSet::All && is_table != (which == LeafSet::Tables)) continue;
    const int i = np++;
    tt.p[i] = t.p; tt.m[i] = t.m; tt.v[i] = t.v; tt.vh[i] = t.vh;
    tt.g[i] = src == GradSrc::Buffers ? t.g.get() : const_cast<float*>(vec) + (src == GradSrc::SmallVector ? t.small_off : t.flat_off);
    tt.n[i] = t.n;
    const bool table = lk && &t == lv.fc_weights;
    tt.rowlen[i] = table ? dm.F * (int64_t)dm.d : 1;
    tt.rowcnt[i] = table ? table_counts : nullptr;
    if (found && &t == find) *found = i;
    if (carry_wmax && !lk && &t == W && ((((uintptr_t)tt.p[i]) | ((uintptr_t)tt.g[i]) | ((uintptr_t)tt.m[i]) | ((uintptr_t)tt.v[i]) | ((uintptr_t)tt.vh[i])) & 15) == 0) {
      tt.wmax = T->wmax[T->wmax_cur ^ 1];
      tt.wmax_of = i;
    }
  }
  return np;
}
// deterministic mode: the squared norm of the table's tensors -- every workgroup's sum into the slab, their fold in one order into *out
static void sumsq_det_launch(TrainState* T, hipStream_t s, const TrainTensors& tt, int np, double* out) {
  hipLaunchKernelGGL(k_tr_sumsq<true>, dim3(512, (unsigned)np), dim3(256), 0, s, tt, -1, T->det_slab.get());
  hipLaunchKernelGGL(k_tr_fold_det, dim3(1), dim3(256), 0, s, T->det_slab.get(), 1, (int64_t)512 * np, out, 0);
}
// clip by the slots' sum + AMSGrad at this update's learning rate (returned); gs: the gradients' scale
static float amsgrad_launch(TrainState* T, hipStream_t s, const TrainTensors& tt, int np, double gs) {
  const coper_train_config& tc = T->cfg;
  const RedLayout red = T->red_layout();
  const float lr_t = (float)((double)tc.learning_rate * std::sqrt(1.0 - T->b2p) / (1.0 - T->b1p));
  hipLaunchKernelGGL(k_tr_amsgrad, dim3(2048, (unsigned)np), dim3(256), 0, s, tt, red.sumsq_slots(), red.total_sumsq(), tc.clip_norm, lr_t, tc.beta1,
                     tc.beta2, tc.epsilon, gs);
  return lr_t;
}
// In front of an update from gradients that an earlier call left: the squared-norm slots hold what that backward's GEMM epilogues added,
// wmax[wmax_cur ^ 1] what the update before last left
static void zero_update_slots(TrainState* T, hipStream_t s) {
  ZeroList zl;
  zl.n = 2;
  zl.p[0] = T->red_layout().sumsq_slots(); zl.bytes[0] = sizeof(double) * TG_SUMSQ_SLOTS;
  zl.p[1] = T->wmax[T->wmax_cur ^ 1].get(); zl.bytes[1] = sizeof(unsigned) * TG_MAX_SLOTS;
  hipLaunchKernelGGL(k_tr_zero_list, dim3(8, (unsigned)zl.n), dim3(256), 0, s, zl);
}
// The host's bookkeeping behind an optimizer pass.  Deferred rows: k_rows_update wrote the listed rows' words -- current as of this update.
static void finish_update(TrainState* T, bool wmax_carried) {
  if (T->rows_deferred) {
    T->rows_now += 1;
    T->rows_l2b1p += T->cfg.beta1 > 0.f ? std::log2((double)T->cfg.beta1) : 0.0;
    T->rows_l2b2p += T->cfg.beta2 > 0.f ? std::log2((double)T->cfg.beta2) : 0.0;
  }
  T->b1p *= T->cfg.beta1;
  T->b2p *= T->cfg.beta2;
  if (T->rows_deferred) rows_log2_from_powers(T);
  T->wmax_cur ^= 1;
  T->wmax_valid = wmax_carried;
}

// clip + AMSGrad over every trainable tensor: the squared norm (k_tr_sumsq; deterministic mode: through the slab and its fold), then
// k_tr_amsgrad.  Deferred rows: ent_emb and pred_bias are left out of both launches, and the rows of `rows_list` (its length on the
// device, `rows_count`) go through k_rows_sumsq / k_rows_update between and behind them.  The caller has zeroed the squared-norm slots
// and wmax[wmax_cur ^ 1].  flat: the gradients are read from the flat gradient vector in place (each leaf at its flat_off) instead of the gradient buffers.  sumsq_done: the leaf whose squares a GEMM of
// the same step already added to the slots.  table_counts: the relation counts that say which rows of the looked-up dense table
// exist.  gs: coper_train_apply's scale (1: the fused step).  flat_small: `flat` is the small flat vector of coper_train_rows_apply (each
// leaf at its small_off; with rows_list).  Returns whether the pass carried the dense weights' maximum.
static bool optimizer_launch(coper_handle* h, TrainState* T, hipStream_t s, const float* flat, const TrainParam* sumsq_done,
                             const int32_t* table_counts, double gs, const int32_t* rows_list = nullptr, const int32_t* rows_count = nullptr,
                             bool flat_small = false, int64_t rows_n = 0 /* ordered rows: the host's bound of the list's length */) {
  const coper_train_config& tc = T->cfg;
  const RedLayout red = T->red_layout();
  TrainTensors tt;      // tensors of the two launches: every leaf, or every leaf but the two tables
  int skip = -1;
  const int np = train_tensors(h, T, rows_list ? LeafSet::Small : LeafSet::All, !flat ? GradSrc::Buffers : flat_small ? GradSrc::SmallVector : GradSrc::FlatVector,
                               flat, table_counts, true, tt, sumsq_done, &skip);
  double* const ssq = red.sumsq_slots();
  if (T->det) sumsq_det_launch(T, s, tt, np, ssq);      // (skip is -1: no GEMM added squares) into slot 0 of the zeroed slots
  else hipLaunchKernelGGL(k_tr_sumsq<false>, dim3(512, (unsigned)np), dim3(256), 0, s, tt, skip, ssq);
  prof_count(h, "train.sumsq.leaves", np);
  if (rows_list && T->rows_ordered) {
    // the listed rows' share in partial sums of ORD_SUMSQ_ROWS list positions (the slab is free again behind the fold above), folded
    // into slot 1: the small leaves' share in slot 0, the rows' in slot 1, and every reader adds the slots in index order
    const int64_t parts = std::max<int64_t>((rows_n + ORD_SUMSQ_ROWS - 1) / ORD_SUMSQ_ROWS, 1);
    hipLaunchKernelGGL(k_rows_sumsq_ord, dim3((unsigned)parts), dim3(256), 0, s, row_tables(h, T), rows_list, rows_count, T->det_slab.get());
    hipLaunchKernelGGL(k_tr_fold_det, dim3(1), dim3(256), 0, s, T->det_slab.get(), 1, parts, ssq + 1, 0);
    prof_count(h, "train.order.sumsq");
  } else if (rows_list) {
    hipLaunchKernelGGL(k_rows_sumsq, rows_grid(T->rows_cap), dim3(256), 0, s, row_tables(h, T), rows_list, rows_count, ssq);
    prof_count(h, "train.rows.sumsq");
  }
  const float lr_t = amsgrad_launch(T, s, tt, np, gs);
  prof_count(h, "train.amsgrad.leaves", np);
  if (rows_list) {      // (behind k_tr_amsgrad on the same stream: both read the slots, neither writes them)
    hipLaunchKernelGGL(k_rows_update, rows_grid(T->rows_cap), dim3(256), 0, s, row_tables(h, T), rows_list, rows_count, (const double*)ssq,
                       tc.clip_norm, lr_t, tc.beta1, tc.beta2, tc.epsilon, gs, T->rows_now + 1);
    prof_count(h, "train.rows.update");
  }
  return tt.wmax != nullptr;
}

// The stages of a step in execution order: the one schedule of this file.  Every entry point runs a range of it (Step::run) -- the fused
// calls [ConvFilters, End) or, forward only, [ConvFilters, ScorerBwd); the calls of a step held open (OpenStep) the ranges between their
// exchanges.  The *Sums stages end where a batch-wide sum is needed.
enum class Stage {
  ConvFilters, Bn1Sums, Bn1, Dense, FcbnSums, Fcbn, Score,
  ScorerBwd, FcbnBwdSums, FcbnBwd, DenseBwd, ChainsBwd, Bn1BwdSums, Bn1Bwd, ConvBwd, ConvFiltersBwd, End
};

// One call of the step: its arguments (StepArgs), what they and the configuration decide once, the few values a stage hands to a later
// one (and StepCarry), the stages themselves and run(), which executes a range of them.
struct Step : StepArgs, StepCarry {
  coper_handle* const h;
  TrainState* const T;
  const Dims& dm; const coper_train_config& tc; const TrainLeaves& lv;
  Step(coper_handle* h_, TrainState* T_, const StepArgs& a) : StepArgs(a), h(h_), T(T_), dm(h_->dm), tc(T_->cfg), lv(T_->lv) {}
  const int nomov = keeps_moving_stats(kind) ? 2 : 0, use_batch = tc.batch_norm_train_stats ? 1 : 0;
  const bool one_vs_all = !plan.sampled();   // use_negative_sampling = False: labels are the dense e2_multi [B, |E|] or id lists
  const bool cat = dm.concat_rel, two_streams = T->side[0] != nullptr;
  const bool det = T->det;          // coper_train_config.deterministic: every sum in one defined order
  const bool lk = dm.lookup && dm.gen_fc;    // dense layer from g_lookup tables (otherwise static: models.py:217-228 with context_rel_out None)
  const bool gen = dm.gen_fc && !dm.lookup;
  const bool genc = dm.gen_conv && !dm.lookup, lkc = dm.gen_conv && dm.lookup;     // conv filters from projection generators / g_lookup tables
  const int d = dm.d, r = dm.r, C = dm.C, P = dm.Ho * dm.Wo, isz = dm.in_h * dm.in_w, NT = dm.fh * dm.fw;   // NT: filter taps
  const int64_t F = dm.F, Fc = dm.F_conv, nBF = B * Fc, nBd = B * d;   // dense input width (F_conv + r under concat_rel), conv features
  const int nh = T->nh, nhc = T->nhc;
  const int rc_w = nh ? T->chain[0].dims[nh] : r, rc_b = nh ? T->chain[1].dims[nh] : r;   // widths of the contexts that multiply the last projections
  const int rc_cw = nhc ? T->chain[2].dims[nhc] : r, rc_cb = nhc ? T->chain[3].dims[nhc] : r;
  const uint32_t thr_h = dropout_threshold24(tc.hidden_dropout), thr_o = dropout_threshold24(tc.output_dropout), thr_c = dropout_threshold24(tc.context_rel_dropout);
  const float ks_h = 1.f / (1.f - tc.hidden_dropout), ks_o = 1.f / (1.f - tc.output_dropout), ks_c = 1.f / (1.f - tc.context_rel_dropout);
  const uint32_t step = T->step;
  // the dropout counter of element i of a [B, n] tensor is (sample_offset + b) n + j: i plus these (0 outside a synchronised step)
  uint32_t drop_off(int64_t n) const { return (uint32_t)(sample_offset * n); }
  const uint32_t off_h = drop_off(dm.F_conv), off_o = drop_off(dm.d);
  const int64_t Bn = B_stat ? B_stat : B;      // the samples the batch statistics of Conv1BN / FCBN are taken over
  const float inv_BL = (float)(1.0 / ((double)B * (double)L));
  const RedLayout red = T->red_layout();
  float *const mean1 = T->bn_row(BN1_MEAN), *const inv1 = T->bn_row(BN1_INV), *const mean2 = T->bn_row(FCBN_MEAN), *const inv2 = T->bn_row(FCBN_INV);
  SideJoin sj{T, s};
  const bool rows = T->rows_deferred;
  // ---- from phase to phase (and StepCarry)
  float *Tf = nullptr, *dTf = nullptr;                // generated dense: T[rho][b][k] | dT (in T->A, once grow_workspaces has seen to it)
  const float *K_ps = nullptr, *kb_ps = nullptr;      // per-sample conv filters / biases (T->Kt, T->Kbv; null where they are static)
  int t_slices = 1, dx_slices = 1;   // K slices the T and dx products left for k_tr_fc_post_slices / k_tr_bn1_bwd_sums to add
  const TrainParam* sumsq_done = nullptr;   // the leaf whose squared gradient norm its own GEMM accumulated
  const int32_t *rows_list = nullptr, *rows_count = nullptr;   // deferred rows: the rows this call claimed (rows_claim_catch_up)
  // Set by the driver of a step that is open across exchanges (coper_train_sync_next): TrainState::sync_sums, [2][2 mx] doubles.  The
  // FCBN backward runs as its sums | apply pair around the exchange and the two backward apply stages read the whole batch's sums from
  // [0] (bwd_all_sums); null (every other call): one k_tr_fcbn_bwd launch, and Conv1BN's backward reads this call's own sums.
  double* sync_sums = nullptr;
  double* bwd_all_sums() const { return sync_sums; }
  bool scorer_bwd_on_side() const { return two_streams && plan.dh == DhRoute::Fused && tg_split_k(dm.E, d, B) == 1; }

  int grow_workspaces() {
    int rc;
    if (B > T->capB || (!one_vs_all && L > T->capL)) {
      COPER_HIP_TRY(h, hipStreamSynchronize(s));
      int64_t cb = B > T->capB ? B : T->capB, cl = (!one_vs_all && L > T->capL) ? L : (T->capL > 0 ? T->capL : 1);
      T->capB = T->capL = 0;      // (until the last of them exists: a failure leaves the whole group to the next step)
      auto ws = [&](auto& buf, size_t n) { return buf.alloc(h, n, "training workspace"); };
      if ((rc = ws(T->img, (size_t)cb * isz)) || (rc = ws(T->y, (size_t)cb * F)) ||
          (rc = ws(T->x, (size_t)cb * F)) ||
          // (dx doubles as the looked-up dense layer's scratch: TR_LK_NSL partial sums of [B, d] -- more than [B, F] where F < 4 d: a fuzz
          //  shape of round 6, d = 77 with three channels, wrote past the end of it)
          (rc = ws(T->dx, (size_t)cb * (size_t)(F > (int64_t)TR_LK_NSL * d ? F : (int64_t)TR_LK_NSL * d))) ||
          (rc = ws(T->c, (size_t)cb * r)) || (rc = ws(T->dc, (size_t)cb * r)) ||
          (rc = ws(T->z0, (size_t)cb * d)) || (rc = ws(T->z1, (size_t)cb * d)) ||
          (rc = ws(T->hv, (size_t)cb * d)) || (rc = ws(T->dh, (size_t)cb * d)) ||
          (rc = ws(T->dz, (size_t)cb * d)) || (rc = ws(T->ds, (size_t)cb * cl)))      // (capL entries per sample whatever this call's label form: capL is what the next sampled call compares its L with)
        return rc;
      if (cat && ((rc = ws(T->xc, (size_t)cb * F)) || (rc = ws(T->dxc, (size_t)cb * F)))) return rc;
      if (gen) {
        if ((rc = ws(T->A, (size_t)2 * rc_w * cb * d))) return rc;
        const int64_t nrk = (int64_t)rc_w * d;
        struct { PlaneSet* p; int64_t rows, K; } planes[] = {{&T->pX, cb, F}, {&T->pXt, F, cb}, {&T->pP1, nrk, F}, {&T->pP3, F, nrk},
                                                            {&T->pTn, nrk, cb}, {&T->pTb, cb, nrk}};
        for (auto& pl : planes)
          if ((rc = ws(pl.p->hi, tg_plane_elems(pl.rows, pl.K))) || (rc = ws(pl.p->lo, tg_plane_elems(pl.rows, pl.K)))) return rc;
      }
      for (int g = 0; g < 4; ++g) {
        if (g < 2 ? !gen : !genc) continue;
        const int nhx = g < 2 ? nh : nhc;
        TrainState::Chain& ch = T->chain[g];
        for (int i = 0; i <= nhx; ++i) {
          if (i > 0 && (rc = ws(ch.v[i], (size_t)cb * ch.dims[i]))) return rc;
          if ((rc = ws(ch.dv[i], (size_t)cb * ch.dims[i]))) return rc;
          if (i < nhx && ((rc = ws(ch.u[i], (size_t)cb * ch.dims[i + 1])) || (rc = ws(ch.a[i], (size_t)cb * ch.dims[i + 1])) ||
                          (rc = ws(ch.du[i], (size_t)cb * ch.dims[i + 1])) || (rc = ws(ch.st[i], (size_t)2 * ch.dims[i + 1]))))
            return rc;
        }
      }
      if (dm.gen_conv && ((rc = ws(T->Kt, (size_t)cb * NT * C)) || (rc = ws(T->Kbv, (size_t)cb * C)))) return rc;
      // per-query filter / bias gradients: what the generators and tables reduce (gen_conv), and -- round 6 -- what the STATIC filters'
      // gradients are summed from (512 workgroups adding to the same 320 addresses were 50 of k_tr_conv_bwd's 60 us)
      if ((rc = ws(T->dKs, (size_t)cb * NT * C)) || (rc = ws(T->dkbs, (size_t)cb * C))) return rc;
      if (det && ((rc = ws(T->dimg, (size_t)cb * isz)) || (rc = ws(T->det_perm, (size_t)cb)))) return rc;
      T->capB = cb; T->capL = cl;
    }
    if (det) {
      // the slab of the widest reducing launch: DET_CS_WGS workgroups of column sums (2 mx doubles each), a loss kernel's grid (B, 2048,
      // or B x the stretches of a chunk), k_tr_sumsq's 512 x tensors
      const bool ordered = plan.ordered();
      const int64_t cwid = (csr.indptr || plan.shard) ? ova_chunk(B, plan.n, tc.one_vs_all_chunk) : 0;
      size_t need = (size_t)DET_CS_WGS * 2 * T->mx;
      // (as floats: the 64-row stretches of a column sum over |E|, the filter taps or d columns, or of the [rc_b, d] bias-projection product)
      // (ordered rows: no column sum over |E|; the partial sums of the listed rows' norm instead)
      const size_t widest = std::max({(size_t)((one_vs_all || ordered) ? 0 : dm.E), (size_t)NT * C, (size_t)d, (size_t)rc_b * d});
      for (size_t n : {(size_t)2048, (size_t)B, (size_t)(B * ((cwid + TR_CSR_STRETCH - 1) / TR_CSR_STRETCH)), (size_t)512 * TR_MAX_PARAMS,
                       (size_t)((B + 63) / 64) * widest / 2 + 1, (size_t)(ordered ? (B * (L + 1) + ORD_SUMSQ_ROWS - 1) / ORD_SUMSQ_ROWS + 1 : 0)})
        need = n > need ? n : need;
      if (need > T->det_slab.size()) {
        COPER_HIP_TRY(h, hipStreamSynchronize(s));
        if ((rc = T->det_slab.alloc(h, need, "deterministic slabs"))) return rc;
      }
    }
    // (Round 6 tried the sampled scorer's forward and dh in ONE pass over the gathered rows -- a wave per row, the score a butterfly
    //  sum over its lanes: 242 us against 61 + 45 for the two kernels.  Thirty-two sequential iterations per wave, each with two
    //  dependent round trips and eight six-step cross-lane sums, are latency end to end; removed.)
    if (plan.table == TableGrad::DenseS && (size_t)(B * dm.E) > T->Sd.size()) {
      COPER_HIP_TRY(h, hipStreamSynchronize(s));
      if ((rc = T->Sd.alloc(h, (size_t)(B * dm.E), "training workspace"))) return rc;
    }
    Tf = T->A;
    dTf = T->A + (size_t)rc_w * nBd;
    K_ps = dm.gen_conv ? T->Kt.get() : nullptr;
    kb_ps = dm.gen_conv ? T->Kbv.get() : nullptr;
    plan.resolve_dh(d, L, lv.ent_emb->p, T->dh.get(), T->hv.get());
    return COPER_OK;
  }
  // ---- deterministic mode: the launches that replace an atomic site
  static constexpr int DET_CS_WGS = 256;      // workgroups (= slabs) of a column-sum launch
  void det_fold(int n, int64_t nslots, double* out, int accumulate) {
    hipLaunchKernelGGL(k_tr_fold_det, dim3((unsigned)n), dim3(256), 0, s, T->det_slab.get(), n, nslots, out, accumulate);
  }
  // per-column sum | sum of squares of m [rows, cols] -> cs
  void det_col_sums(const float* m, int64_t rows, int cols, double* cs, int wgs) {
    hipLaunchKernelGGL(k_tr_col_sums<true>, dim3((unsigned)wgs), dim3(256), 0, s, m, rows, cols, T->det_slab.get(), 1);
    det_fold(2 * cols, wgs, cs, 0);
  }
  // out[c] = the column sum of src [B, cols]: stretches of 64 rows as the default mode's launch, stored, then added in ascending stretch
  void det_col_sum_f32(const float* src, int64_t cols, float* out, hipStream_t q) {
    const unsigned nz = (unsigned)((B + 63) / 64);
    hipLaunchKernelGGL(k_tr_col_sums_add<true>, dim3((unsigned)((cols + 255) / 256), nz), dim3(256), 0, q, src, B, cols, (float*)T->det_slab.get());
    hipLaunchKernelGGL(k_tr_fold_f32_det, grid1d(cols), dim3(256), 0, q, (const float*)T->det_slab.get(), cols, (int)nz, out);
  }
  // dst[key[b]] += src[b, col0 : col0 + n], one writer per row, ascending b
  void det_rows_by_key(const float* src, int64_t stride, int64_t col0, int n, const int64_t* keys, int64_t K, float* dst) {
    hipLaunchKernelGGL(k_tr_rows_by_key_det, dim3((unsigned)B), dim3(256), 0, s, src, stride, col0, n, keys, K, B, dst);
  }
  // ---- zero what is accumulated by atomics: one launch
  void zero_accumulators() {
    ZeroList zl;
    zl.n = 0;
    auto add = [&](void* p, size_t bytes) { if (p && bytes && zl.n < TR_ZERO_MAX) { zl.p[zl.n] = p; zl.bytes[zl.n] = bytes; ++zl.n; } };
    auto grad = [&](const TrainParam* t) { if (t) { add(t->g, sizeof(float) * t->n); if (h->profile) prof_count(h, "train.zero." + t->name); } };
    add(red.base, sizeof(double) * red.doubles());
    // (deferred rows: the two tables' gradients are zero but for the rows of the call before, which rows_rezero clears)
    for (const TrainParam* t : {rows ? nullptr : lv.ent_emb, lv.rel_emb, lv.conv1_weights, lv.conv1_bias, rows ? nullptr : lv.pred_bias}) grad(t);
    if (lk) grad(lv.fc_bias);
    else if (gen) add(lv.gen[1].proj[nh]->g, sizeof(float) * rc_b * d);
    else add(lv.fc_bias->g, sizeof(float) * d);
    // (the dense S of the sampled scorer's backward is written whole by k_tr_build_S: nothing to zero)
    if (runs_optimizer(kind)) add(T->wmax[T->wmax_cur ^ 1], sizeof(unsigned) * TG_MAX_SLOTS);      // what this step's optimizer pass fills for the next step
    for (unsigned* slots : {T->xmax.get(), T->dtmax.get(), T->smax.get()}) add(slots, sizeof(unsigned) * TG_MAX_SLOTS);
    hipLaunchKernelGGL(k_tr_zero_list, dim3(256, (unsigned)zl.n), dim3(256), 0, s, zl);
    T->exp_cache.clear();
    w_slots = T->wmax_valid ? T->wmax[T->wmax_cur].get() : nullptr;
    // (a coper_group_next registration, or a grouping prepared ahead, was for an evaluation pass: a training step drops both)
    h->pipe.invalidate_grouping();
  }
  // The same for a forward-only call on a sharded state, which leaves the last step's gradients and its global norm where
  // they are: the reduction scratch but for the norm's double, and the maximum slots the forward kernels fill -- no gradient buffer.
  void zero_forward_scratch() {
    ZeroList zl;
    zl.n = 0;
    auto add = [&](void* p, size_t bytes) { zl.p[zl.n] = p; zl.bytes[zl.n] = bytes; ++zl.n; };
    add(red.loss(), sizeof(double));
    add(red.total_sumsq() + 1, sizeof(double) * (red.doubles() - 2));
    for (unsigned* slots : {T->xmax.get(), T->dtmax.get(), T->smax.get()}) add(slots, sizeof(unsigned) * TG_MAX_SLOTS);
    hipLaunchKernelGGL(k_tr_zero_list, dim3(256, (unsigned)zl.n), dim3(256), 0, s, zl);
    T->exp_cache.clear();
    w_slots = T->wmax_valid ? T->wmax[T->wmax_cur].get() : nullptr;
    h->pipe.invalidate_grouping();
  }
  // ---- deferred rows, in front of every forward kernel: the id lists hold B (L + 1) entries
  int rows_grow() {
    const int64_t need = B * (L + 1);
    if (need <= T->rows_cap) return COPER_OK;
    int rc;
    // the list of the call before is still owed its re-zero: pay it from the old buffers, then replace both
    if (T->rows_cap) rows_rezero_launch(h, T, s);
    COPER_HIP_TRY(h, hipStreamSynchronize(s));
    T->rows_cap = 0;
    if ((rc = T->rows_list[0].alloc(h, (size_t)need, "deferred-row list")) || (rc = T->rows_list[1].alloc(h, (size_t)need, "deferred-row list"))) return rc;
    COPER_HIP_TRY(h, hipMemsetAsync(T->rows_count, 0, 2 * sizeof(int32_t), s));
    T->rows_cap = need;
    return COPER_OK;
  }
  // 1. + 2. claim the batch's rows into the free list and bring them current.  The list is the handle's "list of the call before" from
  // here on, whatever becomes of the call: the next one re-zeroes it.
  void rows_claim_catch_up() {
    const int cur = T->rows_prev ^ 1;
    const int64_t n = B * (L + 1);
    // (ordered rows: the list is the sort's segment heads -- ascending id -- and the heads set the claim bits)
    if (plan.ordered()) order_rows(T->rows_list[cur].get(), T->rows_count + cur, T->rows_claim.get());
    else {
      hipLaunchKernelGGL(k_rows_claim, grid1d(n), dim3(256), 0, s, e1, B, lookup, n, (int64_t)dm.E, T->rows_claim.get(), T->rows_list[cur].get(),
                         T->rows_count + cur);
      prof_count(h, "train.rows.claim");
    }
    T->rows_prev = cur;
    T->rows_list_unsorted = false;
    rows_list = T->rows_list[cur];
    rows_count = T->rows_count + cur;
    hipLaunchKernelGGL(k_rows_catch_up, rows_grid(n), dim3(256), 0, s, row_tables(h, T), row_catch_up_args(T), rows_list, rows_count);
    prof_count(h, "train.rows.catch_up");
  }
  // The same on a shard, in front of the sampled scorer: the sort and the heads over ALL B (L + 1) ids (k_ord_reduce reads
  // them as with the mode off), the owned run of the heads as local rows into the free list with their claim bits, those rows current.
  void shard_rows_list_catch_up() {
    const int cur = T->rows_prev ^ 1;
    const int64_t n = B * (L + 1), most = std::min<int64_t>(n, plan.n);
    order_rows(T->ord_list.get(), T->ord_count.get(), nullptr);
    hipLaunchKernelGGL(k_shard_list_owned, dim3((unsigned)std::min<int64_t>(std::max<int64_t>((most + 255) / 256, 1), 1024)), dim3(256), 0, s,
                       (const int32_t*)T->ord_list.get(), (const int32_t*)T->ord_count.get(), plan.lo, plan.n, T->rows_list[cur].get(), T->rows_count + cur,
                       T->rows_claim.get());
    prof_count(h, "train.rows.list_owned");
    T->rows_prev = cur;
    T->rows_list_unsorted = false;
    rows_list = T->rows_list[cur];
    rows_count = T->rows_count + cur;
    hipLaunchKernelGGL(k_rows_catch_up, rows_grid(most), dim3(256), 0, s, row_tables(h, T), row_catch_up_args(T), rows_list, rows_count);
    prof_count(h, "train.rows.catch_up");
  }
  // ---- ordered rows: the B L lookup ids and the B e1 ids in ascending (id, b, l) -- the stable sort -- then the segment
  // heads: the batch's unique rows ascending into `list` / `count`, their segment offsets into T->ord_seg, their claim bits when asked.
  // Once per call: in front of the forward pass with deferred rows (the list is what is caught up), else in front of the reduce.
  void order_rows(int32_t* list, int32_t* count, unsigned* claim) {
    const int64_t n = B * (L + 1);
    OrdSrc src{nullptr, nullptr, e1, lookup, B * L, (int64_t)dm.E};
    const int at = ord_sort_launch(h, T, s, src, nullptr, n, true);
    const unsigned tiles = (unsigned)ord_tiles(n);
    int32_t* const tile_heads = T->ord_hist + (size_t)256 * tiles;
    hipLaunchKernelGGL(k_ord_head_count, dim3(tiles), dim3(256), 0, s, (const int32_t*)T->ord_key[at].get(), n, tile_heads);
    hipLaunchKernelGGL(k_ord_heads, dim3(tiles), dim3(256), 0, s, (const int32_t*)T->ord_key[at].get(), n, (const int32_t*)tile_heads, list,
                       T->ord_seg.get(), count, claim);
    prof_count(h, "train.order.heads", 2);
    ord_vals = T->ord_val[at];
    ord_rows = list;
    ord_rows_count = count;
  }
  // looked-up dense table: group the batch by relation (perm / rel_offset / rel_count of the inference path): the table gradient is
  // written per present relation, never zero-filled (1.75 GB at FB15k-237 shapes)
  int group_for_lookup() {
    int rc;
    if ((rc = coper_reserve(h, B, 0, (void*)s))) return rc;
    h->gcur = 0;
    if ((rc = launch_group_by_relation(h, e1, rel, plan.shard /* no table row is looked up by e1 there */, B, 32, s))) return rc;
    if (differentiates(kind)) COPER_HIP_TRY(h, hipMemcpyAsync(T->step_rel_count, h->grouping().rel_count, sizeof(int32_t) * ((size_t)dm.R + 1), hipMemcpyDeviceToDevice, s));
    // (the grouping's order inside a relation is arrival order, and the order k_tr_lookup_dW sums in: a sorted copy for it)
    if (det && differentiates(kind))
      hipLaunchKernelGGL(k_tr_sort_groups_det, dim3((unsigned)dm.R), dim3(256), 0, s, h->grouping().perm, h->grouping().rel_offset,
                         h->grouping().rel_count, T->det_perm.get());
    return COPER_OK;
  }
  // ---- forward
  // g_MLP generator chain g: context rows c -> v[nhx] (models.py:56-68); g_linear: the context is c itself
  void chain_forward(int g, int nhx) {
    TrainState::Chain& ch = T->chain[g];
    for (int i = 0; i < nhx; ++i) {
      const int ni = ch.dims[i], nj = ch.dims[i + 1];
      const TrainLeaves::Bn& b = lv.gen[g].bn[i];
      const int64_t tot = B * nj;
      hipLaunchKernelGGL(k_tr_small_mm, grid1d(tot), dim3(256), 0, s, i ? ch.v[i] : T->c, lv.gen[g].proj[i]->p, B, ni, nj, ch.u[i]);
      const float *ga = nullptr, *be = nullptr;
      if (dm.ctx_bn) {
        double* cs = red.colsum_slice(cs_chain(g, i));
        if (use_batch && det) det_col_sums(ch.u[i], B, nj, cs, 64);
        else if (use_batch) hipLaunchKernelGGL(k_tr_col_sums<false>, dim3(64), dim3(256), 0, s, ch.u[i], B, nj, cs, 1);
        hipLaunchKernelGGL(k_tr_bn_finish, dim3((nj + 63) / 64), dim3(64), 0, s, cs, nj, (double)B, use_batch, tc.batch_norm_momentum, 0 | nomov,
                           b.mov_mean, b.mov_var, ch.st[i], ch.st[i] + nj);
        ga = b.gamma->p;
        be = b.beta->p;
      }
      hipLaunchKernelGGL(k_tr_chain_act, grid1d(tot), dim3(256), 0, s, ch.u[i], ch.st[i], ga, be, nj, tot, tc.seed, step, drop_off(nj),
                         dropout_stage_chain(g, i), thr_c, ks_c, ch.a[i], ch.v[i + 1]);
    }
  }
  // per-sample conv filters (models.py:231-250,374-380): generated from the relation rows, or looked up
  void fwd_conv_filters() {
    if (genc) {
      hipLaunchKernelGGL(k_tr_gather_rows, grid1d(B * r), dim3(256), 0, s, lv.rel_emb->p, rel, dm.R, r, B * r, T->c);
      for (int g : {2, 3}) chain_forward(g, nhc);
      ccw = nhc ? T->chain[2].v[nhc] : T->c;
      ccb = nhc ? T->chain[3].v[nhc] : T->c;
      hipLaunchKernelGGL(k_tr_small_mm, grid1d(B * NT * C), dim3(256), 0, s, ccw, lv.gen[2].proj[nhc]->p, B, rc_cw, NT * C, T->Kt);
      hipLaunchKernelGGL(k_tr_small_mm, grid1d(B * C), dim3(256), 0, s, ccb, lv.gen[3].proj[nhc]->p, B, rc_cb, C, T->Kbv);
    } else if (lkc) {
      hipLaunchKernelGGL(k_tr_gather_rows, grid1d(B * NT * C), dim3(256), 0, s, lv.conv1_weights->p, rel, dm.R, NT * C, B * NT * C, T->Kt);
      hipLaunchKernelGGL(k_tr_gather_rows, grid1d(B * C), dim3(256), 0, s, lv.conv1_bias->p, rel, dm.R, C, B * C, T->Kbv);
    }
  }
  // the conv, Conv1BN, ReLU, dropout -> x [B, F_conv]; concat_rel: [x | c]
  // In two stages, cut where a batch-wide sum is needed: the conv and the column sums of this call's rows | the
  // statistics from the sums (over Bn samples) and what follows.  bn1_fwd_sums(): where the first stage leaves the sums.
  double* bn1_fwd_sums() const { return red.cs_slots(CSS_BN1_FWD); }
  void fwd_conv_sums() {
    const size_t lds_conv = sizeof(float) * (size_t)(isz + (NT + 1) * C);
    // (sharded: the image of sample b is row b of the gathered rows)
    hipLaunchKernelGGL(k_tr_conv_fwd, dim3((unsigned)B), dim3(256), lds_conv, s, img_rows ? T->sh_iota.get() : e1, rel, img_rows ? img_rows : lv.ent_emb->p,
                       lv.rel_emb ? lv.rel_emb->p : nullptr,
                       dm.gen_conv ? nullptr : lv.conv1_weights->p, dm.gen_conv ? nullptr : lv.conv1_bias->p, img_rows ? B : (int64_t)dm.E, dm.R, d, r, dm.in_h, dm.in_w,
                       dm.stacked ? 1 : 0, C, dm.Ho, dm.Wo, T->img, ((gen || cat) && !genc) ? T->c.get() : nullptr, T->y, K_ps, kb_ps, dm.fh, dm.fw);
    double* const cs = bn1_fwd_sums();
    if (use_batch && det) det_col_sums(T->y, B * (int64_t)P, C, cs, DET_CS_WGS);
    else if (use_batch) {
      hipLaunchKernelGGL(k_tr_col_sums<false>, dim3(1024), dim3(256), 0, s, T->y, B * (int64_t)P, C, cs, TR_CS_SLOTS);
      hipLaunchKernelGGL(k_tr_fold_slots, dim3(1), dim3(256), 0, s, cs, 2 * C, TR_CS_SLOTS);
    }
  }
  void fwd_bn1() {
    double* const cs = bn1_fwd_sums();
    hipLaunchKernelGGL(k_tr_bn_finish, dim3((C + 63) / 64), dim3(64), 0, s, cs, C, (double)Bn * P, use_batch, tc.batch_norm_momentum, 1 | nomov,
                       lv.bn1.mov_mean, lv.bn1.mov_var, mean1, inv1);
    hipLaunchKernelGGL(k_tr_bn1_fwd, grid1d(nBF), dim3(256), 0, s, T->y, mean1, inv1, lv.bn1.gamma->p, lv.bn1.beta->p, C, nBF, tc.seed,
                       step, off_h, thr_h, ks_h, T->x, T->xmax);
    x_slots = cat ? nullptr : T->xmax.get();      // (concat_rel: the dense layer's input is another tensor)
    if (cat) hipLaunchKernelGGL(k_tr_concat, grid1d(B * F), dim3(256), 0, s, T->x, T->c, Fc, r, B * F, T->xc);
    xin = cat ? T->xc : T->x;
    dxin = cat ? T->dxc : T->dx;
  }
  // the dense layer (static, generated or looked up) + bias, dropout -> z1 [B, d]
  int fwd_dense() {
    int rc;
    for (int g : {0, 1}) chain_forward(g, nh);
    cw = nh ? T->chain[0].v[nh] : T->c;
    cbv = nh ? T->chain[1].v[nh] : T->c;
    W = gen ? lv.gen[0].proj[nh] : lv.fc_weights;
    const TrainParam* const blast = gen ? lv.gen[1].proj[nh] : nullptr;   // the last projection of the fc_bias generator
    if (lk) {
      // z0[b] = x[b] W[rel[b]]: one pass over the looked-up rows (B * F * d * 4 bytes), in TR_LK_NSL slices of F (deterministic partial sums)
      hipLaunchKernelGGL(k_tr_lookup_fwd, dim3((unsigned)B, TR_LK_NSL), dim3(256), sizeof(float) * (size_t)((F + TR_LK_NSL - 1) / TR_LK_NSL + 1), s,
                         T->x, W->p, rel, dm.R, F, d, TR_LK_NSL, B, T->dx /* scratch: [NSL][B][d], allocated for it */);
      hipLaunchKernelGGL(k_tr_lookup_post, grid1d(nBd), dim3(256), 0, s, T->dx, TR_LK_NSL, lv.fc_bias->p, rel, dm.R, d, nBd, tc.seed, step, off_o, thr_o,
                         ks_o, T->z1);
      return COPER_OK;
    }
    if (gen) {
      // T[rho][b][k] = sum_f x[b][f] P[rho][f][k] on the bf16 matrix cores with split operands (train_gemm_bf16.hip): x and P
      // are packed into fragment planes (P as rows (rho, k) with f contracted), one GEMM of [B] x [r*d] outputs
      const int64_t nrk = (int64_t)rc_w * d;
      if ((rc = tg_pack(h, xin, tg_idx(F), tg_idx(1), B, F, tg_rows_pad(B), false, T->pX, s, T->tg_scratch, nullptr, x_slots))) return rc;
      // the projection is an operand of two products, contracted over f here and over (rho, k) in dx: a training step packs BOTH
      // views from one read (tg_pack_both: 118 MB read once instead of twice, one launch instead of two)
      // (round 6 also ran this pack on a side stream beside the conv / Conv1BN launches in front of it: the stream takes the memory
      //  system, k_tr_bn1_fwd beside it 38 us for 9 -- 5 us gained, not kept)
      if (differentiates(kind) && (d & 3) == 0 && (((uintptr_t)W->p) & 15) == 0) {
        if ((rc = tg_pack_both(h, W->p, tg_idx(d), tg_idx2(d, F * (int64_t)d, 1), F, nrk, T->pP3, T->pP1, s, T->tg_scratch, w_slots))) return rc;
        p3_packed = true;
      } else if ((rc = tg_pack(h, W->p, tg_idx2(d, F * (int64_t)d, 1), tg_idx(d), nrk, F, tg_rows_pad(nrk), true, T->pP1, s, T->tg_scratch, nullptr, w_slots)))
        return rc;
      if ((rc = tg_gemm_split(h, T, s, T->pX, B, T->pP1, nrk, F, Tf, tg_idx(d), tg_idx2(d, nBd, 1), &t_slices))) return rc;
    } else if ((rc = tg_matmul(h, T, s, MmView{xin, tg_idx(F), tg_idx(1), false}, B, MmView{W->p, tg_idx(1), tg_idx(d), true}, d, F, T->z0,
                               tg_idx(d), tg_idx(1), nullptr, x_slots, w_slots)))      // z0[B,d] = x[B,F] W[F,d]: 8 output tiles, K = F cut into slices
      return rc;
    if (t_slices > 1) {
#define COPER_FC_SLICES(NS)                                                                                                                          \
    case NS:                                                                                                                                         \
      hipLaunchKernelGGL(k_tr_fc_post_slices<NS>, grid1d(nBd), dim3(256), 0, s, T->mmP, cw, rc_w, cbv, blast->p, rc_b, d, nBd, tc.seed,              \
                         step, off_o, thr_o, ks_o, Tf, T->z1);                                                                                              \
      break;
      switch (t_slices) {
        COPER_FC_SLICES(2) COPER_FC_SLICES(3) COPER_FC_SLICES(4) COPER_FC_SLICES(5) COPER_FC_SLICES(6) COPER_FC_SLICES(7) COPER_FC_SLICES(8)
      }
#undef COPER_FC_SLICES
    } else
      hipLaunchKernelGGL(k_tr_fc_post, grid1d(nBd), dim3(256), 0, s, gen ? Tf : T->z0.get(), gen ? nullptr : lv.fc_bias->p, cw, rc_w, cbv,
                         gen ? blast->p : nullptr, rc_b, d, nBd, tc.seed, step, off_o, thr_o, ks_o, T->z1);
    return COPER_OK;
  }

  // FCBN -> h [B, d], in two stages as Conv1BN
  double* fcbn_fwd_sums() const { return red.colsum_slice(CS_FCBN); }
  void fwd_fcbn_sums() {
    double* const cs = fcbn_fwd_sums();
    if (use_batch && det) det_col_sums(T->z1, B, d, cs, 64);
    else if (use_batch) hipLaunchKernelGGL(k_tr_col_sums<false>, dim3(64), dim3(256), 0, s, T->z1, B, d, cs, 1);
  }
  void fwd_fcbn_apply() {
    double* const cs = fcbn_fwd_sums();
    hipLaunchKernelGGL(k_tr_bn_finish, dim3((d + 63) / 64), dim3(64), 0, s, cs, d, (double)Bn, use_batch, tc.batch_norm_momentum, 0 | nomov,
                       lv.fcbn.mov_mean, lv.fcbn.mov_var, mean2, inv2);
    hipLaunchKernelGGL(k_tr_fcbn_fwd, grid1d(nBd), dim3(256), 0, s, T->z1, mean2, inv2, lv.fcbn.gamma->p, lv.fcbn.beta->p, d, nBd, T->hv);
  }
  // the scorer (sampled lookup, or 1-vs-all by GEMM) and the loss; what coper_train_forward asked to see
  int fwd_score_loss() {
    int rc;
    float* const ent = lv.ent_emb->p;
    const float* const pred_bias = lv.pred_bias->p;
    const float eps = tc.label_smoothing_epsilon, inv_E = (float)(1.0 / (double)dm.E);
    if (one_vs_all) {
      if ((size_t)(B * dm.E) > T->Sd.size()) {
        COPER_HIP_TRY(h, hipStreamSynchronize(s));
        if ((rc = T->Sd.alloc(h, (size_t)(B * dm.E), "training workspace"))) return rc;
      }
      // S[B,E] = h E^T
      if ((rc = tg_matmul(h, T, s, MmView{T->hv, tg_idx(d), tg_idx(1), false}, B, MmView{ent, tg_idx(d), tg_idx(1), false}, dm.E, d, T->Sd,
                          tg_idx(dm.E), tg_idx(1))))
        return rc;
      if (pred_out) hipLaunchKernelGGL(k_tr_add_bias_out, grid1d(B * dm.E), dim3(256), 0, s, T->Sd, pred_bias, dm.E, B * dm.E, pred_out);
      for (size_t i = 0; i < T->exp_cache.size(); ++i)      // (the loss kernel rewrites S in place: its power of two as an OUTPUT operand is gone)
        if (T->exp_cache[i].first == T->Sd) T->exp_cache[i].first = nullptr;
      if (det) {
        hipLaunchKernelGGL(k_tr_dense_loss<true>, dim3(2048), dim3(256), 0, s, T->Sd, pred_bias, labels, dm.E, B * dm.E, eps, inv_E, inv_BL, T->det_slab.get());
        det_fold(1, 2048, red.loss(), 1);
      } else
      hipLaunchKernelGGL(k_tr_dense_loss<false>, dim3(2048), dim3(256), 0, s, T->Sd, pred_bias, labels, dm.E, B * dm.E, eps, inv_E, inv_BL, red.loss());
    } else if (plan.shard) {
      // A sharded state (always deterministic): the SHARD forms score the entries (b, l) whose clamped id this handle holds
      // and write ds there only -- the same route by the same plan, so a shard that is the whole table leaves the whole-table step's bits.
      // (CURRENT, DESIGN 6.12: the same two kernels with the row load that forms a row as of the current update in registers)
      if (plan.dh == DhRoute::Fused) {
        const size_t lds_sf = plan.lds_fused;
        if (plan.current) {
          if (lds_sf > 64 * 1024)
            COPER_HIP_TRY(h, hipFuncSetAttribute((const void*)k_tr_score_loss_dh<true, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_sf));
          hipLaunchKernelGGL((k_tr_score_loss_dh<true, true, true>), dim3((unsigned)B), dim3(256), lds_sf, s, T->hv, ent, pred_bias, lookup, labels, dm.E, d,
                             (int)L, eps, inv_E, inv_BL, T->ds, T->dh, T->det_slab.get(), plan.lo, plan.n, row_tables(h, T), row_catch_up_args(T));
        } else {
        if (lds_sf > 64 * 1024)
          COPER_HIP_TRY(h, hipFuncSetAttribute((const void*)k_tr_score_loss_dh<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_sf));
        hipLaunchKernelGGL((k_tr_score_loss_dh<true, true>), dim3((unsigned)B), dim3(256), lds_sf, s, T->hv, ent, pred_bias, lookup, labels, dm.E, d,
                           (int)L, eps, inv_E, inv_BL, T->ds, T->dh, T->det_slab.get(), plan.lo, plan.n);
        }
      } else if (plan.current)
        hipLaunchKernelGGL((k_tr_score_loss<true, true, true>), dim3((unsigned)B), dim3(256), sizeof(float) * d, s, T->hv, ent, pred_bias, lookup, labels, dm.E,
                           d, L, eps, inv_E, inv_BL, T->ds, T->det_slab.get(), plan.lo, plan.n, row_tables(h, T), row_catch_up_args(T));
      else
        hipLaunchKernelGGL((k_tr_score_loss<true, true>), dim3((unsigned)B), dim3(256), sizeof(float) * d, s, T->hv, ent, pred_bias, lookup, labels, dm.E,
                           d, L, eps, inv_E, inv_BL, T->ds, T->det_slab.get(), plan.lo, plan.n);
    } else if (plan.dh == DhRoute::Fused) {
      const size_t lds_sf = plan.lds_fused;
      if (det)
        hipLaunchKernelGGL(k_tr_score_loss_dh<true>, dim3((unsigned)B), dim3(256), lds_sf, s, T->hv, ent,
                           pred_bias, lookup, labels, dm.E, d, (int)L, eps, inv_E, inv_BL, T->ds, T->dh, T->det_slab.get());
      else
      hipLaunchKernelGGL(k_tr_score_loss_dh<false>, dim3((unsigned)B), dim3(256),
                         lds_sf, s, T->hv, ent,
                         pred_bias, lookup, labels, dm.E, d, (int)L, eps, inv_E, inv_BL, T->ds, T->dh, red.loss());
    } else if (det) {
      hipLaunchKernelGGL(k_tr_score_loss<true>, dim3((unsigned)B), dim3(256), sizeof(float) * d, s, T->hv, ent, pred_bias, lookup, labels, dm.E, d, L,
                         eps, inv_E, inv_BL, T->ds, T->det_slab.get());
    } else {
      hipLaunchKernelGGL(k_tr_score_loss<false>, dim3((unsigned)B), dim3(256), sizeof(float) * d, s, T->hv, ent, pred_bias, lookup, labels, dm.E, d, L,
                         eps, inv_E, inv_BL, T->ds, red.loss());
    }
    if (det && !one_vs_all) det_fold(1, B, red.loss(), 1);      // (the B workgroups' loss shares, in sample order)
    if (loss_out) hipLaunchKernelGGL(k_tr_store_loss, dim3(1), dim3(1), 0, s, red.loss(), 1.0 / ((double)B * (double)L), loss_out);
    if (!one_vs_all && pred_out && plan.shard) {      // (coper_train_shard_forward_lookup's pred_part: the owned entries, +0.f elsewhere)
      if (plan.current)
        hipLaunchKernelGGL(k_tr_scores_out_shard<true>, dim3((unsigned)B), dim3(256), 0, s, T->hv, ent, pred_bias, lookup, dm.E, d, L, pred_out, plan.lo,
                           plan.n, row_tables(h, T), row_catch_up_args(T));
      else
        hipLaunchKernelGGL(k_tr_scores_out_shard<false>, dim3((unsigned)B), dim3(256), 0, s, T->hv, ent, pred_bias, lookup, dm.E, d, L, pred_out, plan.lo,
                           plan.n, RowTables(), RowCatchUp());
    } else if (!one_vs_all && pred_out)
      hipLaunchKernelGGL(k_tr_scores_out, dim3((unsigned)B), dim3(256), 0, s, T->hv, ent, pred_bias, lookup, dm.E, d, L, pred_out);
    if (h_out) COPER_HIP_TRY(h, hipMemcpyAsync(h_out, T->hv, sizeof(float) * (size_t)nBd, hipMemcpyDeviceToDevice, s));
    return COPER_OK;
  }
  // The 1-vs-all scorer from sparse labels, forward AND backward, in chunks of entity columns [c0, c0 + w): the scorer is separable by
  // column, so per chunk S_c = h E_c^T, the loss kernel (labels from membership in the row's id list; S_c becomes d(loss)/d(logits)),
  // dbias[c0 : c0 + w] = column sums, dE[c0 : c0 + w] = S_c^T h, and the chunk's share of dh = S_c E_c -- the first chunk's into dh, a
  // later one's into dhc and added behind it, in chunk order.  Neither the labels nor the logits exist as [B, |E|].  One chunk: the
  // launches of fwd_score_loss + bwd_scorer with k_tr_csr_loss for k_tr_dense_loss.
  // Operand exponents: h keeps one power of two for the whole step (one tensor: tg_matmul's cache); a chunk of the table and a chunk
  // of S get their own -- per CHUNK, not per tensor: a chunk is packed when it is used, nothing scans the whole table first, and a
  // chunk's own maximum wastes no bits on a larger row elsewhere.  Their cache words are handed back behind every chunk.
  int score_csr() {
    int rc;
    float* const ent = lv.ent_emb->p;
    const float* const pred_bias = lv.pred_bias->p;
    float *const dE = lv.ent_emb->g, *const dbias = lv.pred_bias->g;
    const float eps = tc.label_smoothing_epsilon, inv_E = (float)(1.0 / (double)dm.E);
    // (sharded: E is the handle's own rows -- local columns c0, entity sh_lo + c0; inv_E above stays that of the whole table)
    const int64_t E = plan.n, sh_lo = plan.lo, cw = ova_chunk(B, E, tc.one_vs_all_chunk);
    const bool diff = differentiates(kind);
    if ((size_t)(B * cw) > T->Sd.size() || (diff && cw < E && (size_t)nBd > T->dhc.size())) {
      COPER_HIP_TRY(h, hipStreamSynchronize(s));
      if ((rc = T->Sd.ensure(h, (size_t)(B * cw), "training workspace")) || (diff && cw < E && (rc = T->dhc.ensure(h, (size_t)nBd, "training workspace"))))
        return rc;
    }
    const size_t cached = T->exp_cache.size();
    for (int64_t c0 = 0; c0 < E; c0 += cw) {
      const int64_t w = E - c0 < cw ? E - c0 : cw;
      float* const ent_c = ent + c0 * d;
      if ((rc = tg_matmul(h, T, s, MmView{T->hv, tg_idx(d), tg_idx(1), false}, B, MmView{ent_c, tg_idx(d), tg_idx(1), false}, w, d, T->Sd,
                          tg_idx(w), tg_idx(1))))
        return rc;
      if (pred_out) hipLaunchKernelGGL(k_tr_add_bias_out_cols, grid1d(B * w), dim3(256), 0, s, T->Sd, pred_bias + c0, w, B * w, E, pred_out + c0);      // (sharded: coper_train_shard_forward_csr's pred_local, row stride n_local)
      const int64_t n_stretch = (w + TR_CSR_STRETCH - 1) / TR_CSR_STRETCH;
      const int vec = (w & 3) == 0 && (((uintptr_t)T->Sd.get() | (uintptr_t)(pred_bias + c0)) & 15) == 0;
      if (det) {      // (a later chunk's shares onto the earlier chunks' sum: chunk order)
        hipLaunchKernelGGL(k_tr_csr_loss<true>, dim3((unsigned)(B * n_stretch)), dim3(256), 0, s, T->Sd, pred_bias + c0, csr.indptr, csr.idx, csr.row,
                           csr.n_rows, sh_lo + c0, w, n_stretch, vec, eps, inv_E, inv_BL, T->det_slab.get());
        det_fold(1, B * n_stretch, red.loss(), 1);
      } else
      hipLaunchKernelGGL(k_tr_csr_loss<false>, dim3((unsigned)(B * n_stretch)), dim3(256), 0, s, T->Sd, pred_bias + c0, csr.indptr, csr.idx, csr.row,
                         csr.n_rows, sh_lo + c0, w, n_stretch, vec, eps, inv_E, inv_BL, red.loss());
      if (diff) {
        hipLaunchKernelGGL(k_tr_col_sum_f32, grid1d(w), dim3(256), 0, s, T->Sd, B, w, dbias + c0);
        if ((rc = tg_matmul(h, T, s, MmView{T->Sd, tg_idx(1), tg_idx(w), true}, w, MmView{T->hv, tg_idx(1), tg_idx(d), true}, d, B, dE + c0 * d,
                            tg_idx(d), tg_idx(1))))
          return rc;
        float* const share = c0 ? T->dhc.get() : T->dh.get();
        if ((rc = tg_matmul(h, T, s, MmView{T->Sd, tg_idx(w), tg_idx(1), false}, B, MmView{ent_c, tg_idx(1), tg_idx(d), true}, d, w, share,
                            tg_idx(d), tg_idx(1))))
          return rc;
        if (c0) hipLaunchKernelGGL(k_tr_add_to, grid1d(nBd), dim3(256), 0, s, T->dh, T->dhc, nBd);
      }
      // (h, packed first, stays; the chunk's S and table rows are other data at the next chunk, S at the same address)
      if (T->exp_cache.size() > cached + 1) T->exp_cache.resize(cached + 1);
    }
    if (loss_out) hipLaunchKernelGGL(k_tr_store_loss, dim3(1), dim3(1), 0, s, red.loss(), 1.0 / ((double)B * (double)L), loss_out);
    if (h_out) COPER_HIP_TRY(h, hipMemcpyAsync(h_out, T->hv, sizeof(float) * (size_t)nBd, hipMemcpyDeviceToDevice, s));
    return COPER_OK;
  }
  // ---- backward
  // d(loss)/d(logits) -> dh [B, d], d(pred_bias), d(ent_emb), by the plan's routes: a GEMM on the dense S where B * |E| is small, sorted
  // segments (ordered rows; a sharded state, over its own rows), else float atomics.
  // Behind the caller's fork (scorer_bwd_on_side) S, dbias and dE = S^T h (~70 us that need ds and h only) run on side[0] beside the dense
  // layer's backward: tg_matmul packs into a second pair of plane sets there, dE needs no K slices (the partial-sum pool is the dx product's)
  int bwd_scorer() {
    int rc;
    float* const ent = lv.ent_emb->p;
    float *const dE = lv.ent_emb->g, *const dbias = lv.pred_bias->g;
    switch (plan.table) {
    case TableGrad::CsrChunks: return COPER_OK;      // (score_csr: the backward ran chunk by chunk)
    case TableGrad::OvaGemm:
      hipLaunchKernelGGL(k_tr_col_sum_f32, grid1d(dm.E), dim3(256), 0, s, T->Sd, B, dm.E, dbias);
      // dE[E,d] = S^T h
      if ((rc = tg_matmul(h, T, s, MmView{T->Sd, tg_idx(1), tg_idx(dm.E), true}, dm.E, MmView{T->hv, tg_idx(1), tg_idx(d), true}, d, B, dE,
                          tg_idx(d), tg_idx(1))))
        return rc;
      // dh[B,d] = S E: 8 output tiles, K = |E| cut into slices
      return tg_matmul(h, T, s, MmView{T->Sd, tg_idx(dm.E), tg_idx(1), false}, B, MmView{ent, tg_idx(1), tg_idx(d), true}, d, dm.E, T->dh,
                       tg_idx(d), tg_idx(1));
    case TableGrad::Atomics:
      hipLaunchKernelGGL(k_tr_score_bwd<true>, dim3((unsigned)B), dim3(256), 0, s, T->hv, ent, lookup, T->ds, dm.E, d, L, T->dh, dE, dbias);
      return COPER_OK;
    case TableGrad::Ordered: {
      // one writer per named row, its addends in ascending (b, l): `=` onto the zeroed rows (the conv backward adds the e1 rows behind it).
      // The sort runs over all B (L + 1) ids (a segment's addends and their order do not depend on what else is sorted); the reduce
      // skips the segments outside the plan's rows.
      if (!ord_vals) order_rows(T->ord_list.get(), T->ord_count.get(), nullptr);
      const int vec = (d & 3) == 0 && (((uintptr_t)T->hv.get() | (uintptr_t)dE) & 15) == 0;
      hipLaunchKernelGGL(k_ord_reduce, rows_grid(std::min<int64_t>(B * (L + 1), dm.E)), dim3(256), 0, s, ord_rows, (const int32_t*)T->ord_seg.get(),
                         ord_rows_count, ord_vals, (const float*)T->ds.get(), (const float*)T->hv.get(), L, B * L, d, vec, plan.lo, plan.n, dE, dbias);
      prof_count(h, "train.order.reduce");
      break;
    }
    case TableGrad::DenseS: {
      hipStream_t const q = sj.on[SJ_SCORER_BWD] >= 0 ? T->side[sj.on[SJ_SCORER_BWD]] : s;
      const size_t lds_s = sizeof(float) * (size_t)(dm.E < TR_S_CHUNK ? dm.E : TR_S_CHUNK);
      // (the kernel also holds 16 bytes of static LDS: asking for the whole 160 KB as dynamic is refused, and so is the launch after it)
      if (!det && lds_s > 64 * 1024) COPER_HIP_TRY(h, hipFuncSetAttribute((const void*)k_tr_build_S, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_s));
      if (det) {      // duplicate ids of a row in ascending l; dbias[c] = the column sum of S in ascending b
        hipLaunchKernelGGL(k_tr_build_S_det, dim3((unsigned)B), dim3(256), 0, q, lookup, T->ds, dm.E, L, T->Sd, T->smax);
        det_col_sum_f32(T->Sd, dm.E, dbias, q);
      } else {
        hipLaunchKernelGGL(k_tr_build_S, dim3((unsigned)B), dim3(256), lds_s, q, lookup, T->ds, dm.E, L, T->Sd, T->smax);
        hipLaunchKernelGGL(k_tr_col_sums_add<false>, dim3((unsigned)((dm.E + 255) / 256), (unsigned)((B + 63) / 64)), dim3(256), 0, q, T->Sd, B, dm.E, dbias);
      }
      // dE[E,d] = S^T h  (overwrites the zeroed gradient; the e1-row contributions are added after it)
      if ((rc = tg_matmul(h, T, q, MmView{T->Sd, tg_idx(1), tg_idx(dm.E), true}, dm.E, MmView{T->hv, tg_idx(1), tg_idx(d), true}, d, B, dE,
                          tg_idx(d), tg_idx(1), nullptr, T->smax)))
        return rc;
      break;
    }
    }
    // dh behind the segments or the dense S, on the step's own stream and in its own fixed order: by the gather (a [d,B] = [d,|E|] x
    // [|E|,B] GEMM has 8 output tiles and a long K: slower than the gather).  The SHARD forms take the row range: an entry of another
    // shard is a (0, 0) addend with nothing loaded.
    if (plan.dh == DhRoute::Gather4) {
      const size_t lds_g = sizeof(float4) * (size_t)(256 / (d >> 2)) * (d >> 2);
      if (plan.shard) hipLaunchKernelGGL(k_tr_dh_gather4<true>, dim3((unsigned)B), dim3(256), lds_g, s, ent, lookup, T->ds, dm.E, d, L, T->dh, plan.lo, plan.n);
      else hipLaunchKernelGGL(k_tr_dh_gather4<>, dim3((unsigned)B), dim3(256), lds_g, s, ent, lookup, T->ds, dm.E, d, L, T->dh);
    } else if (plan.dh == DhRoute::ScoreBwd) {
      if (plan.shard)
        hipLaunchKernelGGL((k_tr_score_bwd<false, true>), dim3((unsigned)B), dim3(256), 0, s, T->hv, ent, lookup, T->ds, dm.E, d, L, T->dh,
                           (float*)nullptr, (float*)nullptr, plan.lo, plan.n);
      else hipLaunchKernelGGL(k_tr_score_bwd<false>, dim3((unsigned)B), dim3(256), 0, s, T->hv, ent, lookup, T->ds, dm.E, d, L, T->dh, nullptr, nullptr);
    }      // (DhRoute::Fused: dh came with the scores, k_tr_score_loss_dh)
    return COPER_OK;
  }

  // FCBN and ReLU backward -> dz: one launch, all of it in the second stage.  A step open across exchanges (sync_sums) takes two, around
  // the exchange: this rank's sums into their half of sync_sums | dz from the sums of the whole batch, the gamma / beta gradients from
  // the rank's own
  double* fcbn_bwd_sums() const { return sync_sums + (size_t)2 * T->mx; }
  void bwd_fcbn_sums() {
    if (!sync_sums) return;
    hipLaunchKernelGGL(k_tr_fcbn_bwd_sums, dim3((unsigned)d), dim3(256), 0, s, T->z1, T->hv, T->dh, mean2, inv2, B, d, fcbn_bwd_sums());
  }
  void bwd_fcbn_apply() {
    if (!sync_sums)
      hipLaunchKernelGGL(k_tr_fcbn_bwd, dim3((unsigned)d), dim3(256), 0, s, T->z1, T->hv, T->dh, mean2, inv2, lv.fcbn.gamma->p, B, d,
                         use_batch, lv.fcbn.gamma->g, lv.fcbn.beta->g, T->dz);
    else
      hipLaunchKernelGGL(k_tr_fcbn_bwd_apply, dim3((unsigned)d), dim3(256), 0, s, T->z1, T->hv, T->dh, mean2, inv2, lv.fcbn.gamma->p, B, d, (double)Bn,
                         (const double*)sync_sums, (const double*)fcbn_bwd_sums(), lv.fcbn.gamma->g, lv.fcbn.beta->g, T->dz);
  }
  // dT[rho][b,:] = cw[b,rho] dz[b,:];  dP[rho][f][k] = sum_b x[b][f] dT[rho][b][k]  and
  // dx[b][f] = sum_(rho,k) dT[rho][b][k] P[rho][f][k]: two split-bf16 GEMMs, the [B, r*F] intermediate dz P2^T is never formed
  int bwd_dense_generated() {
    int rc;
    const int64_t nrk = (int64_t)rc_w * d;
    hipLaunchKernelGGL(k_tr_scale_rows, grid1d(nBd), dim3(256), 0, s, T->dz, cw, rc_w, d, nBd, dTf, T->dtmax);
    // (x and the projection were packed for the forward pass: the same tensors, the same powers of two -- no second reduction)
    if ((rc = tg_pack(h, xin, tg_idx(1), tg_idx(F), F, B, tg_rows_pad(F), true, T->pXt, s, T->tg_scratch, T->pX.exp))) return rc;
    if ((rc = tg_pack(h, dTf, tg_idx2(d, nBd, 1), tg_idx(d), nrk, B, tg_rows_pad(nrk), true, T->pTn, s, T->tg_scratch, nullptr, T->dtmax))) return rc;
    if ((rc = tg_pack(h, dTf, tg_idx(d), tg_idx2(d, nBd, 1), B, nrk, tg_rows_pad(B), false, T->pTb, s, T->tg_scratch, T->pTn.exp))) return rc;
    if (!p3_packed && (rc = tg_pack(h, W->p, tg_idx(d), tg_idx2(d, F * (int64_t)d, 1), F, nrk, tg_rows_pad(F), false, T->pP3, s, T->tg_scratch, T->pP1.exp))) return rc;
    // (the K slices of dx stay in the partial-sum pool for k_tr_bn1_bwd_sums when dx IS the conv features' gradient: no concat_rel)
    if ((rc = tg_gemm_split(h, T, s, T->pTb, B, T->pP3, F, nrk, dxin, tg_idx(F), tg_idx(1), (cat || det) ? nullptr : &dx_slices))) return rc;
    if ((rc = bwd_dense_dP())) return rc;
    hipLaunchKernelGGL(k_tr_dc_from_partials, dim3((unsigned)((B * rc_w + 3) / 4)), dim3(256), 0, s, T->dz, Tf, B, rc_w, d, T->chain[0].dv[nh].get());
    return COPER_OK;
  }
  // the dP product's result is read by the optimizer only: BEHIND the dx product, on the second side stream, beside the dozen short
  // launches between here and the optimizer (slice sum, Conv1BN and conv backward, the generators' chains).  (Beside the dx product
  // itself the two took 211 us for 100 + 84: a SIMD holds one wave of either.)
  int bwd_dense_dP() {
    if (two_streams) sj.fork(SJ_DP, 1);
    sumsq_done = det ? nullptr : W;   // the GEMM adds |dP|^2 to the global-norm accumulator as it stores (deterministic mode: k_tr_sumsq does, as for every leaf)
    return tg_gemm_nt(h, T->pXt, F, T->pTn, (int64_t)rc_w * d, B, W->g, tg_idx(d), tg_idx2(d, F * (int64_t)d, 1), two_streams ? T->side[1] : s, 1,
                      nullptr, det ? nullptr : red.sumsq_slots());
  }

  int bwd_dense() {
    int rc;
    if (lk) {
      if (det) {
        hipLaunchKernelGGL(k_tr_lookup_post_bwd<true>, grid1d(nBd), dim3(256), 0, s, T->dz, rel, dm.R, d, nBd, tc.seed, step, off_o, thr_o, ks_o, lv.fc_bias->g);
        det_rows_by_key(T->dz, d, 0, d, rel, dm.R, lv.fc_bias->g);
      } else
      hipLaunchKernelGGL(k_tr_lookup_post_bwd<false>, grid1d(nBd), dim3(256), 0, s, T->dz, rel, dm.R, d, nBd, tc.seed, step, off_o, thr_o, ks_o, lv.fc_bias->g);
      const int rows_per_wg = 32;
      hipLaunchKernelGGL(k_tr_lookup_dW, dim3((unsigned)((F + rows_per_wg - 1) / rows_per_wg), (unsigned)dm.R), dim3(256), 0, s, T->x, T->dz, det ? T->det_perm.get() : h->grouping().perm,
                         h->grouping().rel_offset, h->grouping().rel_count, F, d, rows_per_wg, W->g);
      hipLaunchKernelGGL(k_tr_lookup_dx, dim3((unsigned)((F + 63) / 64), (unsigned)B), dim3(256), sizeof(float) * d, s, T->dz, W->p, rel, dm.R, F, d, T->dx);
      return COPER_OK;
    }
    // gradients of the two contexts: dcw [B, rc_w] (k_tr_dc_from_partials) and dcb [B, rc_b] (k_tr_fc_post_bwd)
    const TrainParam* const blast = gen ? lv.gen[1].proj[nh] : nullptr;
    if (det) {
      hipLaunchKernelGGL(k_tr_fc_post_bwd<true>, dim3((unsigned)B), dim3(256), sizeof(float) * d, s, T->dz, cbv, gen ? blast->p : nullptr, rc_b, d, tc.seed,
                         step, off_o, thr_o, ks_o, gen ? nullptr : lv.fc_bias->g.get(), gen ? blast->g.get() : nullptr,
                         gen ? T->chain[1].dv[nh].get() : nullptr);
      if (!gen) det_col_sum_f32(T->dz, d, lv.fc_bias->g.get(), s);
    } else
    hipLaunchKernelGGL(k_tr_fc_post_bwd<false>, dim3((unsigned)B), dim3(256), sizeof(float) * d, s, T->dz, cbv, gen ? blast->p : nullptr, rc_b, d, tc.seed,
                       step, off_o, thr_o, ks_o, gen ? nullptr : lv.fc_bias->g.get(), gen ? blast->g.get() : nullptr,
                       gen ? T->chain[1].dv[nh].get() : nullptr);
    if (gen) {     // (into the zeroed gradient: 8 atomics per address; deterministic mode: one thread per entry, ascending b)
      if (det) {
        const unsigned nz = (unsigned)((B + 63) / 64);
        hipLaunchKernelGGL(k_tr_wsum_rows_add<true>, dim3((unsigned)rc_b, nz), dim3(256), 0, s, cbv, T->dz, B, rc_b, d, (float*)T->det_slab.get());
        hipLaunchKernelGGL(k_tr_fold_f32_det, grid1d((int64_t)rc_b * d), dim3(256), 0, s, (const float*)T->det_slab.get(), (int64_t)rc_b * d, (int)nz, blast->g.get());
      } else
      hipLaunchKernelGGL(k_tr_wsum_rows_add<false>, dim3((unsigned)rc_b, (unsigned)((B + 63) / 64)), dim3(256), 0, s, cbv, T->dz, B, rc_b, d, blast->g);
      if ((rc = bwd_dense_generated())) return rc;
    } else {
      // static dense layer (plain ConvE): dW[F,d] = x^T dz and dx[B,F] = dz W^T
      if ((rc = tg_matmul(h, T, s, MmView{xin, tg_idx(1), tg_idx(F), true}, F, MmView{T->dz, tg_idx(1), tg_idx(d), true}, d, B, W->g, tg_idx(d),
                          tg_idx(1), det ? nullptr : red.sumsq_slots())))
        return rc;
      sumsq_done = det ? nullptr : W;
      if ((rc = tg_matmul(h, T, s, MmView{T->dz, tg_idx(d), tg_idx(1), false}, B, MmView{W->p, tg_idx(d), tg_idx(1), false}, F, d, dxin,
                          tg_idx(F), tg_idx(1))))
        return rc;
    }
    if (cat && det) {
      hipLaunchKernelGGL(k_tr_split<true>, grid1d(B * F), dim3(256), 0, s, T->dxc, rel, dm.R, Fc, r, B * F, T->dx, lv.rel_emb->g);
      det_rows_by_key(T->dxc, F, Fc, r, rel, dm.R, lv.rel_emb->g);
    } else if (cat) hipLaunchKernelGGL(k_tr_split<false>, grid1d(B * F), dim3(256), 0, s, T->dxc, rel, dm.R, Fc, r, B * F, T->dx, lv.rel_emb->g);
    return COPER_OK;
  }
  // back through a generator chain to the relation rows: dv[nhx] -> dv[0]
  void chain_backward(int g, int nhx) {
    TrainState::Chain& ch = T->chain[g];
    for (int i = nhx - 1; i >= 0; --i) {
      const int ni = ch.dims[i], nj = ch.dims[i + 1];
      const TrainLeaves::Bn& b = lv.gen[g].bn[i];
      const TrainParam* const proj = lv.gen[g].proj[i];
      const int64_t tot = B * nj;
      hipLaunchKernelGGL(k_tr_chain_drop_bwd, grid1d(tot), dim3(256), 0, s, ch.dv[i + 1], tot, tc.seed, step, drop_off(nj), dropout_stage_chain(g, i), thr_c, ks_c,
                         ch.du[i]);
      // ReLU (+ BN) backward, in place on du; BN gamma / beta gradients
      const bool cb = dm.ctx_bn;
      hipLaunchKernelGGL(k_tr_fcbn_bwd, dim3((unsigned)nj), dim3(256), 0, s, ch.u[i], ch.a[i], ch.du[i], cb ? ch.st[i].get() : nullptr,
                         cb ? ch.st[i] + nj : nullptr, cb ? b.gamma->p : nullptr, B, nj, cb ? use_batch : 0, cb ? b.gamma->g.get() : nullptr,
                         cb ? b.beta->g.get() : nullptr, ch.du[i]);
      hipLaunchKernelGGL(k_tr_small_mm_tn, grid1d((int64_t)ni * nj), dim3(256), 0, s, i ? ch.v[i] : T->c, ch.du[i], B, ni, nj, proj->g);
      hipLaunchKernelGGL(k_tr_small_mm_nt, grid1d(B * ni), dim3(256), 0, s, ch.du[i], proj->p, B, ni, nj, 0, ch.dv[i]);
    }
  }
  // dropout, ReLU and Conv1BN backward on dx (the K slices of the dx product, where it left them, are added on the way)
  // In two stages: this call's sums | the apply.
  double* bn1_bwd_sums() const { return red.cs_slots(CSS_BN1_BWD); }
  void bwd_bn1_sums() {
    double* const colsum = bn1_bwd_sums();
    const dim3 g1((unsigned)((nBF + 255) / 256 < 2048 ? (nBF + 255) / 256 : 2048));
    if (det) {      // (dx is whole: the dx product kept no K slices in this mode)
      hipLaunchKernelGGL(k_tr_bn1_bwd_sums_det, dim3(DET_CS_WGS), dim3(256), 0, s, T->dx, T->y, mean1, inv1, lv.bn1.gamma->p, lv.bn1.beta->p, C,
                         B * (int64_t)P, tc.seed, step, off_h, thr_h, ks_h, T->det_slab.get());
      det_fold(2 * C, DET_CS_WGS, colsum, 0);
    } else {
#define COPER_BN1_SUMS(NS)                                                                                                                           \
    case NS:                                                                                                                                         \
      hipLaunchKernelGGL(k_tr_bn1_bwd_sums<NS>, g1, dim3(256), 0, s, T->dx, NS ? T->mmP : nullptr, T->y, mean1, inv1,                                \
                         lv.bn1.gamma->p, lv.bn1.beta->p, C, nBF, tc.seed, step, off_h, thr_h, ks_h, colsum, TR_CS_SLOTS);                                  \
      break;
    switch (dx_slices > 1 ? dx_slices : 0) {
      COPER_BN1_SUMS(0) COPER_BN1_SUMS(2) COPER_BN1_SUMS(3) COPER_BN1_SUMS(4) COPER_BN1_SUMS(5) COPER_BN1_SUMS(6) COPER_BN1_SUMS(7) COPER_BN1_SUMS(8)
    }
#undef COPER_BN1_SUMS
    hipLaunchKernelGGL(k_tr_fold_slots, dim3(1), dim3(256), 0, s, colsum, 2 * C, TR_CS_SLOTS);
    }
  }
  // all: the sums over the positions the statistics were taken over (this call's own, or the whole batch's of a synchronised step)
  void bwd_bn1_apply() {
    const double* const all = sync_sums ? sync_sums : bn1_bwd_sums();
    hipLaunchKernelGGL(k_tr_bn1_bwd_apply, grid1d(nBF), dim3(256), 0, s, T->dx, T->y, mean1, inv1, lv.bn1.gamma->p, all, (const double*)bn1_bwd_sums(), C, nBF,
                       (double)Bn * P, use_batch, lv.bn1.gamma->g, lv.bn1.beta->g);
  }
  // the conv backward: adds the e1 rows to dE (so the scorer's dE is joined in front of it), leaves per-query filter gradients
  void bwd_conv() {
    const size_t lds_cb = sizeof(float) * (size_t)(isz + (size_t)P * (C + 1) + NT * C);
    if (!det && lds_cb > 64 * 1024) (void)hipFuncSetAttribute((const void*)k_tr_conv_bwd<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    sj.join(SJ_SCORER_BWD);      // (dE = S^T h is stored: the conv backward adds the e1 rows to it)
    if (det) {
      // d(img) per query, then one writer per embedding row: the e1 rows onto what the scorer's GEMM stored in dE, ascending b
      if (lds_cb > 64 * 1024) (void)hipFuncSetAttribute((const void*)k_tr_conv_bwd<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      hipLaunchKernelGGL(k_tr_conv_bwd<true>, dim3((unsigned)B), dim3(256), lds_cb, s, T->dx, T->img, dm.gen_conv ? nullptr : lv.conv1_weights->p, e1, rel,
                         dm.E, dm.R, d, r, dm.in_h, dm.in_w, dm.stacked ? 1 : 0, C, dm.Ho, dm.Wo, T->dimg.get(),
                         (float*)nullptr, K_ps, T->dKs, T->dkbs, dm.fh, dm.fw);
      if (plan.shard) {      // the owned e1 rows alone; a row of another shard is that rank's to write
        float* const dE = lv.ent_emb->g;
        const int vec = (d & 3) == 0 && (isz & 3) == 0 && (((uintptr_t)T->dimg.get() | (uintptr_t)dE) & 15) == 0;
        hipLaunchKernelGGL(k_shard_rows_by_key, dim3((unsigned)B), dim3(256), 0, s, (const float*)T->dimg.get(), (int64_t)isz, (int64_t)0, d, e1, (int64_t)dm.E, B,
                           plan.lo, plan.n, vec, dE);
      } else
      det_rows_by_key(T->dimg, isz, 0, d, e1, dm.E, lv.ent_emb->g);
      if (dm.stacked) det_rows_by_key(T->dimg, isz, d, r, rel, dm.R, lv.rel_emb->g);
      return;
    }
    hipLaunchKernelGGL(k_tr_conv_bwd<false>, dim3((unsigned)B), dim3(256), lds_cb, s, T->dx, T->img, dm.gen_conv ? nullptr : lv.conv1_weights->p, e1, rel,
                       dm.E, dm.R, d, r, dm.in_h, dm.in_w, dm.stacked ? 1 : 0, C, dm.Ho, dm.Wo, lv.ent_emb->g,
                       lv.rel_emb ? lv.rel_emb->g.get() : nullptr, K_ps, T->dKs, T->dkbs, dm.fh, dm.fw);
  }
  // per-query filter gradients -> static filters, generators' last projections and chains, or table rows; every chain's dv[0] -> relation rows
  void bwd_conv_filters() {
    if (!dm.gen_conv && det) {
      det_col_sum_f32(T->dKs, (int64_t)NT * C, lv.conv1_weights->g.get(), s);
      det_col_sum_f32(T->dkbs, C, lv.conv1_bias->g.get(), s);
    } else
    if (!dm.gen_conv) {      // static filters: their gradients are the column sums of the per-query ones (added to the zeroed gradients)
      hipLaunchKernelGGL(k_tr_col_sums_add<false>, dim3((unsigned)((NT * C + 255) / 256), (unsigned)((B + 63) / 64)), dim3(256), 0, s, T->dKs, B,
                         (int64_t)NT * C, lv.conv1_weights->g);
      hipLaunchKernelGGL(k_tr_col_sums_add<false>, dim3(1, (unsigned)((B + 63) / 64)), dim3(256), 0, s, T->dkbs, B, (int64_t)C, lv.conv1_bias->g);
    }
    if (genc) {
      const TrainParam *const cwlast = lv.gen[2].proj[nhc], *const cblast = lv.gen[3].proj[nhc];
      hipLaunchKernelGGL(k_tr_small_mm_tn, grid1d((int64_t)rc_cw * NT * C), dim3(256), 0, s, ccw, T->dKs, B, rc_cw, NT * C, cwlast->g);
      hipLaunchKernelGGL(k_tr_small_mm_nt, grid1d(B * rc_cw), dim3(256), 0, s, T->dKs, cwlast->p, B, rc_cw, NT * C, 0, T->chain[2].dv[nhc]);
      hipLaunchKernelGGL(k_tr_small_mm_tn, grid1d((int64_t)rc_cb * C), dim3(256), 0, s, ccb, T->dkbs, B, rc_cb, C, cblast->g);
      hipLaunchKernelGGL(k_tr_small_mm_nt, grid1d(B * rc_cb), dim3(256), 0, s, T->dkbs, cblast->p, B, rc_cb, C, 0, T->chain[3].dv[nhc]);
      for (int g : {2, 3}) chain_backward(g, nhc);
    } else if (lkc && det) {
      det_rows_by_key(T->dKs, (int64_t)NT * C, 0, NT * C, rel, dm.R, lv.conv1_weights->g);
      det_rows_by_key(T->dkbs, C, 0, C, rel, dm.R, lv.conv1_bias->g);
    } else if (lkc) {
      // table rows: d(conv1_weights)[rel[b]] += dK[b] (the table gradients were zeroed above)
      hipLaunchKernelGGL(k_tr_scatter_rows, grid1d(B * NT * C), dim3(256), 0, s, T->dKs, rel, dm.R, NT * C, B * NT * C, lv.conv1_weights->g);
      hipLaunchKernelGGL(k_tr_scatter_rows, grid1d(B * C), dim3(256), 0, s, T->dkbs, rel, dm.R, C, B * C, lv.conv1_bias->g);
    }
    for (int g = 0; g < 4; ++g)
      if (!(g < 2 ? gen : genc)) continue;
      else if (det) det_rows_by_key(T->chain[g].dv[0], r, 0, r, rel, dm.R, lv.rel_emb->g);      // (chain after chain, each onto the sum so far)
      else
        hipLaunchKernelGGL(k_tr_scatter_rows, grid1d(B * r), dim3(256), 0, s, T->chain[g].dv[0], rel, dm.R, r, B * r, lv.rel_emb->g);
  }
  // ---- the schedule: stages [from, to) in order, to the first failure.  The only caller of the stage functions above.
  int run(Stage from, Stage to) {
    int rc = COPER_OK;
    for (int i = (int)from; i < (int)to && !rc; ++i) switch ((Stage)i) {
      case Stage::ConvFilters: fwd_conv_filters(); break;
      case Stage::Bn1Sums: fwd_conv_sums(); break;
      case Stage::Bn1: fwd_bn1(); break;
      case Stage::Dense: rc = fwd_dense(); break;
      case Stage::FcbnSums: fwd_fcbn_sums(); break;
      case Stage::Fcbn: fwd_fcbn_apply(); break;
      case Stage::Score: rc = csr.indptr ? score_csr() : fwd_score_loss(); break;      // (score_csr: the scorer's backward too, chunk by chunk)
      case Stage::ScorerBwd:      // (nothing left to do behind score_csr; the fork is joined in front of the conv backward, or by the driver)
        if (scorer_bwd_on_side()) sj.fork(SJ_SCORER_BWD, 0);
        rc = bwd_scorer();
        break;
      case Stage::FcbnBwdSums: bwd_fcbn_sums(); break;
      case Stage::FcbnBwd: bwd_fcbn_apply(); break;
      case Stage::DenseBwd: rc = bwd_dense(); break;      // (generated: forks SJ_DP in front of the dP product, bwd_dense_dP)
      case Stage::ChainsBwd: if (gen) { chain_backward(0, nh); chain_backward(1, nh); } break;
      case Stage::Bn1BwdSums: bwd_bn1_sums(); break;
      case Stage::Bn1Bwd: bwd_bn1_apply(); break;
      case Stage::ConvBwd: bwd_conv(); break;             // (joins SJ_SCORER_BWD in front of its launch)
      case Stage::ConvFiltersBwd: bwd_conv_filters(); break;
      case Stage::End: break;
    }
    return rc;
  }
  // what the side streams were given is joined before a call returns: the optimizer, an exchange and the next call find it done
  int join_sides(const char* what) {
    sj.join(SJ_DP);      // (dP and its squared norm)
    sj.join(SJ_SCORER_BWD);
    return sj.err == hipSuccess ? COPER_OK : fail(h, COPER_EHIP, std::string(what) + ": an event call of the side streams failed");
  }
  // ---- clip + AMSGrad
  bool optimizer() {
    return optimizer_launch(h, T, s, nullptr, sumsq_done, lk ? h->grouping().rel_count : nullptr, 1.0, rows_list, rows_count, false,
                            std::min<int64_t>(B * (L + 1), dm.E));
  }
};

// A step held open (TrainState::open) goes on in this call: a Step over the stored arguments -- `args`: those, or the score call's
// amended copy -- on this call's stream, its workspace pointers set (nothing grows: the call that opened the step sized them), the
// carry restored.  The call suspends the step again with `T->open.carry = st`.
static Step open_resume(coper_handle* h, TrainState* T, StepArgs args, hipStream_t s, int* rc) {
  args.s = s;
  Step st(h, T, args);
  if (!(*rc = st.grow_workspaces())) static_cast<StepCarry&>(st) = T->open.carry;
  return st;
}

// The limits a batch meets in every call that runs the forward stages.  grid_rows: the rows the loss kernel of id-list labels sizes
// its grid by (num_ent on a whole table, the shard's own on a sharded state; 0: the call has no such labels).  `what` names the call;
// the whole-table step names its id-list entry point in that one refusal.
static int check_batch_limits(coper_handle* h, const TrainState* T, const std::string& what, int64_t B, int64_t grid_rows) {
  if (grid_rows && B * ((grid_rows + TR_CSR_STRETCH - 1) / TR_CSR_STRETCH) > 0x7fffffff)
    return fail(h, COPER_EINVAL, what + (T->sharded ? "" : "_csr") + ": batch too large for the loss kernel's grid");
  if ((int64_t)B * h->dm.F > 0xffffffffLL) return fail(h, COPER_EINVAL, what + ": batch too large for the dropout counter");
  // (routes chosen by pointer alignment -- the fused scorer, the 16-byte loss stream of the CSR chunks -- sum in another order)
  if (T->det && (((uintptr_t)T->lv.ent_emb->p | (uintptr_t)T->lv.pred_bias->p) & 15) != 0)
    return fail(h, COPER_EUNSUPPORTED, what + ": deterministic mode: ent_emb and pred_bias must be 16-byte aligned");
  return COPER_OK;
}

// A backward pass is complete and no update has consumed it: coper_train_backward leaves the gradients where they are for
// coper_train_grads_export / coper_train_apply; coper_train_rows_backward for coper_train_rows_export / coper_train_rows_apply, the
// table part being the claimed list
static void finish_backward(const coper_handle* h, TrainState* T, StepKind kind, int64_t B, int64_t L) {
  T->step += 1;
  if (kind == StepKind::Backward) T->pending = true;
  else {
    T->rows_pending_small = T->rows_pending_table = true;
    T->rows_bound = std::min<int64_t>(B * (L + 1), h->dm.E);
  }
}

}  // namespace

// coper_prepare, coper_set_param of ent_emb / pred_bias (coper_abi.hip) and the calls here that read or replace the tables whole: with
// deferred rows on, every row current first.  device_wide: for a caller without a stream -- the pass runs on the null stream between two
// device synchronisations.  Nothing to do without a training state or with the mode off.
int coper::train_rows_sync(coper_handle* h, void* stream, bool device_wide) {
  TrainState* T = (TrainState*)h->train;
  if (!T || !T->rows_deferred) return COPER_OK;
  COPER_HIP_TRY(h, hipSetDevice(h->cfg.device));
  if (device_wide) COPER_HIP_TRY(h, hipDeviceSynchronize());
  if (int rc = rows_sync_launch(h, T, device_wide ? nullptr : (hipStream_t)stream)) return rc;
  if (device_wide) COPER_HIP_TRY(h, hipDeviceSynchronize());
  return COPER_OK;
}

// ---- synchronised batch statistics (include/coper_hip.h, "Synchronised batch statistics")
namespace {
// what coper_train_sync_begin / _csr adds to the arguments of coper_train_backward / _rows_backward
struct SyncReq {
  int64_t B_global, sample_offset;
  int32_t rows;
  double* part_out;
  int64_t part_cap;
  int64_t* n_out;
};
inline bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }
// this rank's share of a batch-wide sum, ordered on the caller's stream behind the launches that formed it
static int sync_hand_out(coper_handle* h, hipStream_t s, const double* sums, int64_t n, double* part_out, int64_t* n_out) {
  COPER_HIP_TRY(h, hipMemcpyAsync(part_out, sums, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s));
  *n_out = n;
  return COPER_OK;
}
// the refusals of a begin call that the step's own checks do not make
static int sync_check_begin(coper_handle* h, const TrainState* T, const SyncReq& q, int64_t B) {
  const Dims& dm = h->dm;
  if (q.rows != 0 && q.rows != 1) return fail(h, COPER_EINVAL, "coper_train_sync_begin: rows is 0 or 1");
  if (!q.n_out) return fail(h, COPER_EINVAL, "coper_train_sync_begin: n_out is NULL");
  if (B <= 0 || q.B_global <= 0 || q.B_global % B != 0)
    return fail(h, COPER_EINVAL, "coper_train_sync_begin: B_global must be a multiple of B (even shards)");
  if (q.sample_offset < 0 || q.sample_offset + B > q.B_global)
    return fail(h, COPER_EINVAL, "coper_train_sync_begin: the shard [sample_offset, sample_offset + B) does not lie in [0, B_global)");
  if (T->sharded)
    return fail(h, COPER_EUNSUPPORTED, "coper_train_sync_begin: an entity-sharded state (coper_train_init_sharded) replicates the encoder on the whole "
                                       "batch: its statistics are the whole batch's already");
  if (T->cfg.batch_norm_train_stats && dm.ctx_bn && (T->nh > 0 || T->nhc > 0))
    return fail(h, COPER_EUNSUPPORTED, "coper_train_sync_begin: a generator with hidden layers and context_rel_use_batch_norm: its hidden BN layers take "
                                       "batch statistics too, and synchronising them is not built");
  const int64_t n = T->cfg.batch_norm_train_stats ? 2 * (int64_t)dm.C : 0;
  if (n && (!q.part_out || !aligned8(q.part_out))) return fail(h, COPER_EINVAL, "coper_train_sync_begin: part_out must be an 8-byte aligned device buffer");
  if (q.part_cap < n) return fail(h, COPER_EINVAL, "coper_train_sync_begin: part_cap is below the 2 * conv_num_channels doubles this call hands out");
  if ((q.sample_offset + B) * (int64_t)dm.F > 0xffffffffLL)
    return fail(h, COPER_EINVAL, "coper_train_sync_begin: (sample_offset + B) * features does not fit the dropout counter");
  return COPER_OK;
}
}  // namespace

static int train_step_impl(coper_handle* h, const int64_t* e1, const int64_t* rel, const int32_t* lookup, const float* labels,
                           int64_t B, int64_t L, float* loss_out, void* stream, const StepKind kind, float* pred_out, float* h_out,
                           const CsrLabels csr = CsrLabels(), const SyncReq* sync = nullptr) {
  if (!h) return COPER_EINVAL;
  TrainState* T = (TrainState*)h->train;
  if (!T) return fail(h, COPER_ESTATE, "coper_train_step: call coper_train_init first");
  if (sync) {
    if (int rc = sync_check_begin(h, T, *sync, B)) return rc;
    *sync->n_out = 0;
  }
  if (csr.indptr) {      // sparse 1-vs-all labels: L is num_ent, no [B, L] matrix exists and nothing is indexed by B * L in 32 bits
    if (!e1 || !rel || !csr.idx || B <= 0 || csr.n_rows < 0 || (!csr.row && csr.n_rows != B))
      return fail(h, COPER_EINVAL, "coper_train_step_csr: bad argument (lab_row == NULL needs n_rows == B)");
  } else {
  if (!e1 || !rel || !labels || B <= 0 || L <= 0 || B * L > 0x7fffffff)
    return fail(h, COPER_EINVAL, "coper_train_step: bad argument");
  if (!lookup && L != h->dm.E) return fail(h, COPER_EINVAL, "coper_train_step: lookup == NULL needs labels of shape [B, num_ent]");
  if (!lookup && !dense_S_fits(B, h->dm.E))
    return fail(h, COPER_EUNSUPPORTED, "coper_train_step: 1-vs-all training needs B*num_ent*4 <= 512 MiB in this version");
  }
  if (T->sharded)      // (the entity-sharded state has its own four calls and no other step)
    return fail(h, COPER_EUNSUPPORTED, "coper_train_step / _backward / _forward: an entity-sharded state (coper_train_init_sharded) steps through "
                                       "coper_train_shard_forward | _score_csr | _backward | _apply");
  if (kind == StepKind::RowsBackward && !T->rows_deferred)      // coper_train_rows_backward: the mode's own backward
    return fail(h, COPER_ESTATE, "coper_train_rows_backward: the deferred-rows mode is off (coper_train_defer_rows; coper_train_backward is the dense call)");
  if (T->rows_deferred) {      // what has a gradient in every row, or hands the dense gradient on, is refused
    if (csr.indptr || !lookup)
      return fail(h, COPER_EUNSUPPORTED, "coper_train_step: deferred-rows mode (coper_train_defer_rows): a 1-vs-all step has a gradient in every row");
    if (kind == StepKind::Backward)
      return fail(h, COPER_EUNSUPPORTED, "coper_train_backward: deferred-rows mode (coper_train_defer_rows): the split step's flat gradient is dense "
                                         "(the mode's split step: coper_train_rows_backward / _export / _import / _apply)");
    if (B * (L + 1) > 0x7fffffff) return fail(h, COPER_EINVAL, "coper_train_step: deferred-rows mode: B * (L + 1) ids do not fit the row lists");
  }
  StepArgs a;
  a.kind = kind; a.s = (hipStream_t)stream; a.e1 = e1; a.rel = rel; a.lookup = lookup; a.labels = labels; a.B = B; a.L = L;
  a.loss_out = loss_out; a.pred_out = pred_out; a.h_out = h_out; a.csr = csr;
  a.plan = plan_scorer(h, T, lookup, csr, B);
  if (sync) { a.B_stat = sync->B_global; a.sample_offset = sync->sample_offset; }
  if (T->det) {      // what the mode does not put in order is refused, never served unordered
    // (the plan says atomics: no dense S for this B * num_ent.  Ordered rows: the sorted-segment route at every num_ent)
    if (a.plan.table == TableGrad::Atomics)
      return fail(h, COPER_EUNSUPPORTED, "coper_train_step: deterministic mode: sampled labels at B*num_ent*4 > 512 MiB take the atomic scorer backward");
    if (lookup && T->rows_ordered && (B * (L + 1) > 0x7fffffff || h->dm.E > 0x7fffffff))
      return fail(h, COPER_EINVAL, "coper_train_step: ordered rows: B * (L + 1) ids and num_ent must fit 31 bits");
  }
  int rc;
  if ((rc = check_batch_limits(h, T, "coper_train_step", B, csr.indptr ? (int64_t)h->dm.E : 0))) return rc;
  COPER_HIP_TRY(h, hipSetDevice(h->cfg.device));
  if (runs_optimizer(kind)) h->prepared = false;   // the variables change: per-relation caches, fragment images and folded BN go stale
  Step st(h, T, a);
  if ((rc = st.grow_workspaces())) return rc;
  if (st.plan.ordered() && (rc = ord_grow(h, T, B * (L + 1), st.s))) return rc;
  if (st.rows) {
    if ((rc = rows_wrap_guard(h, T, st.s)) || (rc = st.rows_grow())) return rc;
  }
  T->pending = false;      // (the gradient buffers are zeroed next: what a coper_train_backward left in them is gone)
  T->rows_pending_clear();      // (... and what a coper_train_rows_backward or the imports left: rows_rezero below)
  T->open = OpenStep();         // (... and a synchronised step that was open: abandoned, as a pending backward is dropped)
  st.zero_accumulators();
  if (st.rows) {
    rows_rezero_launch(h, T, st.s);
    st.rows_claim_catch_up();
  }
  if (st.lk && (rc = st.group_for_lookup())) return rc;

  if (sync && st.use_batch) {      // coper_train_sync_begin: up to the first batch-wide sum; the rest of the step is coper_train_sync_next's
    if ((rc = T->sync_sums.ensure(h, (size_t)4 * T->mx, "synchronised BN sums"))) return rc;
    if ((rc = st.run(Stage::ConvFilters, Stage::Bn1))) return rc;
    if ((rc = sync_hand_out(h, st.s, st.bn1_fwd_sums(), 2 * (int64_t)st.C, sync->part_out, sync->n_out))) return rc;
    COPER_HIP_TRY(h, hipGetLastError());
    T->open = OpenStep{a, st /* the StepCarry part */, 1};
    return COPER_OK;
  }
  // coper_train_forward: nothing is differentiated, nothing updated, the step counter (dropout masks) stays
  if ((rc = st.run(Stage::ConvFilters, differentiates(kind) ? Stage::End : Stage::ScorerBwd))) return rc;
  if ((rc = st.join_sides("coper_train_step"))) return rc;
  if (!runs_optimizer(kind)) {
    COPER_HIP_TRY(h, hipGetLastError());
    if (differentiates(kind)) finish_backward(h, T, kind, B, L);
    return COPER_OK;
  }
  const bool wmax_carried = st.optimizer();
  COPER_HIP_TRY(h, hipGetLastError());
  T->step += 1;
  finish_update(T, wmax_carried);
  return COPER_OK;
}

// k_tr_grads_export over every leaf at its flat_off, or (small) over the leaves of the small flat vector at their small_off
static void grads_export_launch(coper_handle* h, TrainState* T, hipStream_t s, bool small, bool accumulate, float* out) {
  ExportList el;
  int np = 0;
  el.table = -1; el.rowlen = 1; el.rowcnt = nullptr;
  for (const TrainParam& t : T->tp) {
    if (small && t.small_off < 0) continue;
    const int i = np++;
    el.g[i] = t.g; el.off[i] = small ? t.small_off : t.flat_off; el.n[i] = t.n; el.span[i] = (t.n + 63) / 64 * 64;
    if (h->dm.lookup && h->dm.gen_fc && &t == T->lv.fc_weights) {      // rows of relations absent from the backward's batch: zeros
      el.table = i; el.rowlen = h->dm.F * (int64_t)h->dm.d; el.rowcnt = T->step_rel_count;
    }
  }
  if (accumulate) hipLaunchKernelGGL(k_tr_grads_export<true>, dim3(1024, (unsigned)np), dim3(256), 0, s, el, out);
  else hipLaunchKernelGGL(k_tr_grads_export<false>, dim3(1024, (unsigned)np), dim3(256), 0, s, el, out);
}

extern "C" {

COPER_API int coper_train_step(coper_handle* h, const int64_t* e1, const int64_t* rel, const int32_t* lookup, const float* labels,
                               int64_t B, int64_t L, float* loss_out, void* stream) {
  return train_step_impl(h, e1, rel, lookup, labels, B, L, loss_out, stream, StepKind::Step, nullptr, nullptr);
}

COPER_API int coper_train_forward(coper_handle* h, const int64_t* e1, const int64_t* rel, const int32_t* lookup, const float* labels,
                                  int64_t B, int64_t L, float* loss_out, float* pred_out, float* h_out, void* stream) {
  return train_step_impl(h, e1, rel, lookup, labels, B, L, loss_out, stream, StepKind::Forward, pred_out, h_out);
}

COPER_API int coper_train_step_csr(coper_handle* h, const int64_t* e1, const int64_t* rel, const int64_t* lab_indptr, const int64_t* lab_idx,
                                   const int64_t* lab_row, int64_t n_rows, int64_t B, float* loss_out, void* stream) {
  if (!h) return COPER_EINVAL;
  if (!lab_indptr) return fail(h, COPER_EINVAL, "coper_train_step_csr: bad argument (lab_indptr is NULL)");
  return train_step_impl(h, e1, rel, nullptr, nullptr, B, h->dm.E, loss_out, stream, StepKind::Step, nullptr, nullptr, CsrLabels{lab_indptr, lab_idx, lab_row, n_rows});
}

COPER_API int coper_train_forward_csr(coper_handle* h, const int64_t* e1, const int64_t* rel, const int64_t* lab_indptr, const int64_t* lab_idx,
                                      const int64_t* lab_row, int64_t n_rows, int64_t B, float* loss_out, float* pred_out, float* h_out,
                                      void* stream) {
  if (!h) return COPER_EINVAL;
  if (!lab_indptr) return fail(h, COPER_EINVAL, "coper_train_step_csr: bad argument (lab_indptr is NULL)");
  return train_step_impl(h, e1, rel, nullptr, nullptr, B, h->dm.E, loss_out, stream, StepKind::Forward, pred_out, h_out, CsrLabels{lab_indptr, lab_idx, lab_row, n_rows});
}

// ---- the split step: backward | export | apply (include/coper_hip.h, "The step in three calls")
COPER_API int coper_train_backward(coper_handle* h, const int64_t* e1, const int64_t* rel, const int32_t* lookup, const float* labels,
                                   int64_t B, int64_t L, float* loss_out, void* stream) {
  return train_step_impl(h, e1, rel, lookup, labels, B, L, loss_out, stream, StepKind::Backward, nullptr, nullptr);
}

COPER_API int coper_train_backward_csr(coper_handle* h, const int64_t* e1, const int64_t* rel, const int64_t* lab_indptr, const int64_t* lab_idx,
                                       const int64_t* lab_row, int64_t n_rows, int64_t B, float* loss_out, void* stream) {
  if (!h) return COPER_EINVAL;
  if (!lab_indptr) return fail(h, COPER_EINVAL, "coper_train_backward_csr: bad argument (lab_indptr is NULL)");
  return train_step_impl(h, e1, rel, nullptr, nullptr, B, h->dm.E, loss_out, stream, StepKind::Backward, nullptr, nullptr, CsrLabels{lab_indptr, lab_idx, lab_row, n_rows});
}

COPER_API int coper_train_grads_layout(coper_handle* h, const char* leaf_name, int64_t* offset, int64_t* n, int64_t* total) {
  if (!h) return COPER_EINVAL;
  TrainState* T = (TrainState*)h->train;
  if (!T) return fail(h, COPER_ESTATE, "coper_train_grads_layout: call coper_train_init first");
  if (total) *total = T->flat_total;
  if (!leaf_name) return COPER_OK;
  const TrainParam* t = T->find(leaf_name);
  if (!t) return fail(h, COPER_EINVAL, std::string("coper_train_grads_layout: not a trainable leaf: ") + leaf_name);
  if (offset) *offset = t->flat_off;
  if (n) *n = t->n;
  return COPER_OK;
}

COPER_API int coper_train_grads_export(coper_handle* h, float* flat, int64_t cap, int32_t accumulate, void* stream) {
  if (!h) return COPER_EINVAL;
  TrainState* T = (TrainState*)h->train;
  if (!T) return fail(h, COPER_ESTATE, "coper_train_grads_export: call coper_train_init first");
  if (T->sync_phase()) return fail(h, COPER_ESTATE, "coper_train_grads_export: a synchronised step is open (coper_train_sync_next completes it; a step-shaped call abandons it)");
  if (T->sharded)
    return fail(h, COPER_EUNSUPPORTED, "coper_train_grads_export: an entity-sharded state (coper_train_init_sharded): no table gradient leaves its shard");
  if (T->rows_deferred)
    return fail(h, COPER_EUNSUPPORTED, "coper_train_grads_export: deferred-rows mode (coper_train_defer_rows): the flat gradient vector is dense by contract "
                                       "(the mode's export: coper_train_rows_export)");
  if (!flat || ((uintptr_t)flat & 15) != 0) return fail(h, COPER_EINVAL, "coper_train_grads_export: flat must be a 16-byte aligned device buffer");
  if (cap < T->flat_total) return fail(h, COPER_EINVAL, "coper_train_grads_export: flat holds fewer than coper_train_grads_layout's total");
  COPER_HIP_TRY(h, hipSetDevice(h->cfg.device));
  grads_export_launch(h, T, (hipStream_t)stream, false, accumulate != 0, flat);
  COPER_HIP_TRY(h, hipGetLastError());
  return COPER_OK;
}

COPER_API int coper_train_apply(coper_handle* h, const float* flat, int64_t n, double scale, void* stream) {
  if (!h) return COPER_EINVAL;
  TrainState* T = (TrainState*)h->train;
  if (!T) return fail(h, COPER_ESTATE, "coper_train_apply: call coper_train_init first");
  if (T->sync_phase()) return fail(h, COPER_ESTATE, "coper_train_apply: a synchronised step is open (coper_train_sync_next completes it; a step-shaped call abandons it)");
  if (T->sharded)
    return fail(h, COPER_EUNSUPPORTED, "coper_train_apply: an entity-sharded state (coper_train_init_sharded): its update is coper_train_shard_apply");
  if (T->rows_deferred)
    return fail(h, COPER_EUNSUPPORTED, "coper_train_apply: deferred-rows mode (coper_train_defer_rows): an update from the dense flat gradient touches every row "
                                       "(the mode's update: coper_train_rows_apply)");
  if (!flat && !T->pending)
    return fail(h, COPER_ESTATE, "coper_train_apply: no gradients pending (no coper_train_backward since the last update, step, forward or init)");
  if (flat && (n != T->flat_total || ((uintptr_t)flat & 15) != 0))
    return fail(h, COPER_EINVAL, "coper_train_apply: flat must be 16-byte aligned and n coper_train_grads_layout's total");
  if (!std::isfinite(scale)) return fail(h, COPER_EINVAL, "coper_train_apply: scale is not finite");
  COPER_HIP_TRY(h, hipSetDevice(h->cfg.device));
  hipStream_t const s = (hipStream_t)stream;
  int rc;
  if (T->det && (size_t)512 * TR_MAX_PARAMS > T->det_slab.size()) {      // (an apply from a flat vector on a handle that ran no backward yet)
    COPER_HIP_TRY(h, hipStreamSynchronize(s));
    if ((rc = T->det_slab.alloc(h, (size_t)512 * TR_MAX_PARAMS, "deterministic slabs"))) return rc;
  }
  h->prepared = false;   // the variables change: per-relation caches, fragment images and folded BN go stale
  T->pending = false;    // (whatever follows: the gradients are consumed, or describe variables that are about to change)
  zero_update_slots(T, s);
  // the norm over every leaf (the epilogues' squares belonged to one backward); absent rows of the looked-up table by the backward's
  // snapshot, never by the grouping workspace (an evaluation pass may have grouped since); from a flat vector every row is present:
  // no counts at all, so the table takes the 16-byte routes of every other leaf (3.0 + 4.7 ms of k_tr_sumsq + k_tr_amsgrad through
  // the row-count route at the FB15k-237 table) -- except in deterministic mode, where counts of one keep it on the
  // fused step's route and in its summation order
  const int32_t* const counts = flat ? (T->det ? T->all_rel_count.get() : nullptr) : T->step_rel_count.get();
  const bool wmax_carried = optimizer_launch(h, T, s, flat, nullptr, counts, scale);
  COPER_HIP_TRY(h, hipGetLastError());
  finish_update(T, wmax_carried);
  return COPER_OK;
}

COPER_API int coper_train_wmax_carried(const coper_handle* h) {
  if (!h) return -COPER_EINVAL;
  const TrainState* T = (const TrainState*)h->train;
  return T ? (T->wmax_valid ? 1 : 0) : -COPER_ESTATE;
}

COPER_API int coper_train_deterministic(const coper_handle* h) {
  if (!h) return -COPER_EINVAL;
  const TrainState* T = (const TrainState*)h->train;
  return T ? (T->det ? 1 : 0) : -COPER_ESTATE;
}

// ---- deferred rows (include/coper_hip.h, "Deferred rows")
COPER_API int coper_train_defer_rows(coper_handle* h, int32_t enable, void* stream) {
  if (!h) return COPER_EINVAL;
  TrainState* T = (TrainState*)h->train;
  if (!T) return fail(h, COPER_ESTATE, "coper_train_defer_rows: call coper_train_init first");
  if (enable != 0 && enable != 1) return fail(h, COPER_EINVAL, "coper_train_defer_rows: enable is 0 or 1");
  // (an entity-sharded state, DESIGN 6.11: between steps only -- the list of a step is built, caught up, summed and updated across its calls)
  if (T->sharded && T->open.phase != SHP_FORWARD)
    return fail(h, COPER_ESTATE, std::string("coper_train_defer_rows: inside an entity-sharded step: the next call of this step is ") + kShardCall[T->open.phase]);
  if (enable && T->det && !T->rows_ordered && !T->sharded)      // (ordered rows put both in order: coper_train_order_rows; a sharded state's sampled call is always ordered)
    return fail(h, COPER_EUNSUPPORTED, "coper_train_defer_rows: a deterministic state: the unique-row list and the atomic scorer backward are unordered");
  if ((enable != 0) == T->rows_deferred) return COPER_OK;
  // (an entity-sharded state chooses the mode before its first step -- train_init's flag; leaving it is served at any step boundary.
  //  Entering it on a state that has stepped is not built, and stays the refusal it was)
  if (enable && T->sharded && T->sh_stepped)
    return fail(h, COPER_EUNSUPPORTED, "coper_train_defer_rows: an entity-sharded state (coper_train_init_sharded) that has made a step: the mode is "
                                       "enabled before the first step of the state (a new coper_train_init_sharded starts one)");
  COPER_HIP_TRY(h, hipSetDevice(h->cfg.device));
  hipStream_t const s = (hipStream_t)stream;
  if (!enable) {      // every row current, then the dense path again (it zeroes the gradient buffers whole; the row state is rebuilt at the next enable)
    if (int rc = rows_sync_launch(h, T, s)) return rc;
    T->rows_deferred = false;
    T->rows_pending_clear();      // (the dense step zeroes the two buffers whole: a pending row gradient is gone)
    T->open = OpenStep();         // (an open synchronised step was the mode's: abandoned)
    return COPER_OK;
  }
  const size_t E = (size_t)rows_held(h, T);      // (a shard: a word and a claim bit per OWNED row)
  int rc;
  if ((rc = T->rows_word.ensure(h, E, "deferred-row step words")) || (rc = T->rows_claim.ensure(h, (E + 31) / 32, "deferred-row claim bits")) ||
      (rc = T->rows_count.ensure(h, 2, "deferred-row counts")) || (rc = T->rows_stats.ensure(h, 2, "deferred-row statistics")))
    return rc;
  // every row is current now; no row is listed; the two gradient buffers are zero everywhere (from here on: but for the listed rows)
  COPER_HIP_TRY(h, hipMemsetAsync(T->rows_word, 0, sizeof(int32_t) * E, s));
  COPER_HIP_TRY(h, hipMemsetAsync(T->rows_claim, 0, sizeof(unsigned) * ((E + 31) / 32), s));
  COPER_HIP_TRY(h, hipMemsetAsync(T->rows_count, 0, 2 * sizeof(int32_t), s));
  COPER_HIP_TRY(h, hipMemsetAsync(T->lv.ent_emb->g, 0, sizeof(float) * (size_t)T->lv.ent_emb->n, s));
  COPER_HIP_TRY(h, hipMemsetAsync(T->lv.pred_bias->g, 0, sizeof(float) * (size_t)T->lv.pred_bias->n, s));
  T->rows_now = 0;
  T->rows_prev = 0;
  T->rows_l2b1p = std::log2(T->b1p);      // (log2(0) = -inf: the power is 0 at every gap, as the dense step has it)
  T->rows_l2b2p = std::log2(T->b2p);
  T->pending = false;      // (a pending backward's gradient is gone with the zeroing)
  T->open = OpenStep();    // (... and an open synchronised step)
  T->rows_pending_clear();
  T->rows_deferred = true;
  return COPER_OK;
}

COPER_API int coper_train_rows_deferred(const coper_handle* h) {
  if (!h) return -COPER_EINVAL;
  const TrainState* T = (const TrainState*)h->train;
  return T ? (T->rows_deferred ? 1 : 0) : -COPER_ESTATE;
}

// the updates made since the mode was enabled (what the rows' step words count in); 0 with the mode off
COPER_API int64_t coper_train_rows_updates(const coper_handle* h) {
  if (!h) return -COPER_EINVAL;
  const TrainState* T = (const TrainState*)h->train;
  return T ? (T->rows_deferred ? (int64_t)T->rows_now : 0) : -COPER_ESTATE;
}

// ---- ordered rows (include/coper_hip.h, "Ordered rows")
COPER_API int coper_train_order_rows(coper_handle* h, int32_t enable, void* stream) {
  if (!h) return COPER_EINVAL;
  TrainState* T = (TrainState*)h->train;
  if (!T) return fail(h, COPER_ESTATE, "coper_train_order_rows: call coper_train_init first");
  if (enable != 0 && enable != 1) return fail(h, COPER_EINVAL, "coper_train_order_rows: enable is 0 or 1");
  if (T->sharded)
    return fail(h, COPER_EUNSUPPORTED, "coper_train_order_rows: an entity-sharded state (coper_train_init_sharded) takes no sampled labels");
  if (!T->det)
    return fail(h, COPER_EUNSUPPORTED, "coper_train_order_rows: a deterministic = 0 state: the rest of its step is unordered, so nothing could be promised");
  if (!enable && T->rows_deferred)
    return fail(h, COPER_ESTATE, "coper_train_order_rows: deferred rows is on and needs the ordered list on this state: disable deferred rows first");
  if ((enable != 0) == T->rows_ordered) return COPER_OK;
  (void)stream;      // (nothing is launched: the workspace grows with the first batch)
  T->rows_ordered = enable != 0;
  T->rows_list_unsorted = false;
  T->pending = false;      // (as switching deferred rows: what a split step left pending is dropped, never applied by another route)
  T->open = OpenStep();    // (... and an open synchronised step with it)
  T->rows_pending_clear();
  return COPER_OK;
}

COPER_API int coper_train_rows_ordered(const coper_handle* h) {
  if (!h) return -COPER_EINVAL;
  const TrainState* T = (const TrainState*)h->train;
  return T ? (T->rows_ordered ? 1 : 0) : -COPER_ESTATE;
}

COPER_API int coper_train_sync_rows(coper_handle* h, void* stream) {
  if (!h) return COPER_EINVAL;
  if (!h->train) return fail(h, COPER_ESTATE, "coper_train_sync_rows: call coper_train_init first");
  return train_rows_sync(h, stream, false);
}

COPER_API int coper_train_row_stats(coper_handle* h, int64_t* rows_last_step, int64_t* rows_behind, int64_t* max_gap, void* stream) {
  if (!h) return COPER_EINVAL;
  TrainState* T = (TrainState*)h->train;
  if (!T) return fail(h, COPER_ESTATE, "coper_train_row_stats: call coper_train_init first");
  if (rows_last_step) *rows_last_step = 0;
  if (rows_behind) *rows_behind = 0;
  if (max_gap) *max_gap = 0;
  if (!T->rows_deferred) return COPER_OK;      // (the dense step: every row current, nothing listed)
  COPER_HIP_TRY(h, hipSetDevice(h->cfg.device));
  hipStream_t const s = (hipStream_t)stream;
  COPER_HIP_TRY(h, hipMemsetAsync(T->rows_stats, 0, 2 * sizeof(unsigned long long), s));
  const int64_t held = rows_held(h, T);      // (a shard: over its own rows)
  hipLaunchKernelGGL(k_rows_stats, dim3((unsigned)std::min<int64_t>((held + 255) / 256, 4096)), dim3(256), 0, s, T->rows_word.get(), held,
                     T->rows_now, T->rows_stats.get());
  COPER_HIP_TRY(h, hipGetLastError());
  unsigned long long st[2] = {0, 0};
  int32_t counts[2] = {0, 0};
  COPER_HIP_TRY(h, hipMemcpyAsync(st, T->rows_stats, sizeof st, hipMemcpyDeviceToHost, s));
  COPER_HIP_TRY(h, hipMemcpyAsync(counts, T->rows_count, sizeof counts, hipMemcpyDeviceToHost, s));
  COPER_HIP_TRY(h, hipStreamSynchronize(s));
  if (rows_last_step) *rows_last_step = counts[T->rows_prev];
  if (rows_behind) *rows_behind = (int64_t)st[0];
  if (max_gap) *max_gap = (int64_t)st[1];
  return COPER_OK;
}

// ---- deferred rows: the step in calls (include/coper_hip.h, "Deferred rows: the step in calls")
static inline int rows_block_stride(int d) { return (d + 1 + 3) & ~3; }

// The id lists at `need` entries or more WITH what they hold (Step::rows_grow re-zeroes the listed rows and drops the list: a step is
// about to do that anyway; an import adds to the list).  Doubles, up to E, so that the imports of one update grow it a few times at most.
static int rows_grow_keep(coper_handle* h, TrainState* T, int64_t need, hipStream_t s) {
  if (need <= T->rows_cap) return COPER_OK;
  const int64_t cap = std::max<int64_t>(need, std::min<int64_t>(2 * T->rows_cap, h->dm.E));
  DevBuf<int32_t> grown[2];
  int rc;
  COPER_HIP_TRY(h, hipStreamSynchronize(s));
  for (int i = 0; i < 2; ++i) {
    if ((rc = grown[i].alloc(h, (size_t)cap, "deferred-row list"))) return rc;      // (nothing has changed: the old lists stand)
    if (T->rows_cap)
      COPER_HIP_TRY(h, hipMemcpyAsync(grown[i], T->rows_list[i], sizeof(int32_t) * (size_t)T->rows_cap, hipMemcpyDeviceToDevice, s));
  }
  COPER_HIP_TRY(h, hipStreamSynchronize(s));
  for (int i = 0; i < 2; ++i) T->rows_list[i] = std::move(grown[i]);
  T->rows_cap = cap;
  return COPER_OK;
}

COPER_API int coper_train_rows_layout(coper_handle* h, const char* leaf_name, int64_t* offset, int64_t* n, int64_t* total, int64_t* row_stride) {
  if (!h) return COPER_EINVAL;
  TrainState* T = (TrainState*)h->train;
  if (!T) return fail(h, COPER_ESTATE, "coper_train_rows_layout: call coper_train_init first");
  if (total) *total = T->small_total;
  if (row_stride) *row_stride = rows_block_stride(h->dm.d);
  if (!leaf_name) return COPER_OK;
  const TrainParam* t = T->find(leaf_name);
  if (!t) return fail(h, COPER_EINVAL, std::string("coper_train_rows_layout: not a trainable leaf: ") + leaf_name);
  if (t->small_off < 0)
    return fail(h, COPER_EINVAL, std::string("coper_train_rows_layout: ") + leaf_name + " travels as row blocks, not in the small flat vector");
  if (offset) *offset = t->small_off;
  if (n) *n = t->n;
  return COPER_OK;
}

COPER_API int coper_train_rows_backward(coper_handle* h, const int64_t* e1, const int64_t* rel, const int32_t* lookup, const float* labels,
                                        int64_t B, int64_t L, float* loss_out, void* stream) {
  return train_step_impl(h, e1, rel, lookup, labels, B, L, loss_out, stream, StepKind::RowsBackward, nullptr, nullptr);
}

COPER_API int coper_train_rows_export(coper_handle* h, float* small, int64_t small_cap, int32_t accumulate, int32_t* ids, float* vals,
                                      int64_t row_cap, int32_t* count, void* stream) {
  if (!h) return COPER_EINVAL;
  TrainState* T = (TrainState*)h->train;
  if (!T) return fail(h, COPER_ESTATE, "coper_train_rows_export: call coper_train_init first");
  if (T->sync_phase()) return fail(h, COPER_ESTATE, "coper_train_rows_export: a synchronised step is open (coper_train_sync_next completes it; a step-shaped call abandons it)");
  if (!T->rows_deferred) return fail(h, COPER_ESTATE, "coper_train_rows_export: the deferred-rows mode is off (coper_train_grads_export is the dense call)");
  if (T->sharded)      // (a shard steps through its four calls in the mode too; the row-block split step is not built there)
    return fail(h, COPER_EUNSUPPORTED, "coper_train_rows_export: an entity-sharded state (coper_train_init_sharded) steps through coper_train_shard_forward | "
                                       "_score_lookup | _backward | _apply in the deferred-rows mode too");
  if ((ids == nullptr) != (vals == nullptr)) return fail(h, COPER_EINVAL, "coper_train_rows_export: ids and vals are given or NULL together");
  if (!small && !ids) return fail(h, COPER_EINVAL, "coper_train_rows_export: nothing to export into");
  if (small && !T->rows_pending_small)
    return fail(h, COPER_ESTATE, "coper_train_rows_export: no gradients pending (no coper_train_rows_backward since the last update, step, forward or init)");
  if (ids && !T->rows_pending_table)
    return fail(h, COPER_ESTATE, "coper_train_rows_export: no row gradients pending (no coper_train_rows_backward or import since the last update, step, forward or init)");
  if (small && (((uintptr_t)small & 15) != 0 || small_cap < T->small_total))
    return fail(h, COPER_EINVAL, "coper_train_rows_export: small must be 16-byte aligned and hold coper_train_rows_layout's total");
  if (ids && (row_cap < T->rows_bound || row_cap > 0x7fffffff))
    return fail(h, COPER_EINVAL, "coper_train_rows_export: row_cap is below the bound of the pending rows (min(B (L + 1), num_ent) of the backward; min(num_ent, entries imported))");
  if (ids && (((uintptr_t)ids & 3) != 0 || ((uintptr_t)vals & 3) != 0)) return fail(h, COPER_EINVAL, "coper_train_rows_export: misaligned ids / vals");
  COPER_HIP_TRY(h, hipSetDevice(h->cfg.device));
  hipStream_t const s = (hipStream_t)stream;
  if (small) grads_export_launch(h, T, s, true, accumulate != 0, small);      // every leaf but the two tables, at their offsets in the small vector
  if (ids) {
    if (int rc = ord_sort_pending_list(h, T, s)) return rc;      // (ordered rows: the block in ascending row id, after imports too)
    const RowTables t = row_tables(h, T);
    const int pv = T->rows_prev;
    hipLaunchKernelGGL(k_rows_export, rows_grid(row_cap), dim3(256), 0, s, t, (const int32_t*)T->rows_list[pv].get(), (const int32_t*)(T->rows_count + pv),
                       ids, vals, rows_block_stride(h->dm.d), (t.vec && ((uintptr_t)vals & 15) == 0) ? 1 : 0, row_cap, count);
    prof_count(h, "train.rows.export");
  }
  COPER_HIP_TRY(h, hipGetLastError());
  return COPER_OK;
}

COPER_API int coper_train_rows_import(coper_handle* h, const int32_t* ids, const float* vals, int64_t n, int32_t first, void* stream) {
  if (!h) return COPER_EINVAL;
  TrainState* T = (TrainState*)h->train;
  if (!T) return fail(h, COPER_ESTATE, "coper_train_rows_import: call coper_train_init first");
  if (!T->rows_deferred) return fail(h, COPER_ESTATE, "coper_train_rows_import: the deferred-rows mode is off (coper_train_defer_rows)");
  if (T->sharded)      // (a shard steps through its four calls in the mode too; the row-block split step is not built there)
    return fail(h, COPER_EUNSUPPORTED, "coper_train_rows_import: an entity-sharded state (coper_train_init_sharded) steps through coper_train_shard_forward | "
                                       "_score_lookup | _backward | _apply in the deferred-rows mode too");
  if (n < 0 || n > 0x7fffffff || (n > 0 && (!ids || !vals)) || ((uintptr_t)ids & 3) != 0 || ((uintptr_t)vals & 3) != 0)
    return fail(h, COPER_EINVAL, "coper_train_rows_import: bad argument");
  if (!first && !T->rows_pending_table)
    return fail(h, COPER_ESTATE, "coper_train_rows_import: no row gradients pending to add to: the first import of an update passes first != 0");
  COPER_HIP_TRY(h, hipSetDevice(h->cfg.device));
  hipStream_t const s = (hipStream_t)stream;
  const int64_t bound = std::min<int64_t>(h->dm.E, (first ? 0 : T->rows_bound) + n);
  int rc;
  // (at least one entry: the optimizer takes "a list exists" for "the mode is on")
  if ((rc = rows_wrap_guard(h, T, s)) || (rc = rows_grow_keep(h, T, std::max<int64_t>(bound, 1), s))) return rc;
  const RowTables t = row_tables(h, T);
  if (first) {      // a new pending gradient: what a step does to the list of the call before (k_rows_rezero), and the free list becomes the current one
    if (T->rows_cap) rows_rezero_launch(h, T, s);
    T->rows_prev ^= 1;      // (a backward's small gradients stay pending: the import replaces the table part alone)
  }
  if (n > 0) {
    const int cur = T->rows_prev;
    hipLaunchKernelGGL(k_rows_import, grid1d(n), dim3(256), 0, s, t, row_catch_up_args(T), ids, vals, rows_block_stride(h->dm.d),
                       (t.vec && ((uintptr_t)vals & 15) == 0) ? 1 : 0, n, T->rows_claim.get(), T->rows_list[cur].get(), T->rows_count + cur, T->rows_cap);
    prof_count(h, "train.rows.import");
    T->rows_list_unsorted = true;      // (appended in wave-arrival order; ordered rows sort the list before anything reads it in order)
  }
  COPER_HIP_TRY(h, hipGetLastError());
  T->rows_pending_table = true;
  T->rows_bound = bound;
  return COPER_OK;
}

COPER_API int coper_train_rows_apply(coper_handle* h, const float* small, int64_t n, double scale, void* stream) {
  if (!h) return COPER_EINVAL;
  TrainState* T = (TrainState*)h->train;
  if (!T) return fail(h, COPER_ESTATE, "coper_train_rows_apply: call coper_train_init first");
  if (T->sync_phase()) return fail(h, COPER_ESTATE, "coper_train_rows_apply: a synchronised step is open (coper_train_sync_next completes it; a step-shaped call abandons it)");
  if (!T->rows_deferred) return fail(h, COPER_ESTATE, "coper_train_rows_apply: the deferred-rows mode is off (coper_train_apply is the dense call)");
  if (T->sharded)      // (a shard steps through its four calls in the mode too; the row-block split step is not built there)
    return fail(h, COPER_EUNSUPPORTED, "coper_train_rows_apply: an entity-sharded state (coper_train_init_sharded) steps through coper_train_shard_forward | "
                                       "_score_lookup | _backward | _apply in the deferred-rows mode too");
  if (!T->rows_pending_table || (!small && !T->rows_pending_small))
    return fail(h, COPER_ESTATE, "coper_train_rows_apply: no gradients pending (no coper_train_rows_backward or import since the last update, step, forward or init)");
  if (small && (n != T->small_total || ((uintptr_t)small & 15) != 0))
    return fail(h, COPER_EINVAL, "coper_train_rows_apply: small must be 16-byte aligned and n coper_train_rows_layout's total");
  if (!std::isfinite(scale)) return fail(h, COPER_EINVAL, "coper_train_rows_apply: scale is not finite");
  COPER_HIP_TRY(h, hipSetDevice(h->cfg.device));
  hipStream_t const s = (hipStream_t)stream;
  const int64_t rows_n = T->rows_bound;
  if (T->rows_ordered) {      // the norm reads the list in ascending id, through the slab (an apply on a handle whose slab no backward has sized)
    int rc;
    if ((rc = ord_sort_pending_list(h, T, s))) return rc;
    const size_t need = std::max<size_t>((size_t)512 * TR_MAX_PARAMS, (size_t)(rows_n / ORD_SUMSQ_ROWS + 2));
    if (need > T->det_slab.size()) {
      COPER_HIP_TRY(h, hipStreamSynchronize(s));
      if ((rc = T->det_slab.alloc(h, need, "deterministic slabs"))) return rc;
    }
  }
  h->prepared = false;   // the variables change: per-relation caches, fragment images and folded BN go stale
  T->rows_pending_clear();
  zero_update_slots(T, s);      // (as coper_train_apply)
  const int pv = T->rows_prev;
  const bool wmax_carried = optimizer_launch(h, T, s, small, nullptr, small ? nullptr : T->step_rel_count.get(), scale, T->rows_list[pv].get(),
                                             T->rows_count + pv, small != nullptr, rows_n);
  COPER_HIP_TRY(h, hipGetLastError());
  finish_update(T, wmax_carried);
  return COPER_OK;
}

COPER_API int coper_train_grad(coper_handle* h, const char* leaf_name, float* out, int64_t cap, int64_t* n, double* global_norm,
                               void* stream) {
  if (!h || !leaf_name) return COPER_EINVAL;
  TrainState* T = (TrainState*)h->train;
  if (!T) return fail(h, COPER_ESTATE, "coper_train_grad: call coper_train_init first");
  TrainParam* t = T->find(leaf_name);
  if (!t) return fail(h, COPER_EINVAL, std::string("coper_train_grad: not a trainable leaf: ") + leaf_name);
  if (n) *n = t->n;
  if (out) {
    if (cap < t->n) return fail(h, COPER_EINVAL, "coper_train_grad: output buffer too small");
    COPER_HIP_TRY(h, hipMemcpyAsync(out, t->g, sizeof(float) * t->n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (h->dm.lookup && h->dm.gen_fc && t == T->lv.fc_weights && T->step_rel_count && T->step > 0) {
      const int64_t rowlen = h->dm.F * (int64_t)h->dm.d;
      hipLaunchKernelGGL(k_tr_zero_absent_rows, dim3((unsigned)((t->n + 255) / 256 < 4096 ? (t->n + 255) / 256 : 4096)), dim3(256), 0, (hipStream_t)stream, out,
                         T->step_rel_count, rowlen, t->n);
      COPER_HIP_TRY(h, hipGetLastError());
    }
  }
  if (global_norm) {
    COPER_HIP_TRY(h, hipStreamSynchronize((hipStream_t)stream));
    double ss = 0;
    COPER_HIP_TRY(h, hipMemcpy(&ss, T->red_layout().total_sumsq(), sizeof(double), hipMemcpyDeviceToHost));
    *global_norm = std::sqrt(ss);
  }
  return COPER_OK;
}

COPER_API int coper_train_slot(coper_handle* h, const char* leaf_name, int32_t which, float* buf, int64_t cap, int32_t set,
                               int64_t* n, void* stream) {
  if (!h || !leaf_name) return COPER_EINVAL;
  TrainState* T = (TrainState*)h->train;
  if (!T) return fail(h, COPER_ESTATE, "coper_train_slot: call coper_train_init first");
  TrainParam* t = T->find(leaf_name);
  if (!t) return fail(h, COPER_EINVAL, std::string("coper_train_slot: not a trainable leaf: ") + leaf_name);
  if (which < 0 || which > 2) return fail(h, COPER_EINVAL, "coper_train_slot: which = 0 (m), 1 (v), 2 (v_hat)");
  float* slot = which == 0 ? t->m : which == 1 ? t->v : t->vh;
  if (n) *n = t->n;
  if (!buf) return COPER_OK;
  if (cap < t->n) return fail(h, COPER_EINVAL, "coper_train_slot: buffer too small");
  // (deferred rows: a slot of the two tables is read or replaced whole -- every row current first, so that what is read is the dense
  //  optimizer's slot and what is planted belongs to the update count the powers stand at)
  if (T->rows_deferred && (t == T->lv.ent_emb || t == T->lv.pred_bias)) {
    COPER_HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (int rc = rows_sync_launch(h, T, (hipStream_t)stream)) return rc;
  }
  COPER_HIP_TRY(h, hipMemcpyAsync(set ? slot : buf, set ? buf : slot, sizeof(float) * t->n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return COPER_OK;
}

COPER_API int coper_train_powers(coper_handle* h, const double* set_beta1_power, const double* set_beta2_power,
                                 const int64_t* set_step, double* beta1_power, double* beta2_power, int64_t* step) {
  if (!h) return COPER_EINVAL;
  TrainState* T = (TrainState*)h->train;
  if (!T) return fail(h, COPER_ESTATE, "coper_train_powers: call coper_train_init first");
  // (deferred rows: a catch-up reads the gap's learning rates off the CURRENT powers -- every row current under the old ones first.  The
  //  call has no stream: the device is synchronised around the pass)
  if (T->rows_deferred && (set_beta1_power || set_beta2_power))
    if (int rc = train_rows_sync(h, nullptr, true)) return rc;
  if (set_beta1_power) { T->b1p = *set_beta1_power; T->rows_l2b1p = std::log2(T->b1p); }
  if (set_beta2_power) { T->b2p = *set_beta2_power; T->rows_l2b2p = std::log2(T->b2p); }
  if (set_step) T->step = (uint32_t)*set_step;
  if (beta1_power) *beta1_power = T->b1p;
  if (beta2_power) *beta2_power = T->b2p;
  if (step) *step = (int64_t)T->step;
  return COPER_OK;
}

}  // extern "C"

// ---- synchronised batch statistics: the backward in phases (include/coper_hip.h).  coper_train_sync_begin is
// train_step_impl up to the first batch-wide sum (SyncReq); every coper_train_sync_next folds the ranks' shares of that sum in ascending
// rank and runs on to the next one.  Between the calls the step is TrainState::open: the begin call's arguments and the StepCarry.
namespace {

// coper_train_sync_next by the exchange it follows (OpenStep::phase 1..4): the ranks' shares of that exchange's sum are folded into
// `fold_into`, the stages [from, to) run, this rank's share of the next sum is handed out from `hand_out` (null: the step is complete).
// (The begin call is [ConvFilters, Bn1) and hands out bn1_fwd_sums.)
struct SyncCut { Stage from, to; double* (Step::*fold_into)() const; double* (Step::*hand_out)() const; };
const SyncCut kSyncCuts[4] = {
    // Conv1BN's statistics over B_global P positions, ReLU, dropout, the dense layer; FCBN's column sums of this rank's rows
    {Stage::Bn1, Stage::Fcbn, &Step::bn1_fwd_sums, &Step::fcbn_fwd_sums},
    // FCBN over B_global samples, the scorer with the loss and its backward; FCBN's backward sums of this rank's rows
    {Stage::Fcbn, Stage::FcbnBwd, &Step::fcbn_fwd_sums, &Step::fcbn_bwd_sums},
    // dz from the whole batch's sums, the dense layer's backward, the generators' chains; Conv1BN's backward sums of this rank's rows
    {Stage::FcbnBwd, Stage::Bn1Bwd, &Step::bwd_all_sums, &Step::bn1_bwd_sums},
    // Conv1BN's backward from the whole batch's sums, the conv's, the filters'
    {Stage::Bn1Bwd, Stage::End, &Step::bwd_all_sums, nullptr}};
// the doubles exchange `phase` carries (1, 4: Conv1BN's channels; 2, 3: FCBN's features; 5: the step is complete)
inline int64_t sync_part_doubles(const Dims& dm, int phase) { return phase > 4 ? 0 : 2 * (int64_t)((phase == 1 || phase == 4) ? dm.C : dm.d); }

}  // namespace

extern "C" {

COPER_API int coper_train_sync_begin(coper_handle* h, const int64_t* e1, const int64_t* rel, const int32_t* lookup, const float* labels, int64_t B,
                                     int64_t L, int64_t B_global, int64_t sample_offset, int32_t rows, double* part_out, int64_t part_cap,
                                     int64_t* n_out, float* loss_out, void* stream) {
  const SyncReq q{B_global, sample_offset, rows, part_out, part_cap, n_out};
  return train_step_impl(h, e1, rel, lookup, labels, B, L, loss_out, stream, rows == 1 ? StepKind::RowsBackward : StepKind::Backward, nullptr, nullptr,
                         CsrLabels(), &q);
}

COPER_API int coper_train_sync_begin_csr(coper_handle* h, const int64_t* e1, const int64_t* rel, const int64_t* lab_indptr, const int64_t* lab_idx,
                                         const int64_t* lab_row, int64_t n_rows, int64_t B, int64_t B_global, int64_t sample_offset,
                                         double* part_out, int64_t part_cap, int64_t* n_out, float* loss_out, void* stream) {
  if (!h) return COPER_EINVAL;
  if (!lab_indptr) return fail(h, COPER_EINVAL, "coper_train_sync_begin_csr: bad argument (lab_indptr is NULL)");
  const SyncReq q{B_global, sample_offset, 0, part_out, part_cap, n_out};
  return train_step_impl(h, e1, rel, nullptr, nullptr, B, h->dm.E, loss_out, stream, StepKind::Backward, nullptr, nullptr,
                         CsrLabels{lab_indptr, lab_idx, lab_row, n_rows}, &q);
}

COPER_API int coper_train_sync_next(coper_handle* h, const double* parts_in, int32_t G, double* part_out, int64_t part_cap, int64_t* n_out,
                                    void* stream) {
  if (!h) return COPER_EINVAL;
  TrainState* T = (TrainState*)h->train;
  if (!T) return fail(h, COPER_ESTATE, "coper_train_sync_next: call coper_train_init first");
  const int ph = T->sync_phase();
  if (!ph) return fail(h, COPER_ESTATE, "coper_train_sync_next: no synchronised step is open (coper_train_sync_begin opens one)");
  if (G < 1) return fail(h, COPER_EINVAL, "coper_train_sync_next: G < 1");
  if (!parts_in || !aligned8(parts_in) || !n_out) return fail(h, COPER_EINVAL, "coper_train_sync_next: parts_in must be an 8-byte aligned device buffer, n_out not NULL");
  const Dims& dm = h->dm;
  const int64_t n_in = sync_part_doubles(dm, ph), n_next = sync_part_doubles(dm, ph + 1);
  if (n_next && (!part_out || !aligned8(part_out))) return fail(h, COPER_EINVAL, "coper_train_sync_next: part_out must be an 8-byte aligned device buffer");
  if (part_cap < n_next) return fail(h, COPER_EINVAL, "coper_train_sync_next: part_cap is below the doubles this call hands out (coper_train_sync_part_len holds every call's)");
  COPER_HIP_TRY(h, hipSetDevice(h->cfg.device));
  hipStream_t const s = (hipStream_t)stream;
  T->open.phase = 0;      // (a call that fails leaves no step open: what it left half done is no state to go on from)
  int rc;
  Step st = open_resume(h, T, T->open.args, s, &rc);
  if (rc) return rc;
  st.sync_sums = T->sync_sums.get();
  const SyncCut& cut = kSyncCuts[ph - 1];
  hipLaunchKernelGGL(k_tr_fold_parts, grid1d(n_in), dim3(256), 0, s, parts_in, (int)G, (int)n_in, (st.*cut.fold_into)());
  if ((rc = st.run(cut.from, cut.to))) return rc;
  if ((rc = st.join_sides("coper_train_sync_next"))) return rc;
  *n_out = 0;
  if (cut.hand_out && (rc = sync_hand_out(h, s, (st.*cut.hand_out)(), n_next, part_out, n_out))) return rc;
  COPER_HIP_TRY(h, hipGetLastError());
  T->open.carry = st;      // (the StepCarry part)
  if (ph < 4) { T->open.phase = ph + 1; return COPER_OK; }
  // complete: the handle is where coper_train_backward / coper_train_rows_backward leaves it
  finish_backward(h, T, st.kind, st.B, st.L);
  T->open = OpenStep();
  return COPER_OK;
}

COPER_API int coper_train_sync_phase(const coper_handle* h) {
  if (!h) return -COPER_EINVAL;
  const TrainState* T = (const TrainState*)h->train;
  return T ? T->sync_phase() : -COPER_ESTATE;
}

COPER_API int64_t coper_train_sync_part_len(const coper_handle* h) {
  if (!h) return -COPER_EINVAL;
  return 2 * (int64_t)std::max(h->dm.C, h->dm.d);
}

}  // extern "C"

// ---- entity-sharded training (include/coper_hip.h, "Entity-sharded training")
namespace {

// the sharded state of a call `what` that the state machine expects at `phase`; null (with the status in *rc) otherwise
static TrainState* shard_state(coper_handle* h, const char* what, int phase, int* rc) {
  TrainState* T = (TrainState*)h->train;
  if (!T) { *rc = fail(h, COPER_ESTATE, std::string(what) + ": call coper_train_init_sharded first"); return nullptr; }
  if (!T->sharded) { *rc = fail(h, COPER_ESTATE, std::string(what) + ": not an entity-sharded state (coper_train_init_sharded)"); return nullptr; }
  if (phase >= 0 && T->open.phase != phase) {
    *rc = fail(h, COPER_ESTATE, std::string(what) + ": out of order: the next call of this step is " + kShardCall[T->open.phase]);
    return nullptr;
  }
  return T;
}

// Deferred rows on a shard: the two row lists at `need` = B (L + 1) entries or more, in front of the score call's list.  The list of the
// step before has had its re-zero (the forward call of this step), so nothing of the old buffers is owed anything.
static int shard_rows_grow(coper_handle* h, TrainState* T, int64_t need, hipStream_t s) {
  if (need <= T->rows_cap) return COPER_OK;
  int rc;
  COPER_HIP_TRY(h, hipStreamSynchronize(s));
  T->rows_cap = 0;
  if ((rc = T->rows_list[0].alloc(h, (size_t)need, "deferred-row list")) || (rc = T->rows_list[1].alloc(h, (size_t)need, "deferred-row list"))) return rc;
  COPER_HIP_TRY(h, hipMemsetAsync(T->rows_count, 0, 2 * sizeof(int32_t), s));
  T->rows_cap = need;
  return COPER_OK;
}

// sh_e1 / sh_rel / sh_iota at B entries or more; sh_iota is filled where it grows
static int shard_ids_grow(coper_handle* h, TrainState* T, int64_t B, hipStream_t s) {
  if (B <= T->sh_cap) return COPER_OK;
  int rc;
  COPER_HIP_TRY(h, hipStreamSynchronize(s));
  T->sh_cap = 0;
  if ((rc = T->sh_e1.alloc(h, (size_t)B, "sharded step ids")) || (rc = T->sh_rel.alloc(h, (size_t)B, "sharded step ids")) ||
      (rc = T->sh_iota.alloc(h, (size_t)B, "sharded step ids")))
    return rc;
  T->sh_cap = B;
  hipLaunchKernelGGL(k_shard_iota, grid1d(B), dim3(256), 0, s, T->sh_iota.get(), B);
  return COPER_OK;
}

}  // namespace

extern "C" {

COPER_API int coper_train_sharded(const coper_handle* h) {
  if (!h) return -COPER_EINVAL;
  const TrainState* T = (const TrainState*)h->train;
  return T ? (T->sharded ? 1 : 0) : -COPER_ESTATE;
}

// out[b] = ent_emb[e1[b]] for the ids this handle holds, a zero row for every other: an addend of the all-reduce that forms e1_rows.
// Reads the registered table as it stands (no coper_prepare needed: the step before has just changed it).
COPER_API int coper_train_shard_gather(coper_handle* h, const int64_t* e1, int64_t B, float* rows_out, void* stream) {
  if (!h) return COPER_EINVAL;
  int rc = COPER_OK;
  TrainState* T = shard_state(h, "coper_train_shard_gather", -1, &rc);
  if (!T) return rc;
  if (!e1 || !rows_out || B <= 0) return fail(h, COPER_EINVAL, "coper_train_shard_gather: bad argument");
  COPER_HIP_TRY(h, hipSetDevice(h->cfg.device));
  if (!T->rows_deferred) return launch_gather_entities(h, e1, B, rows_out, (hipStream_t)stream);
  // deferred rows: the table may hold a row several updates behind -- the row as of the current update, formed in
  // registers; nothing of the table, the slots or the words is written
  const RowTables t = row_tables(h, T);
  hipLaunchKernelGGL(k_shard_gather_current, rows_grid(B), dim3(256), 0, (hipStream_t)stream, t, row_catch_up_args(T), e1, B, (int64_t)h->cfg.shard_lo,
                     (t.vec && ((uintptr_t)rows_out & 15) == 0) ? 1 : 0, rows_out);
  prof_count(h, "train.rows.gather_current");
  COPER_HIP_TRY(h, hipGetLastError());
  return COPER_OK;
}

COPER_API int coper_train_shard_forward(coper_handle* h, const int64_t* e1, const int64_t* rel, const float* e1_rows, int64_t B, float* h_out,
                                        void* stream) {
  if (!h) return COPER_EINVAL;
  int rc = COPER_OK;
  TrainState* T = shard_state(h, "coper_train_shard_forward", SHP_FORWARD, &rc);
  if (!T) return rc;
  if (!e1 || !rel || !e1_rows || B <= 0) return fail(h, COPER_EINVAL, "coper_train_shard_forward: bad argument");
  if ((rc = check_batch_limits(h, T, "coper_train_shard_forward", B, h->dm.n_local))) return rc;
  COPER_HIP_TRY(h, hipSetDevice(h->cfg.device));
  hipStream_t const s = (hipStream_t)stream;
  if ((rc = shard_ids_grow(h, T, B, s))) return rc;
  COPER_HIP_TRY(h, hipMemcpyAsync(T->sh_e1, e1, sizeof(int64_t) * (size_t)B, hipMemcpyDeviceToDevice, s));
  COPER_HIP_TRY(h, hipMemcpyAsync(T->sh_rel, rel, sizeof(int64_t) * (size_t)B, hipMemcpyDeviceToDevice, s));
  // the step's arguments, over the state's copy of the ids: a fused step's (StepKind::Step); the plan names the handle's own rows for the
  // tables.  No labels yet and L is num_ent: the score call amends them.
  StepArgs a;
  a.kind = StepKind::Step; a.s = s; a.e1 = T->sh_e1.get(); a.rel = T->sh_rel.get(); a.B = B; a.L = (int64_t)h->dm.E;
  a.img_rows = e1_rows;
  a.plan = plan_scorer(h, T, nullptr, CsrLabels(), B);
  Step st(h, T, a);
  if ((rc = st.grow_workspaces())) return rc;
  if (st.rows && (rc = rows_wrap_guard(h, T, s))) return rc;
  T->pending = false;
  st.zero_accumulators();      // (deferred rows: the two tables' gradients are left out ...)
  if (st.rows && T->rows_cap) rows_rezero_launch(h, T, s);      // (... the rows the step before listed are zeroed, their claim bits cleared)
  if (st.lk && (rc = st.group_for_lookup())) return rc;
  if ((rc = st.run(Stage::ConvFilters, Stage::Score))) return rc;
  if (h_out) COPER_HIP_TRY(h, hipMemcpyAsync(h_out, T->hv, sizeof(float) * (size_t)st.nBd, hipMemcpyDeviceToDevice, s));
  COPER_HIP_TRY(h, hipGetLastError());
  a.img_rows = nullptr;      // (the caller's until this call returns; no later stage reads the input rows)
  T->open = OpenStep{a, st /* the StepCarry part */, SHP_SCORE};
  T->sh_stepped = true;
  return COPER_OK;
}

COPER_API int coper_train_shard_score_csr(coper_handle* h, const int64_t* lab_indptr, const int64_t* lab_idx, const int64_t* lab_row, int64_t n_rows,
                                          int64_t B, float* dh_part, double* loss_part, void* stream) {
  if (!h) return COPER_EINVAL;
  int rc = COPER_OK;
  TrainState* T = shard_state(h, "coper_train_shard_score_csr", SHP_SCORE, &rc);
  if (!T) return rc;
  if (T->rows_deferred)      // (the phase stays "score expected": coper_train_shard_score_lookup may follow)
    return fail(h, COPER_EUNSUPPORTED, "coper_train_shard_score_csr: deferred-rows mode (coper_train_defer_rows): a 1-vs-all step has a gradient in every row");
  if (!lab_indptr || !lab_idx || !dh_part || !loss_part || B <= 0 || n_rows < 0 || (!lab_row && n_rows != B))
    return fail(h, COPER_EINVAL, "coper_train_shard_score_csr: bad argument (lab_row == NULL needs n_rows == B)");
  if (B != T->open.args.B) return fail(h, COPER_EINVAL, "coper_train_shard_score_csr: B is not the forward call's");
  COPER_HIP_TRY(h, hipSetDevice(h->cfg.device));
  hipStream_t const s = (hipStream_t)stream;
  StepArgs a = T->open.args;      // (amended on a copy: a call that fails leaves the open step as the forward call left it)
  a.lookup = nullptr; a.labels = nullptr; a.L = (int64_t)h->dm.E;
  a.csr = CsrLabels{lab_indptr, lab_idx, lab_row, n_rows};
  a.plan = plan_scorer(h, T, nullptr, a.csr, B);
  Step st = open_resume(h, T, a, s, &rc);
  if (rc) return rc;
  // the chunk loop over the own rows: d(pred_bias), d(ent_emb), the chunk shares of dh in ascending chunk order, the loss shares onto the
  // zeroed sum (Stage::ScorerBwd has nothing left to do behind it)
  if ((rc = st.run(Stage::Score, Stage::FcbnBwdSums))) return rc;
  COPER_HIP_TRY(h, hipMemcpyAsync(dh_part, T->dh, sizeof(float) * (size_t)st.nBd, hipMemcpyDeviceToDevice, s));
  COPER_HIP_TRY(h, hipMemcpyAsync(loss_part, st.red.loss(), sizeof(double), hipMemcpyDeviceToDevice, s));
  COPER_HIP_TRY(h, hipGetLastError());
  T->open = OpenStep{a, st /* the StepCarry part */, SHP_BACKWARD};
  return COPER_OK;
}

COPER_API int coper_train_shard_score_lookup(coper_handle* h, const int32_t* lookup, const float* labels, int64_t B, int64_t L, float* dh_part,
                                             double* loss_part, void* stream) {
  if (!h) return COPER_EINVAL;
  int rc = COPER_OK;
  TrainState* T = shard_state(h, "coper_train_shard_score_lookup", SHP_SCORE, &rc);
  if (!T) return rc;
  if (!lookup || !labels || !dh_part || !loss_part || B <= 0 || L <= 0) return fail(h, COPER_EINVAL, "coper_train_shard_score_lookup: bad argument");
  if (B != T->open.args.B) return fail(h, COPER_EINVAL, "coper_train_shard_score_lookup: B is not the forward call's");
  if (B * (L + 1) > 0x7fffffff || h->dm.E > 0x7fffffff)
    return fail(h, COPER_EINVAL, "coper_train_shard_score_lookup: ordered rows: B * (L + 1) ids and num_ent must fit 31 bits");
  COPER_HIP_TRY(h, hipSetDevice(h->cfg.device));
  hipStream_t const s = (hipStream_t)stream;
  // d(loss)/d(scores) [B, L]: grown here, alone -- the other workspaces hold what the forward call left for the backward call
  if ((size_t)T->capB * (size_t)L > T->ds.size()) {
    COPER_HIP_TRY(h, hipStreamSynchronize(s));
    if ((rc = T->ds.alloc(h, (size_t)T->capB * (size_t)L, "training workspace"))) return rc;
  }
  if (L > T->capL) T->capL = L;
  StepArgs a = T->open.args;      // (amended on a copy, as the CSR score call)
  a.lookup = lookup; a.labels = labels; a.L = L; a.csr = CsrLabels();
  a.plan = plan_scorer(h, T, lookup, a.csr, B);
  Step st = open_resume(h, T, a, s, &rc);
  if (rc || (rc = ord_grow(h, T, B * (L + 1), s))) return rc;
  if (st.rows && (rc = shard_rows_grow(h, T, B * (L + 1), s))) return rc;
  // (deferred rows: the sort and the heads first -- the owned rows of the list are what is caught up, in front of the scorer that reads them)
  if (st.rows) st.shard_rows_list_catch_up();
  // the owned entries' scores, loss shares and ds, then d(pred_bias), d(ent_emb) by sorted segments over the own rows, and this shard's share of dh
  if ((rc = st.run(Stage::Score, Stage::FcbnBwdSums))) return rc;
  COPER_HIP_TRY(h, hipMemcpyAsync(dh_part, T->dh, sizeof(float) * (size_t)st.nBd, hipMemcpyDeviceToDevice, s));
  COPER_HIP_TRY(h, hipMemcpyAsync(loss_part, st.red.loss(), sizeof(double), hipMemcpyDeviceToDevice, s));
  COPER_HIP_TRY(h, hipGetLastError());
  T->open = OpenStep{a, st /* the StepCarry part */, SHP_BACKWARD};
  return COPER_OK;
}

COPER_API int coper_train_shard_backward(coper_handle* h, const float* dh_parts, const double* loss_parts, int32_t G, float* loss_out,
                                         double* sumsq_part, void* stream) {
  if (!h) return COPER_EINVAL;
  int rc = COPER_OK;
  TrainState* T = shard_state(h, "coper_train_shard_backward", SHP_BACKWARD, &rc);
  if (!T) return rc;
  if (!dh_parts || !loss_parts || !sumsq_part || G < 1) return fail(h, COPER_EINVAL, "coper_train_shard_backward: bad argument");
  COPER_HIP_TRY(h, hipSetDevice(h->cfg.device));
  hipStream_t const s = (hipStream_t)stream;
  Step st = open_resume(h, T, T->open.args, s, &rc);      // (with the score call's labels: L is what its loss is a mean over)
  if (rc) return rc;
  // dh and the loss: the ranks' shares in ascending rank
  const int64_t nBd = st.nBd;
  const int vec = (nBd & 3) == 0 && (((uintptr_t)dh_parts | (uintptr_t)T->dh.get()) & 15) == 0;
  hipLaunchKernelGGL(k_shard_fold_parts, dim3((unsigned)std::min<int64_t>(((vec ? nBd / 4 : nBd) + 255) / 256, 2048)), dim3(256), 0, s, dh_parts, (int)G, nBd,
                     vec, T->dh.get(), loss_parts, st.red.loss());
  // (the mean is over the labels of the score call that ran: B num_ent of a 1-vs-all step, B L of a sampled one)
  if (loss_out) hipLaunchKernelGGL(k_tr_store_loss, dim3(1), dim3(1), 0, s, st.red.loss(), 1.0 / ((double)st.B * (double)st.L), loss_out);
  // (the conv backward: the owned e1 rows onto what the score call stored in d(ent_emb))
  if ((rc = st.run(Stage::FcbnBwdSums, Stage::End))) return rc;
  // the squared norm of this shard's table gradients, in the fixed order of the slab's fold, into its own double
  if (st.rows) {
    // deferred rows: every row off the step's list has a zero gradient -- the listed rows' squares in partial sums of ORD_SUMSQ_ROWS list
    // positions (exact zeros behind the list's end), folded in the slab's fixed order (the slab holds them: the score call sized it)
    const int pv = T->rows_prev;
    const int64_t parts = std::max<int64_t>((std::min<int64_t>(st.B * (st.L + 1), rows_held(h, T)) + ORD_SUMSQ_ROWS - 1) / ORD_SUMSQ_ROWS, 1);
    hipLaunchKernelGGL(k_rows_sumsq_ord, dim3((unsigned)parts), dim3(256), 0, s, row_tables(h, T), (const int32_t*)T->rows_list[pv].get(),
                       (const int32_t*)(T->rows_count + pv), T->det_slab.get());
    hipLaunchKernelGGL(k_tr_fold_det, dim3(1), dim3(256), 0, s, T->det_slab.get(), 1, parts, sumsq_part, 0);
    prof_count(h, "train.order.sumsq");
  } else {
  TrainTensors tt;
  const int np = train_tensors(h, T, LeafSet::Tables, GradSrc::Buffers, nullptr, nullptr, false, tt);
  sumsq_det_launch(T, s, tt, np, sumsq_part);
  }
  COPER_HIP_TRY(h, hipGetLastError());
  T->open.carry = st;      // (the StepCarry part)
  T->step += 1;
  T->open.phase = SHP_APPLY;
  return COPER_OK;
}

COPER_API int coper_train_shard_apply(coper_handle* h, const double* sumsq_parts, int32_t G, void* stream) {
  if (!h) return COPER_EINVAL;
  int rc = COPER_OK;
  TrainState* T = shard_state(h, "coper_train_shard_apply", SHP_APPLY, &rc);
  if (!T) return rc;
  if (!sumsq_parts || G < 1) return fail(h, COPER_EINVAL, "coper_train_shard_apply: bad argument");
  if (G > TG_SUMSQ_SLOTS - 1) return fail(h, COPER_EUNSUPPORTED, "coper_train_shard_apply: more shards than squared-norm slots (63)");
  COPER_HIP_TRY(h, hipSetDevice(h->cfg.device));
  hipStream_t const s = (hipStream_t)stream;
  h->prepared = false;   // the variables change: per-relation caches, fragment images and folded BN go stale
  // (the slots are zero since the forward call's zero list: nothing of a deterministic step adds to them)
  // (the looked-up table's rows by the forward call's snapshot: an evaluation may have grouped since)
  double* const ssq = T->red_layout().sumsq_slots();
  TrainTensors tt;
  int np = train_tensors(h, T, LeafSet::Small, GradSrc::Buffers, nullptr, T->step_rel_count.get(), false, tt);
  sumsq_det_launch(T, s, tt, np, ssq);
  hipLaunchKernelGGL(k_shard_place_sumsq, dim3(1), dim3(64), 0, s, sumsq_parts, (int)G, ssq);
  if (T->rows_deferred) {
    // deferred rows: k_tr_amsgrad over the small leaves, k_rows_update over the step's list -- both read the slots as placed above (slot
    // 0, then the G shares in index order) -- and the listed rows' words say "current as of this update"
    const coper_train_config& tc = T->cfg;
    const int pv = T->rows_prev;
    np = train_tensors(h, T, LeafSet::Small, GradSrc::Buffers, nullptr, T->step_rel_count.get(), true, tt);
    const float lr_t = amsgrad_launch(T, s, tt, np, 1.0);
    prof_count(h, "train.amsgrad.leaves", np);
    hipLaunchKernelGGL(k_rows_update, rows_grid(T->rows_cap), dim3(256), 0, s, row_tables(h, T), (const int32_t*)T->rows_list[pv].get(),
                       (const int32_t*)(T->rows_count + pv), (const double*)ssq, tc.clip_norm, lr_t, tc.beta1, tc.beta2, tc.epsilon, 1.0, T->rows_now + 1);
    prof_count(h, "train.rows.update");
  } else {
  np = train_tensors(h, T, LeafSet::All, GradSrc::Buffers, nullptr, T->step_rel_count.get(), true, tt);      // (the only table of this call that carries wmax)
  amsgrad_launch(T, s, tt, np, 1.0);
  }
  COPER_HIP_TRY(h, hipGetLastError());
  finish_update(T, tt.wmax != nullptr);
  T->open.phase = SHP_FORWARD;
  return COPER_OK;
}

// ---- forward-only calls on a sharded state (include/coper_hip.h): coper_train_forward / _csr restricted to the handle's
// rows, in one call between steps.  Nothing of the state moves: no variable, moving statistic, gradient, slot, counter, row word or list.
static int shard_forward_only(coper_handle* h, const char* what, const bool sampled, const int64_t* e1, const int64_t* rel, const float* e1_rows, const int32_t* lookup,
                              const float* labels, int64_t L, const CsrLabels& csr, int64_t B, double* loss_part, float* pred, float* h_out,
                              void* stream) {
  if (!h) return COPER_EINVAL;
  int rc = COPER_OK;
  TrainState* T = shard_state(h, what, SHP_FORWARD, &rc);
  if (!T) return rc;
  const std::string w(what);
  if (!sampled && T->rows_deferred)
    return fail(h, COPER_EUNSUPPORTED, w + ": deferred-rows mode (coper_train_defer_rows): 1-vs-all scores read every row; " +
                                       "coper_train_shard_forward_lookup serves the mode");
  if (!e1 || !rel || !e1_rows || !loss_part || B <= 0) return fail(h, COPER_EINVAL, w + ": bad argument");
  if (sampled) {
    if (!lookup || !labels || L <= 0) return fail(h, COPER_EINVAL, w + ": bad argument");
    if (B * (L + 1) > 0x7fffffff || h->dm.E > 0x7fffffff) return fail(h, COPER_EINVAL, w + ": B * (L + 1) ids and num_ent must fit 31 bits");
  } else if (!csr.indptr || !csr.idx || csr.n_rows < 0 || (!csr.row && csr.n_rows != B))
    return fail(h, COPER_EINVAL, w + ": bad argument (lab_row == NULL needs n_rows == B)");
  if ((rc = check_batch_limits(h, T, w, B, h->dm.n_local))) return rc;
  COPER_HIP_TRY(h, hipSetDevice(h->cfg.device));
  hipStream_t const s = (hipStream_t)stream;
  if ((rc = shard_ids_grow(h, T, B, s))) return rc;      // (the row numbers of the gathered input rows)
  StepArgs a;
  a.kind = StepKind::Forward; a.s = s; a.e1 = e1; a.rel = rel; a.lookup = lookup; a.labels = labels;
  a.B = B; a.L = sampled ? L : (int64_t)h->dm.E;
  a.pred_out = pred; a.h_out = h_out; a.csr = csr; a.img_rows = e1_rows;
  a.plan = plan_scorer(h, T, lookup, csr, B);
  a.plan.current = sampled && T->rows_deferred;
  Step st(h, T, a);
  if ((rc = st.grow_workspaces())) return rc;      // (between steps the workspaces are free: scratch)
  if (st.plan.current && st.plan.dh == DhRoute::Fused && st.plan.lds_fused > 160 * 1024)
    return fail(h, COPER_EUNSUPPORTED, w + ": deferred-rows mode: L is too large for the fused scorer's LDS with the rows' catch-up scalars");
  st.zero_forward_scratch();
  if (st.lk && (rc = st.group_for_lookup())) return rc;
  // (deferred rows: no sort, no list, no catch-up launch -- the CURRENT row loads; the list of the step before keeps its re-zero owed)
  if ((rc = st.run(Stage::ConvFilters, Stage::ScorerBwd))) return rc;
  COPER_HIP_TRY(h, hipMemcpyAsync(loss_part, st.red.loss(), sizeof(double), hipMemcpyDeviceToDevice, s));
  COPER_HIP_TRY(h, hipGetLastError());
  return COPER_OK;
}

COPER_API int coper_train_shard_forward_lookup(coper_handle* h, const int64_t* e1, const int64_t* rel, const float* e1_rows, const int32_t* lookup,
                                               const float* labels, int64_t B, int64_t L, double* loss_part, float* pred_part, float* h_out,
                                               void* stream) {
  return shard_forward_only(h, "coper_train_shard_forward_lookup", true, e1, rel, e1_rows, lookup, labels, L, CsrLabels(), B, loss_part, pred_part, h_out, stream);
}

COPER_API int coper_train_shard_forward_csr(coper_handle* h, const int64_t* e1, const int64_t* rel, const float* e1_rows, const int64_t* lab_indptr,
                                            const int64_t* lab_idx, const int64_t* lab_row, int64_t n_rows, int64_t B, double* loss_part,
                                            float* pred_local, float* h_out, void* stream) {
  return shard_forward_only(h, "coper_train_shard_forward_csr", false, e1, rel, e1_rows, nullptr, nullptr, 0, CsrLabels{lab_indptr, lab_idx, lab_row, n_rows}, B,
                            loss_part, pred_local, h_out, stream);
}

}  // extern "C"
