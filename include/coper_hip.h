/*
 * coper_hip.h -- C ABI of libcoper_hip.so: the MI355X (gfx950) CoPER-ConvE scoring engine.
 *
 * The reference (otiliastr/coper, CoPER_ConvE/qa_cpg) has NO FFI / plugin interface for this
 * path: the seam is a Python object protocol between run_cpg.py / metrics.py and models.py.
 * Each entry point below therefore cites the reference *Python* interface it replaces
 * (paths relative to CoPER_ConvE/qa_cpg/).  The reference-side binding a maintainer would add
 * is the ctypes stub shown in INTEGRATION.md (it is what coper_amd/_lib.py does).
 *
 * Conventions
 *   - plain C, no C++ exceptions cross the boundary; every call returns a coper_status.
 *   - all tensor arguments are DEVICE pointers owned by the caller (row-major, fp32 unless
 *     stated); ids are int64 like the reference batch contract (models.py:139-152), lookup
 *     indices int32.
 *   - every call is asynchronous on the hipStream_t it is given (passed as void* so that the
 *     header needs no HIP include); the handle's workspace is stream-ordered: use one handle
 *     per (GPU, stream).  A handle is not thread-safe.
 *   - parameters are BORROWED: the caller keeps the device buffers alive and must call
 *     coper_prepare() again after changing their contents (it rebuilds every derived cache).
 */
#ifndef COPER_HIP_H_
#define COPER_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(COPER_BUILD)
#define COPER_API __attribute__((visibility("default")))
#else
#define COPER_API
#endif

#define COPER_ABI_VERSION 3
#define COPER_MAX_CTX 8 /* max hidden layers of a g_MLP generator (models.py:44-54 loops over any number; no shipped YAML has more than 1) */

typedef enum coper_status {
  COPER_OK = 0,
  COPER_EINVAL = 1,    /* bad argument / ill-formed model_descriptors */
  COPER_EMISSING = 2,  /* a required parameter was never set */
  COPER_ESHAPE = 3,    /* parameter shape does not match the configuration */
  COPER_EHIP = 4,      /* HIP runtime error, text in coper_last_error() */
  COPER_ESTATE = 5,    /* call order violated (e.g. encode before prepare) */
  COPER_ENOMEM = 6,
  COPER_EUNSUPPORTED = 7
} coper_status;

typedef enum coper_score_mode {
  COPER_SCORE_F32 = 0,   /* entity table fp32, exact-f32 MFMA (v_mfma_f32_32x32x2_f32): parity mode */
  COPER_SCORE_BF16X3 = 1 /* "x3" (the name is round 2's): every fp32 operand split into two fp16 terms hi + lo, 3 fp16 MFMAs per
                          * product with fp32 accumulation.  Operands are first moved into fp16's window by exact powers of two
                          * (per table, per relation's weights, per packed batch of queries), so hi + lo carries 22 bits at any
                          * magnitude: logits within 2.5e-7 |h||E| of the fp32 chain; integer ranks ARE the fp32 chain's (the
                          * exact band, rank_band_kappa below), checked at run time by coper_band_audit */
  /* (a single-16-bit mode, ~2^-9 per product, cannot meet the 1e-3 logit gate of the path and is not part of the ABI) */
} coper_score_mode;

/* Mirrors the `model_descriptors` dict of ConvE.__init__ (models.py:98-130) -- only the keys
 * that influence inference -- plus what the build adds: (emb_h, emb_w) replacing the
 * hard-coded (10, d // 10) of models.py:261-262,355; the entity shard; the score precision. */
typedef struct coper_config {
  int32_t abi_version;          /* = COPER_ABI_VERSION */
  int32_t device;               /* HIP device ordinal */
  int64_t num_ent;              /* |E| (global)                          models.py:102 */
  int64_t num_rel;              /* R2 = 2|R| incl. _reverse relations    models.py:103 */
  int32_t ent_emb_size;         /* d <= 640 (COPER_EINVAL beyond: the count kernels hold a 128-query tile in LDS, whole up to
                                 * d = 320, in two halves of K up to 640)      models.py:104 */
  int32_t rel_emb_size;         /* r                                     models.py:105 */
  int32_t emb_h, emb_w;         /* image reshape, emb_h * emb_w == d     models.py:355 */
  int32_t conv_filter_height;   /* default 3                             models.py:109 */
  int32_t conv_filter_width;    /* default 3                             models.py:110 */
  int32_t conv_num_channels;    /* default 32                            models.py:111 */
  int32_t concat_rel;           /*                                       models.py:113 */
  int32_t do_parameter_lookup;  /* g_lookup                              models.py:107 */
  /* context_rel_conv / context_rel_out (models.py:114-115):
   *   n = -1 -> None (static parameter), n = 0 -> [] (g_linear), n > 0 -> hidden sizes (g_MLP) */
  int32_t n_ctx_conv;
  int32_t ctx_conv[COPER_MAX_CTX];
  int32_t n_ctx_out;
  int32_t ctx_out[COPER_MAX_CTX];
  int32_t context_rel_use_batch_norm; /*                                 models.py:117 */
  float bn_epsilon;             /* 1e-3 = tf.layers.batch_normalization default */
  int64_t shard_lo, shard_hi;   /* entity rows [lo, hi) held by this handle; [0, num_ent) = unsharded */
  int32_t score_mode;           /* coper_score_mode */
  /* COPER_SCORE_BF16X3: kappa, the relative half-width of the exact band.  A comparison of a competitor's logit with the
   * target's that is closer than
   *       tau_q = 2 (kappa (|h_q| max|E_e| + 8 max|pred_bias|) + 2^-25 sqrt(d) (max|E_e| 2^-e_h + |h_q| 2^-e_E))
   * is decided by the fp32 chain of COPER_SCORE_F32 instead of the mode's own arithmetic (integer ranks: metrics.py:44-50).
   * 0 = the library default 1e-6: four to five times the largest error measured over 6e6 - 3e8 logits at every operand scale
   * (tests/test_gpu_scale.py: <= 0.24 kappa (...) ), for logits dominated by their products and by pred_bias alike (the
   * weight 8: an accumulation that runs at the magnitude of the bias rounds to ulps of it at every step).  The last term is
   * rigorous: elements more than 2^17 below their class maximum lose bits to fp16's subnormals (e_h, e_E: the powers of
   * two of the packed batch and of the table).  kappa itself is EMPIRICAL -- the proven bound of the split and of fp32
   * accumulation in any order is 3 * 2^-22 + 2 (48 ceil(d/16) + 1) 2^-24 = 7.5e-5 at d = 200 -- which is why every count
   * launch can audit it (coper_band_audit).  Larger = more pairs re-scored by the chain, proportionally. */
  float rank_band_kappa;
  /* COPER_SCORE_BF16X3: the entity planes hold ent_emb 2^e with e chosen so that this magnitude lands in [2^14, 2^15) of
   * fp16's range.  0 = the largest |ent_emb| element of the handle's own rows.  Entity shards of one table pass the table-wide
   * maximum (coper_amd/sharding.py all-reduces it) so that the mode's logits do not depend on the shard layout; a value below
   * the shard's own maximum is refused by coper_prepare.  The same magnitude bounds the encoder's INPUT rows: rows handed in through
   * `e1_rows` (an entity-sharded evaluation passes rows of other shards) must not exceed it in any element -- the conv activations'
   * power of two and the fp16 image planes of the fused encoder are derived from it; larger elements are clamped to fp16's range
   * and `h` saturates silently.  coper_amd/sharding.py keeps the table-wide maximum agreed on every chunk. */
  float x3_ent_absmax;
  /* COPER_SCORE_BF16X3: which count launches carry the band audit (coper_band_audit).  0 = the library default: the first
   * launch after coper_prepare and every 8th from there (+3 us per 0.5 ms pass), every launch of more than 2^31 logits;
   * n > 0: every n-th launch; negative: never.  Launches recorded into a hipGraph carry the audit only with n = 1. */
  int32_t band_audit_period;
  /* What the handle is built for (round 6; 0 = COPER_ROLE_BOTH = every earlier caller).  An entity-sharded evaluation runs the
   * rank's share of the encoder and its count over the rank's entity rows on TWO streams (coper_amd/sharding.py: steps 1 - 2 of
   * chunk n + 1 under chunk n's count launch), which one handle's workspace cannot serve: it creates one handle per role over the
   * SAME parameter tensors.  COPER_ROLE_ENCODE builds no entity planes (4 x |E_local| d 2 + |E_local| d 4 bytes) and refuses the
   * scoring entry points; COPER_ROLE_SCORE evaluates no generator and caches no W_r (R2 F d 4 bytes: 12.8 GB for the 10M-entity
   * config) and refuses coper_encode / coper_encode_rank / training.  Everything both roles derive (folded BN, the band constants,
   * the powers of two of split16.h) is the same values on both. */
  int32_t role;                 /* coper_role */
  /* The generated dense weights W_r of the relations r with r mod rel_mod_world == rel_mod_rank ONLY (round 6; 0 or 1 = all of
   * them).  An entity-sharded evaluation splits its encoder by relation -- rank g of G encodes the queries whose relation id is
   * g mod G (coper_amd/sharding.py step 2) -- so its encoder handle needs R2 / G weight sets, not R2: 1.6 GB instead of 12.8 GB per
   * rank for the 10M-entity config at G = 8.  Everything small that is derived per relation (conv filters, biases, the powers
   * of two of split16.h) is still built for every relation, from the same values: h[b] is the same bits as on a handle that holds
   * all weight sets.  A query whose relation the handle does not hold is encoded with another relation's weights and COUNTED
   * (coper_check_ids).  COPER_SCORE_BF16X3 with generated dense weights (context_rel_out) on the fused encoder only:
   * COPER_EUNSUPPORTED from coper_prepare otherwise; no training. */
  int32_t rel_mod_world;
  int32_t rel_mod_rank;
  /* How the handle applies a GENERATED dense layer at inference (0 = COPER_DENSE_CACHED = every earlier caller; the field took the
   * last reserved slot: the struct size and COPER_ABI_VERSION are unchanged).
   *   COPER_DENSE_CACHED: coper_prepare evaluates the generator once per relation and caches every W_r as MFMA images (R2 F d 4 bytes:
   *     1.96 GB at FB15k-237 shapes); the encoder streams them.  Right for many queries over frozen weights.
   *   COPER_DENSE_FACTORED: no W_r is ever formed.  coper_prepare keeps the [R2, K] context of the fc_weights generator and packs its
   *     last projection P [K, F d] once (2 K d F 2 bytes); an encode computes  T[b] = x[b] P  (one GEMM [B, F] x [F, K d], in chunks of
   *     a fixed number of queries so that T stays below 256 MB) and  h_pre[b, k] = sum_rho ctx[rel_b, rho] T[b, rho d + k] + fc_b[rel_b, k].
   *     Right where the weights have just moved (an evaluation between training steps: coper_prepare costs a pack of P, not R2 weight
   *     sets) or the handle only ever sees small batches.  Everything downstream of h -- coper_score_all, coper_rank, the exact band,
   *     the audit, top-k -- is the same code.  h[b] stays a pure function of (e1[b], rel[b]) and the parameters (the power of two of x,
   *     the K slices and the GEMM variant are chosen from the configuration at coper_prepare, never from the batch), but it is NOT
   *     bit-equal to a cached handle's h: the sums run in another order.  Ranks are the fp32 chain's ranks on the handle's own h.
   *     Accepted for COPER_SCORE_BF16X3 with context_rel_out set and do_parameter_lookup off, role BOTH or ENCODE; COPER_EUNSUPPORTED from
   *     coper_create for plain ConvE, g_lookup, COPER_SCORE_F32, COPER_ROLE_SCORE and rel_mod_world > 1 (there is no cache to split).
   *     coper_encode / coper_encode_rank on a stream that is being captured return COPER_EUNSUPPORTED.  Pending coper_stage_ids_next /
   *     coper_post_i32_next jobs are served by launches of their own, a pending coper_group_next is dropped. */
  int32_t dense_mode;           /* coper_dense_mode */
} coper_config;

typedef enum coper_role { COPER_ROLE_BOTH = 0, COPER_ROLE_ENCODE = 1, COPER_ROLE_SCORE = 2 } coper_role;
typedef enum coper_dense_mode { COPER_DENSE_CACHED = 0, COPER_DENSE_FACTORED = 1 } coper_dense_mode;

typedef struct coper_handle coper_handle;

/* Replaces ConvE.__init__ / _create_variables shape logic (models.py:98-130, 203-336):
 * validates the configuration exactly as the reference derives its shapes.  No parameter
 * memory is allocated: parameters are borrowed through coper_set_param. */
COPER_API int coper_create(const coper_config* cfg, coper_handle** out);
COPER_API void coper_destroy(coper_handle* h);

/* Text of the last failure on this handle (never NULL).  With h == NULL: last coper_create failure. */
COPER_API const char* coper_last_error(const coper_handle* h);
COPER_API int coper_abi_version(void);

/* CRC-32C (Castagnoli) of a host buffer, continuing from `crc` (0 for a fresh one): the checksum of the TensorFlow
 * checkpoint files `tf.train.Saver` writes and reads (run_cpg.py:189,206,252; tensor_bundle.proto crc32c fields, the table
 * blocks of the .index file).  Host code (SSE4.2 crc32 instruction when the CPU has it): coper_amd/tf_bundle.py checks a
 * 500 MB checkpoint with it in well under a second, its NumPy form needs 65 MB/s. */
COPER_API uint32_t coper_crc32c(uint32_t crc, const void* data, uint64_t n);

/* Derived sizes (models.py:261-271): F = fc_input_size, Ho/Wo = conv output; n_local = shard_hi - shard_lo. */
COPER_API int coper_get_dims(const coper_handle* h, int64_t* F, int32_t* Ho, int32_t* Wo, int64_t* n_local);

/* Number of parameters the configuration requires and their leaf names / shapes, named as
 * the reference's TF variables: ent_emb, rel_emb, pred_bias, conv1_weights,
 * conv1_bias, fc_weights, fc_bias, "<name>/CPG/Projection<i>",
 * "<name>/CPG/Projection<i>/BatchNorm/{gamma,beta,moving_mean,moving_variance}",
 * "Conv1BN/...", "FCBN/...".  shape_out must hold 4 entries. */
COPER_API int coper_num_params(const coper_handle* h);
COPER_API int coper_param_spec(const coper_handle* h, int index, const char** leaf_name, int64_t* shape_out, int* ndim_out);

/* Replaces variable assignment / Saver.restore (models.py:203-336, run_cpg.py:205-206).
 * dev_ptr: fp32, contiguous, on cfg.device.  ent_emb / pred_bias are the LOCAL shard rows. */
COPER_API int coper_set_param(coper_handle* h, const char* leaf_name, const void* dev_ptr,
                    const int64_t* shape, int ndim);

/* coper_config.x3_ent_absmax after coper_create (a host that learns the table-wide maximum only when the parameters arrive:
 * coper_amd.models.ConvE.load_parameters, coper_amd/sharding.py).  The handle must be prepared (again) afterwards. */
COPER_API int coper_set_x3_ent_absmax(coper_handle* h, float absmax);

/* Builds everything inference derives from the parameters (re-run after any weight change):
 *   - BN (Conv1BN, FCBN, generator BNs) folded to per-channel affine   models.py:61-65,386-388,416-418
 *   - per-relation generated / looked-up conv filters, conv bias, dense weights, dense bias
 *     (ContextualParameterGenerator.generate / ParameterLookup.generate, models.py:56-76,90-94,
 *      338-352) evaluated once per relation id instead of once per sample
 *   - dense weights and the entity table re-laid out in MFMA-fragment-major order. */
COPER_API int coper_prepare(coper_handle* h, void* stream);

/* Pre-size the workspace so later calls with B <= max_queries and nnz <= max_filter_nnz do
 * not allocate (needed before hipGraph capture).  Optional: calls grow the workspace lazily. */
COPER_API int coper_reserve(coper_handle* h, int64_t max_queries, int64_t max_filter_nnz, void* stream);

/* Batch staging: the reference's placeholders hold int32 ids (e1, e2, rel: models.py:148-152; so do the indices a host
 * builds a CSR filter from), this ABI takes int64.  dst[i] = src[i] for n values; `src` may be device memory or PINNED,
 * device-mapped HOST memory (hipHostMalloc): the kernel then pulls the ids over PCIe itself -- one launch instead of a copy
 * engine transfer plus a widening pass.  No handle state is touched. */
COPER_API int coper_widen_ids(coper_handle* h, const int32_t* src, int64_t n, int64_t* dst, void* stream);

/* The same staging, overlapped: registers (src, n, dst) as a job the NEXT coper_encode / coper_encode_rank on this handle carries
 * out beside its encoder launch -- extra workgroups of that launch read the pinned batch over PCIe while the relation tiles
 * stream their weights (fewer tiles than CUs at the BASELINE shapes: they run on CUs that would idle), so the batch of pass
 * n + 1 arrives under pass n's kernels without a second stream.  dst must not be an array pass n itself reads (two staging
 * buffers, used alternately); configurations the fused encoder does not serve run the job as a launch of its own at the same
 * point.  Nothing is queued on a stream by this call; a later call replaces a job that has not run.  A pass that is being
 * captured into a hipGraph leaves the job pending for the next eager call (a replay must not repeat a read with the pointers
 * recorded at capture time). */
COPER_API int coper_stage_ids_next(coper_handle* h, const int32_t* src, int64_t n, int64_t* dst);

/* The way back: n int32 values (the ranks of a pass) from device memory to `dst`, which may be PINNED, device-mapped HOST
 * memory -- the kernel posts the writes over PCIe right behind the pass's last kernel (a copy-engine D2H on the same stream
 * starts ~12 us later on this runtime).  The host reads dst after synchronising with the stream. */
COPER_API int coper_copy_out_i32(coper_handle* h, const int32_t* src, int64_t n, int32_t* dst, void* stream);

/* The same copy, overlapped: registers (src, n, dst) as a job the NEXT call on this handle that groups a batch by relation
 * (coper_encode, coper_encode_rank, a training step of a parameter-lookup model) carries out beside its first launch, on that call's stream: the ranks of pass
 * n reach the host under pass n + 1's histogram instead of through a launch of their own behind pass n.  src must stay
 * unchanged until then (it is: the next pass writes its ranks in its third launch); the last pass of a loop is followed by
 * coper_copy_out_i32.  A later registration replaces a job that has not run; n == 0 cancels; a call that is being captured into
 * a hipGraph leaves the job to the next eager one.  Nothing is queued by this call. */
COPER_API int coper_post_i32_next(coper_handle* h, const int32_t* src, int64_t n, int32_t* dst);

/* The NEXT pass's grouping, overlapped.  Every pass starts by sorting its batch by relation (the reference instead materialises
 * per-query weights, models.py:350,412): two small launches that nothing else can overlap, 18 us of a 487 us pass at the BASELINE
 * shapes.  This call registers the id arrays of the pass that will FOLLOW the next one enqueued on this handle -- device addresses
 * (e1 / rel of that later coper_encode / coper_encode_rank call; have_e1_rows != 0: it will pass e1_rows, e1 is ignored), whose
 * contents are either there already or are what a coper_stage_ids_next job registered for the same launch will write there.  One
 * more workgroup of the next fused encoder launch then sorts that batch into a second set of grouping arrays while the relation
 * tiles stream their weights; the following coper_encode_rank call with exactly these pointers and B finds its grouping done and
 * starts with its encoder launch (a pending coper_post_i32_next job rides there instead).  Any other call in between (coper_encode
 * included: only a pass that writes ranks may run on a prepared grouping), a coper_prepare, a training step, a growing workspace
 * or a pass captured into a hipGraph drops the prepared grouping: the pass then groups itself as always.  The registration is for
 * the NEXT encode / encode_rank call only: a call that cannot carry it (captured into a hipGraph, a configuration the fused
 * encoder does not serve) drops it.  Nothing is queued by this call; B == 0 cancels.
 * THE GUARD.  The pointers identify the batch, not its contents: if the ids at those addresses are rewritten between the launch
 * that sorted them and the pass that consumes the sorting (the natural mistake with two staging buffers), that pass would encode
 * the ids that WERE there and rank them against the new e2 / filters.  So the consuming pass checks on the device: every tile
 * of its encoder launch compares the live (e1, rel) of each of its queries with what was sorted -- every query exactly once, its
 * loads beside the tile's own first loads -- and on ANY difference the pass's ranks are all written as COPER_RANK_STALE (negative:
 * no consumer can mistake them for ranks, which start at 1; n_equal / h of that call are undefined) and the pass is counted
 * (coper_stale_passes).  The caller ranks such a batch again with a plain call; coper_amd.metrics.ranking_and_hits and
 * bench.py do.  A stale grouping never reaches the ranks; a grouping that is not stale is never reported (tests/test_gpu_pipeline.py:
 * random interleavings of every registration, pass, prepare, training step, capture and workspace growth, ids rewritten at random). */
COPER_API int coper_group_next(coper_handle* h, const int64_t* e1, const int64_t* rel, int64_t B, int32_t have_e1_rows);

/* Row gather tf.nn.embedding_lookup(ent_emb, ids) (models.py:176) restricted to the shard:
 * out[b,:] = ent_emb[ids[b]] if shard_lo <= ids[b] < shard_hi else 0.  (Multi-GPU: sum over
 * ranks = the full gather.)  out: [B, d]. */
COPER_API int coper_gather_entities(coper_handle* h, const int64_t* ids, int64_t B, float* out, void* stream);

/* Replaces ConvE._create_predictions (models.py:354-426) in inference mode:
 * h_out[B, d] = predicted_e2_emb.  e1_rows: optional [B, d] pre-gathered ent_emb[e1] rows
 * (required when the shard does not hold every e1; NULL = gather locally). */
COPER_API int coper_encode(coper_handle* h, const int64_t* e1, const int64_t* rel, int64_t B,
                 const float* e1_rows, float* h_out, void* stream);

/* Replaces ConvE._compute_likelihoods(..., ent_indices=None) (models.py:428-437):
 * logits[B, n_local] = h . ent_emb_shard^T + pred_bias_shard  (no sigmoid). ld = row stride of logits. */
COPER_API int coper_score_all(coper_handle* h, const float* hvec, int64_t B, float* logits, int64_t ld, void* stream);

/* Replaces ConvE._compute_likelihoods(..., ent_indices=lookup) (models.py:438-443):
 * out[B, L] = h[b] . ent_emb[lookup[b,l]] + pred_bias[lookup[b,l]]; lookup holds GLOBAL ids,
 * entries outside the shard produce 0 (sum over ranks = full result). */
COPER_API int coper_score_lookup(coper_handle* h, const float* hvec, const int32_t* lookup, int64_t B, int64_t L,
                       float* out, void* stream);

/* Target scores, tgt: float [2 B].  tgt[b] = logit(b, e2[b]) in the mode's own arithmetic, bit-identical to the value
 * coper_score_all writes for that element (metrics.py:44); tgt[B + b] = the same logit by the fp32 chain of COPER_SCORE_F32
 * (equal to tgt[b] in that mode): what the x3 mode's exact band decides close comparisons against.  Entries whose e2 is not
 * in the shard are 0 in both halves: the sum over shards is the full result. */
COPER_API int coper_target_scores(coper_handle* h, const float* hvec, const int64_t* e2, int64_t B, float* tgt, void* stream);

/* out[b] = pred_bias_b + rows[b] . hvec[b] by the fp32 chain, for entity rows the caller holds (rows float [B, d], bias float
 * [B]): entity-sharded evaluation gathers ent_emb[e2] and pred_bias[e2] together with ent_emb[e1] in ONE all-reduce and
 * every rank then scores the targets from its copy -- no exchange of target logits (coper_amd/sharding.py; SURVEY 8(e)
 * step 1).  {out, out} is a valid `tgt` for coper_rank_counts. */
COPER_API int coper_score_rows(coper_handle* h, const float* hvec, const float* rows, const float* bias, int64_t B, float* out,
                               void* stream);

/* Replaces the host ranker loop of ranking_and_hits (metrics.py:44-50) without materialising
 * logits: for every query b over the shard's entities j, with the known-answer filter given
 * in CSR form (filt_idx[filt_indptr[b] .. filt_indptr[b+1]) = GLOBAL ids, sorted ascending;
 * the dense e2_multi mask of data.py:182-186 made sparse):
 *   n_greater[b] = #{ j != e2[b], j not filtered : logit(b,j) >  tgt[b] }
 *   n_equal[b]   = #{ j != e2[b], j not filtered : logit(b,j) == tgt[b] }
 * so that rank = 1 + sum_over_shards(n_greater) when tie-free (any value in
 * [1+n_greater, 1+n_greater+n_equal] under ties -- the reference's np.argsort is unstable).
 * n_equal may be NULL: ties are then not counted (the reference never computes them; saves one compare per
 * score) and rank = 1 + n_greater is the optimistic end of the band.
 * tgt: [2 B] global target scores (from coper_target_scores, summed over shards; or {t, t} from coper_score_rows): the count
 *   kernel of the x3 mode leaves every comparison closer than its own error (the band around tgt[b]) to the fp32 chain, which
 *   compares against tgt[B + b]: n_greater / n_equal of both modes are those of the fp32 chain on hvec.
 * filt_nnz = filt_indptr[B], passed from the host that built the CSR (sizes the launch).
 * k > 0 additionally returns the shard's top-k of the FILTERED row (target kept, like
 * metrics.py:46), order (score desc, id asc): topk_val [B,k] (-inf padded), topk_idx [B,k]
 * global ids (-1 padded).  k == 0: both may be NULL.  Not needed for ranks.  k <= 128 selects from
 * per-block maxima written by the count pass (no logits; workspace: one float per (32 entities, query) -- per (64 entities, query) on shards of 65,536 rows and more -- of a
 * query chunk + 32 floats per (k + filter entries)); otherwise logits are materialised chunk by chunk (<= 256 MiB). */
COPER_API int coper_rank_counts(coper_handle* h, const float* hvec, const float* tgt, const int64_t* e2,
                      const int64_t* filt_indptr, const int64_t* filt_idx, int64_t filt_nnz, int64_t B, int32_t k,
                      int32_t* n_greater, int32_t* n_equal, float* topk_val, int64_t* topk_idx,
                      void* stream);

/* Single-shard convenience: coper_target_scores + coper_rank_counts + rank = 1 + n_greater.
 * ranks: int32 [B]. */
COPER_API int coper_rank(coper_handle* h, const float* hvec, const int64_t* e2, const int64_t* filt_indptr,
               const int64_t* filt_idx, int64_t filt_nnz, int64_t B, int32_t* ranks, int32_t* n_equal,
               void* stream);

/* One evaluation batch end to end: coper_encode + coper_rank in one call -- what one `session.run` of the
 * reference's ranker loop computes (metrics.py:40-57).  h_out: optional float [B, d] (NULL: the embedding is
 * not needed; in the bf16x3 mode it then never exists in fp32 -- the dense finalize writes the operand planes
 * of the rank kernels directly).  Same results as the two calls, bit for bit.
 * Cost model of the filter: in the bf16x3 mode the workgroup that finalizes 32 consecutive queries also takes back their
 * known answers, the first 352 CSR entries of the block; entries beyond that (one (e1, rel) with 5,000 known tails) are
 * dealt over the whole chip by a second launch that costs ~2 us when no block needs it.  Callers have nothing to route. */
COPER_API int coper_encode_rank(coper_handle* h, const int64_t* e1, const int64_t* rel, const float* e1_rows,
                                const int64_t* e2, const int64_t* filt_indptr, const int64_t* filt_idx, int64_t filt_nnz,
                                int64_t B, float* h_out, int32_t* ranks, int32_t* n_equal, void* stream);

/* Answering a query: which entities complete (e1, rel, ?).  The reference has no such entry point -- its callers take the top of
 * `predictions` (models.py:183-192) on the host; coper_rank_counts' k > 0 side output needs a target and exempts it from the filter.
 * For every query b, over the entities j of the handle's shard that are NOT in the query's filter row (no entity is exempt: there is
 * no target), the k entries with the largest logit in (score desc, global id asc) order: topk_idx [B, k] global ids, topk_val [B, k]
 * logits; rows with fewer than k unfiltered entities are padded with (-inf, -1) like coper_rank_counts.
 *   query:   either (e1, rel, e1_rows) as coper_encode_rank takes them (hvec NULL), or hvec = finished h rows [B, d] (the others NULL);
 *   filter:  CSR of known answers, GLOBAL ids ascending per row, filt_nnz = filt_indptr[B]; all NULL / 0 = raw (unfiltered).
 * EXACT in both score modes: topk_val[b, i] is the logit of (b, topk_idx[b, i]) by the fp32 chain of COPER_SCORE_F32 -- the value
 * coper_score_all of an f32 handle writes for that element from the same h -- and the selected set and its order are that chain's,
 * bit for bit.  In COPER_SCORE_BF16X3 the matrix-core logits only PRUNE: block maxima select k + 4 + (filter entries) candidate
 * blocks, the candidates within tau_q (rank_band_kappa above) of the k-th largest x3 logit are re-scored by the chain and selected by
 * it; a query whose near-ties reach beyond the emitted blocks is served, in the same call, from chain logits of its whole row
 * (counted: coper_predict_stats).  h is what the handle's encoder produces, as for ranks.  No logits are materialised on the common
 * route (workspace: the block maxima of coper_rank_counts + 32 floats per (k + 4 + filter entries) and query + at most 64 MiB of rows
 * for unresolved queries); stream-ordered, no host synchronisation once the workspace has its size.
 * 1 <= k <= 128; larger k: COPER_EUNSUPPORTED (use coper_score_all).  k <= 0, B < 0, a half-given CSR, both or neither of
 * (e1 / rel, hvec): COPER_EINVAL.  B == 0: COPER_OK, nothing launched.  Not prepared: COPER_ESTATE.  COPER_ROLE_ENCODE handles have
 * no entity table: COPER_EUNSUPPORTED.  Out-of-range e1 / rel are clamped and counted (coper_check_ids).  Entity shards return the
 * top-k of THEIR rows with global ids: coper_amd.sharding.merge_topk over the shards is the global answer.  Not for hipGraph capture. */
COPER_API int coper_predict_topk(coper_handle* h, const int64_t* e1, const int64_t* rel, const float* e1_rows, const float* hvec,
                                 const int64_t* filt_indptr, const int64_t* filt_idx, int64_t filt_nnz, int64_t B, int32_t k,
                                 float* topk_val, int64_t* topk_idx, void* stream);
/* What coper_predict_topk did since the last reset (synchronises the stream): queries answered; of those (COPER_SCORE_BF16X3) the
 * UNRESOLVED ones, served from chain logits of their whole row; candidates re-scored by the fp32 chain on the common route; and the
 * largest |logit_x3 - logit_chain| / (tau_q / 2) over those re-scored candidates -- every one is an audit sample of the bound the
 * selection rests on (below 1 is what makes it exact; the library's tests assert <= 0.5, like coper_band_audit).  Any output may be
 * NULL.  COPER_SCORE_F32 handles report their queries and zeros. */
COPER_API int coper_predict_stats(coper_handle* h, int32_t reset, int64_t* n_queries, int64_t* n_unresolved, int64_t* n_rescored,
                                  float* max_ratio, void* stream);

/* The known facts of the KG, resident on the handle.  Replaces the table the reference writes as e1rel_to_e2_full.json and looks up
 * once per sample to form `e2_multi` (data.py:464-469, 494-503): the filter of a query (e1, rel) is a row of ONE fixed table, so a
 * handle that holds the table needs three ids per query and no CSR from the caller.  All arrays are device int64, in the layout of
 * coper_sample_train_batch's records: one row per distinct (e1, rel), rows ascending by key = e1 * num_rel + rel, tail_indptr
 * [n_keys + 1] from 0 to nnz, tail_idx [nnz] GLOBAL ids strictly ascending within a row (a row may be empty).
 * The library COPIES them into buffers of its own (entered in the ledger of coper_live_device_bytes; tails as int32 while num_ent
 * fits): the caller's arrays may be freed once the stream has reached this call.  The same pass checks them on the device; the call
 * synchronises the stream once and returns COPER_EINVAL -- coper_last_error names the first kind found, in this order: keys not
 * ascending, a key twice, an e1 / rel / tail out of range, tails of a row not strictly ascending, tail_indptr[0] != 0, tail_indptr
 * decreasing, tail_indptr[n_keys] != nnz -- leaving the index that was in force in force.  A second call replaces the index;
 * n_keys == 0 removes it and frees everything it and its lookups allocated.  The index is no function of the parameters: it survives
 * coper_prepare, coper_train_step and coper_reserve, and may be set before coper_prepare.  Entity shards take the whole table as it
 * is (filters carry global ids).  COPER_ROLE_ENCODE handles answer no queries: COPER_EUNSUPPORTED; so are more than 2^31 - 1 rows,
 * num_ent * num_rel beyond 63 bits and a stream that is being captured. */
COPER_API int coper_set_known_facts(coper_handle* h, const int64_t* e1, const int64_t* rel, const int64_t* tail_indptr,
                                    const int64_t* tail_idx, int64_t n_keys, int64_t nnz, void* stream);

/* The CSR filter of a batch from the resident index: what `eval_dataset` reads back per sample as `e2_multi` (data.py:464-469,
 * 494-503, then the dense mask of data.py:182-186), built on the device in three launches.  (1) a lane per query finds its key's row
 * and writes the row's length -- 0 for a key the index does not hold and for an e1 / rel outside the model's range (the encoder
 * clamps and counts those: coper_check_ids); (2) the lengths are scanned into filt_indptr [B + 1] (device int64; any B); (3) a lane
 * per OUTPUT entry copies the rows into filt_idx (device int64, ascending within a row as stored): a row of thousands of tails is
 * shared by as many lanes, stores are contiguous.  *nnz (host) = filt_indptr[B], read back with one 8-byte copy and one
 * synchronisation of the stream -- the explicit-CSR entry points size their launches by it.
 *   filt_idx == NULL: steps 1 - 2 and the readback only (size a buffer, call again);  filt_idx given with cap < *nnz: COPER_EINVAL,
 *   nothing written to filt_idx;  no index set: COPER_ESTATE;  B == 0: COPER_OK, *nnz = 0;  a stream that is being captured:
 *   COPER_EUNSUPPORTED (the readback).  Needs no prepared handle. */
COPER_API int coper_known_filter(coper_handle* h, const int64_t* e1, const int64_t* rel, int64_t B, int64_t* filt_indptr, int64_t* filt_idx,
                                 int64_t cap, int64_t* nnz, void* stream);

/* coper_predict_topk and coper_encode_rank with the filter looked up in the resident index instead of passed in: what the reference's
 * evaluation gets from `e2_multi` of its records (data.py:464-469, 494-503; metrics.py:44-46).  coper_known_filter runs into
 * workspaces of the handle (grown on demand where the total is known), then the body of the explicit-CSR call runs unchanged: same
 * results as that call given the same CSR, bit for bit; ranking keeps the target's own entry exempt from the filter.  e1 is required
 * (it forms the key) and e1_rows may accompany it for the encoder.  Every other argument, limit and error code is the explicit
 * call's; no index set: COPER_ESTATE; neither call can be captured into a hipGraph (COPER_EUNSUPPORTED: the filter's size is read
 * back). */
COPER_API int coper_predict_topk_known(coper_handle* h, const int64_t* e1, const int64_t* rel, const float* e1_rows, int64_t B, int32_t k,
                                       float* topk_val, int64_t* topk_idx, void* stream);
COPER_API int coper_encode_rank_known(coper_handle* h, const int64_t* e1, const int64_t* rel, const float* e1_rows, const int64_t* e2, int64_t B,
                                      float* h_out, int32_t* ranks, int32_t* n_equal, void* stream);

/* COPER_SCORE_BF16X3: the run-time audit of the exact band.  An AUDITED count launch (coper_config.band_audit_period: by default
 * the first after coper_prepare and every 8th, a sample of its workgroups, 128 pairs per round) re-scores pairs its band walk
 * decides (the competitors closest to each target) with the mode's own arithmetic as well and keeps the largest
 *        |logit_x3 - logit_chain| / (tau_q / 2)      (tau_q / 2: the error the band allows one logit; see rank_band_kappa)
 * seen since the last reset, and the number of pairs audited (modulo 2^32).  A ratio below 1 on every audited pair is what
 * makes the mode's ranks the fp32 chain's; the library's tests assert <= 0.5, coper_amd.metrics.ranking_and_hits logs a
 * warning above it.  Synchronises the stream.  COPER_SCORE_F32 handles report 0 / 0.  The reference has no counterpart: its
 * ranker works on materialised fp32 logits (metrics.py:40-50). */
COPER_API int coper_band_audit(coper_handle* h, int32_t reset, float* max_ratio, int64_t* n_pairs, void* stream);
/* The same two words without a synchronisation: dst2[0] = the ratio's float bits, dst2[1] = the pair count, posted to `dst2`
 * (device memory or PINNED, device-mapped host memory, like coper_copy_out_i32) behind the work already on the stream; a
 * host that waits for its ranks anyway reads them with the same wait.  COPER_ESTATE on a COPER_SCORE_F32 handle. */
COPER_API int coper_band_audit_post(coper_handle* h, int32_t reset, uint32_t* dst2, void* stream);
/* coper_copy_out_i32 and coper_band_audit_post in ONE launch: the n int32 ranks of a pass to dst[0, n) and the audit's two words to
 * dst[n], dst[n + 1] (zeros on a handle without a band), the audit reset for the next pass when reset != 0.  dst: n + 2 int32,
 * device or pinned host memory.  What `ranking_and_hits` fetches per `session.run` (metrics.py:40-43) plus the audit, behind the
 * pass's last kernel. */
COPER_API int coper_post_ranks_audit(coper_handle* h, const int32_t* ranks, int64_t n, int32_t* dst, int32_t reset, void* stream);
/* What a host DOES with the audit's two words (from coper_band_audit or coper_band_audit_post); host logic, no device work, no
 * synchronisation.  The contract of the path is integer ranks (metrics.py:44-50), so a measured error near the band's allowance
 * must not only be logged:
 *   ratio <= 0.5 (or no pair audited)  *action = COPER_BAND_KEEP;
 *   0.5 < ratio < 1                    the handle's kappa is doubled for every later pass         *action = COPER_BAND_WIDENED;
 *   ratio >= 1                         kappa is multiplied by the power of two that puts the error seen at or below a quarter of
 *                                      the new allowance, and the pass the words belong to must be ranked AGAIN by the caller
 *                                      (same call, same arguments: its close comparisons now go to the fp32 chain)
 *                                                                                                   *action = COPER_BAND_RERANK.
 * After a change the next count launch carries the audit whatever band_audit_period says, so a re-ranked pass is checked against
 * its new band at once.  The multiplier survives coper_prepare (it is a fact about the arithmetic, not about the weights);
 * *kappa_now = the relative half-width now in force.  coper_amd.metrics.ranking_and_hits applies this after every pass.
 * Sampling: with the default band_audit_period the first count launch after coper_prepare and every 8th from there are audited,
 * on the first round of at most ~512 workgroups and 128 pairs per round -- a sample; band_audit_period = 1 audits every launch.
 * No counterpart in the reference (it ranks materialised fp32 logits). */
#define COPER_BAND_KEEP 0
#define COPER_BAND_WIDENED 1
#define COPER_BAND_RERANK 2
COPER_API int coper_band_policy(coper_handle* h, float max_ratio, int64_t n_pairs, int32_t* action, float* kappa_now);

/* Timing hook used by bench.py: average device time (ms) of the dominant kernel
 * (score_count) over the launches since the last reset, measured with hipEvents recorded on
 * the launch stream.  enable != 0 turns per-launch event recording on. */
/* Step 1 of the entity-sharded exchange (coper_amd/sharding.py): every rank needs ent_emb[e1], ent_emb[e2] and pred_bias[e2] of the chunk
 * (models.py:176, :437); each row lives on one shard.  coper_pack_owned_rows writes what THIS shard owns for the all-gather --
 * buf[cap + 1][d + 1] float: row 0 = the header { hdr0, hdr1, 0... } (the shard's largest |ent_emb| and the table-wide maximum in
 * force: how the ranks keep ONE power of two for their entity planes), row 1 + i = { ent_emb[local_rows[i]], pred_bias[local_rows[i]] }
 * from the registered parameter tensors (no prepared state needed; a row number outside [0, n_local) gives a zero row and is counted
 * by coper_check_ids once the handle has a workspace), zeros up to cap -- and coper_unpack_rows hands the gathered rows
 * out: rows1[b] = gathered[take1[b]][0, d), rows2[b] = gathered[take2[b]][0, d), bias2[b] = gathered[take2[b]][d].  One launch each. */
COPER_API int coper_pack_owned_rows(coper_handle* h, const int64_t* local_rows, int64_t n, int64_t cap, float hdr0, float hdr1, float* buf,
                                    void* stream);
COPER_API int coper_unpack_rows(coper_handle* h, const float* gathered, const int64_t* take1, const int64_t* take2, int64_t B, float* rows1,
                                float* rows2, float* bias2, void* stream);

/* Step 3 of the entity-sharded exchange (coper_amd/sharding.py; north_star's one collective of counts + top-k): the record a shard
 * contributes, packed by ONE launch -- rec[B + 1][1 + 2 k] int64: row b = { n_greater << 32 | n_equal, the k top scores' float bits
 * (sign-extended int32), the k global ids } from coper_rank_counts' outputs; row B = the shard's band-audit words
 * { ratio bits << 32 | min(pairs, 2^31 - 1) } read on the device (and reset when reset_audit != 0: no host round trip; zeros on a
 * handle without a band) -- and, after the all-gather, the merge of all_rec[world][B + 1][1 + 2 k] by one more: ranks = 1 + the
 * summed n_greater (metrics.py:50), n_equal summed (may be NULL), the candidates side by side cand_val / cand_idx [B][world k]
 * (shard-major; the global top-k is their (score desc, id asc) selection).  Integer sums: bit-equal to the single-GPU ranks. */
COPER_API int coper_pack_shard_record(coper_handle* h, const int32_t* n_greater, const int32_t* n_equal, const float* topk_val,
                                      const int64_t* topk_idx, int64_t B, int32_t k, int32_t reset_audit, int64_t* rec, void* stream);
COPER_API int coper_merge_shard_records(coper_handle* h, const int64_t* all_rec, int32_t world, int64_t B, int32_t k, int32_t* ranks,
                                        int32_t* n_equal, float* cand_val, int64_t* cand_idx, void* stream);

/* Host only: n int64 ids narrowed to int32 into dst (the pinned staging buffer coper_widen_ids / coper_stage_ids_next read), checked on
 * the way: *status bit 0 = a value does not fit int32 (the caller then passes int64 arrays the ordinary way), bit 1 (with a CSR
 * indptr of n_rows rows over this array, indptr[0] = 0, indptr[n_rows] = n) = a row is not ascending (the filter contract of
 * coper_rank / coper_encode_rank: the caller sorts such rows first).  One pass instead of three over the bulk of a batch's host
 * marshalling (metrics.py:40-45 feeds placeholders; here the feed is the staging buffer). */
COPER_API int coper_pack_ids_i32(const int64_t* src, int64_t n, int32_t* dst, const int64_t* indptr, int64_t n_rows, int32_t* status);

/* Host only: the metrics of a pass's ranks as the reference computes them (metrics.py:53-57, 65-76): mean rank and mean reciprocal
 * rank as float64 means (the same summation order as numpy's np.mean, so the values are the ones the reference's expressions
 * give), hits[k] = the fraction of ranks <= levels[k].  ranks start at 1 (metrics.py:50); EINVAL otherwise and for n == 0. */
COPER_API int coper_hits_means(const int32_t* ranks, int64_t n, const int32_t* levels, int32_t n_levels, double* mean_rank, double* mrr,
                               double* hits);

/* One training batch of the reference's samplers (CoPER_ConvE/qa_cpg/data.py:228-311), built on the device by ONE launch (round 6).
 * Replaces what `train_dataset(...)`'s map function does per record on 32 tf.data threads (data.py:93-94, 138-156).  All pointers are
 * device memory on `device`:
 *   rec int64 [B]: the (e1, rel) record of each row of the batch (the host keeps the record stream, its shuffle buffer and the batching:
 *     data.py:136-160 on ids only); pos_tail int64 [B]: the row's positive (one positive per row: data.py:278-311; NULL when proportional);
 *   rec_e1, rec_rel int64 [n_rec]; tail_indptr int64 [n_rec + 1], tail_idx int64: the known train tails of every record (CSR);
 *   max_tails: the longest tail list among the batch's records (sizes the workgroups' hash set of known tails);
 *   proportional != 0: data.py:228-277 with prop_negatives -- the first `lead` of the record's tails in a fresh random order, then sampled
 *     entities; lead = the number of tails when that is <= int(L / (1 + prop_negatives)), L - min(num_ent, L - that) otherwise;
 * out: e1, rel, e2 int64 [B]; lookup int32 [B, L] (obj_lookup_values); labels float [B, L] (e2_multi: 1 where the looked-up entity is a
 *   known tail of the record -- a sampled "negative" that is one is supervised as positive, as the reference comments).
 * The sampled entities of a row are the head of a fresh uniform permutation of all entities (an ordered uniform sample without
 * replacement), a function of (seed, batch, row) alone.  L <= 2048, num_ent < 2^31 (the lookup's dtype); EUNSUPPORTED otherwise.
 * Asynchronous on `stream`; no handle: the sampler knows nothing of the model. */
COPER_API int coper_sample_train_batch(int32_t device, const int64_t* rec, const int64_t* pos_tail, const int64_t* rec_e1,
                                       const int64_t* rec_rel, const int64_t* tail_indptr, const int64_t* tail_idx, int64_t B, int64_t L,
                                       int64_t num_ent, int32_t proportional, double prop_negatives, int64_t max_tails, uint64_t seed,
                                       uint64_t batch, int64_t* e1, int64_t* rel, int64_t* e2, int32_t* lookup, float* labels, void* stream);

/* Ids are validated on the device and clamped, never trusted: returns in *n_bad the number of
 * out-of-range relation ids seen by coper_encode since the last call (synchronises the stream). */
COPER_API int coper_check_ids(coper_handle* h, int64_t* n_bad, void* stream);

/* The rank written for EVERY query of a coper_encode_rank pass that ran on a grouping prepared ahead (coper_group_next) whose id
 * arrays had been rewritten since: see "THE GUARD" there.  Whatever the count and band launches add to it stays negative. */
#define COPER_RANK_STALE (-(1 << 30))
/* Passes since the last call whose prepared grouping was found stale (synchronises the stream; the counter restarts at 0). */
COPER_API int coper_stale_passes(coper_handle* h, int64_t* n_passes, void* stream);

/* Device memory (bytes) currently held by all handles of this process: every allocation of the library is entered in a
 * ledger.  Returns to its previous value when a handle is destroyed (tests/test_gpu_train.py checks exactly that).  The
 * reference has no counterpart: TensorFlow owns its allocations (`tf.Session` of run_cpg.py:111). */
COPER_API int64_t coper_live_device_bytes(void);

COPER_API int coper_profile_enable(coper_handle* h, int enable);
COPER_API int coper_profile_read(coper_handle* h, const char* kernel, double* total_ms, int64_t* launches);

/* ---------------------------------------------------------------------------------------------
 * Training step: replaces `session.run(model.train_op)` of run_cpg.py:211-219, i.e.
 * models.py:176-200 (train-mode forward, sampled scorer, label-smoothed sigmoid cross-entropy),
 * tf.clip_by_global_norm(5.0) (models.py:199) and utils/amsgrad.py:130-189.
 * Supported: static (plain ConvE), g_linear / g_MLP generated or g_lookup dense layer; static, generated or
 * looked-up conv filters; concat_rel.  Looked-up conv filters with a static dense layer: COPER_EUNSUPPORTED.
 * The parameters registered with coper_set_param are UPDATED IN PLACE (they are the variables), including
 * the BN moving statistics; the caches built by coper_prepare go stale, so the handle must be prepared
 * again before the next inference call (enforced).
 * Dropout uses a counter-based hash of (seed, step, stage, element) instead of TF's RNG stream.
 * ------------------------------------------------------------------------------------------- */
typedef struct coper_train_config {
  int32_t abi_version;            /* COPER_ABI_VERSION */
  float learning_rate;            /* model_descriptors['learning_rate'] (models.py:130) */
  float beta1, beta2, epsilon;    /* AMSGrad defaults 0.9, 0.999, 1e-8 (amsgrad.py:60-62) */
  float clip_norm;                /* 5.0 (models.py:199) */
  float label_smoothing_epsilon;  /* models.py:101,450 */
  float hidden_dropout;           /* after conv BN ReLU (models.py:390) */
  float output_dropout;           /* before FCBN (models.py:414) */
  float batch_norm_momentum;      /* moving-average DECAY (models.py:64,387,417) */
  int32_t batch_norm_train_stats; /* BN uses batch statistics while training (models.py:62,358) */
  uint32_t seed;                  /* dropout stream */
  float context_rel_dropout;      /* dropout inside the g_MLP generators (models.py:67-68,118) */
  int32_t one_vs_all_chunk;       /* entity columns per chunk of coper_train_step_csr / coper_train_forward_csr; 0: the library's
                                   * choice, the widest chunk whose [B, chunk] float workspace stays within 256 MiB.  A request is
                                   * rounded UP to the GEMM column grain of 128 (the row padding of an operand plane) and capped at
                                   * num_ent; negative: COPER_EINVAL.  Took the first reserved slot: layout and version unchanged */
  union {                         /* the six words behind one_vs_all_chunk, where reserved[6] always was: word 0 has a name now */
  int32_t deterministic;          /* 0: the step as it always was (the default; same launches, same results).  1: BIT-REPRODUCIBLE
                                   * training: given the same library build and GPU model, the same coper_config and coper_train_config,
                                   * the same variables, optimizer slots, beta powers and step counter, and the same batch arrays (same
                                   * values in the same order), coper_train_step, coper_train_step_csr, coper_train_forward and
                                   * coper_train_forward_csr return the same BITS in every output -- loss_out, pred_out, h_out, every
                                   * coper_train_grad leaf and its global_norm (a double), every variable after the step (BN moving
                                   * statistics included) and every AMSGrad slot -- from call to call, between handles and between
                                   * processes, on any stream, with COPER_TRAIN_ONE_STREAM set or not, whatever else runs on the GPU and
                                   * whatever addresses the allocations got.  Every sum of the step has one defined order: reducing
                                   * launches store per-workgroup partial sums that a fold launch adds in ascending workgroup index, and
                                   * embedding / relation rows have one writer that adds a row's samples in ascending sample index (then
                                   * ascending lookup position) after what the scorer's GEMM stored there.  The step runs as one chain
                                   * on `stream` (no side streams).  NOT promised: the default mode's bits; equality across permutations
                                   * of a batch, across one_vs_all_chunk widths, GPU models or builds.  Refused with COPER_EUNSUPPORTED
                                   * by the step, never served unordered: sampled labels with B * num_ent * 4 > 512 MiB (the scorer's
                                   * atomic backward); an ent_emb or pred_bias tensor that is not 16-byte aligned (routes chosen by
                                   * alignment sum in another order).  Any other value: COPER_EINVAL from coper_train_init.  Took the
                                   * second reserved slot, reserved[0]: layout, sizeof and COPER_ABI_VERSION unchanged, and a caller
                                   * built against the earlier header, which zeroed reserved[], asks for the default mode */
  int32_t reserved[6];            /* [0] is `deterministic`; [1 .. 5] are reserved and must be 0 */
  };
} coper_train_config;

/* Allocates gradients and the AMSGrad slots m, v, v_hat (zeros) for every trainable parameter; every
 * parameter must have been registered with coper_set_param. */
COPER_API int coper_train_init(coper_handle* h, const coper_train_config* cfg);
/* The mode in force: 1 (coper_train_config.deterministic) or 0; -COPER_ESTATE without a training state, -COPER_EINVAL for a null handle. */
COPER_API int coper_train_deterministic(const coper_handle* h);
/* One optimisation step on a training batch in the reference batch contract (models.py:139-152):
 * e1, rel int64 [B]; lookup int32 [B,L] (obj_lookup_values); labels float [B,L] (e2_multi for the looked-up
 * entities).  lookup == NULL with L == num_ent is 1-vs-all training (use_negative_sampling = False, run_cpg.py:116:
 * labels are the dense e2_multi [B, num_ent], models.py:159-162).  loss_out: device float[1], the batch loss
 * (models.py:448-453).
 * The registered tensors ARE the variables and the step keeps facts about them from one step to the next (round 6: the largest
 * magnitude of the dense weights, noted by the optimizer's pass as it writes them, is what the next step's operand packing scales
 * by).  A caller that changes parameter CONTENTS between steps by other means than this call registers the tensor again
 * (coper_set_param on the same pointer is enough; coper_amd.ConvE.load_parameters does) -- as coper_prepare asks for inference.
 * coper_set_param with another pointer moves the variable there: later steps read and update the tensor registered last.
 * Ordering: to the caller the step is one sequence of launches on `stream`.  Inside, two stretches that do not depend on the chain
 * beside them (the scorer's backward; the projection gradient's product) run on streams of the training state's own, forked from
 * `stream` and joined to it by events before the call returns -- nothing of the step is left outside `stream`'s order. */
COPER_API int coper_train_step(coper_handle* h, const int64_t* e1, const int64_t* rel, const int32_t* lookup,
                               const float* labels, int64_t B, int64_t L, float* loss_out, void* stream);
/* The train-mode graph WITHOUT the update: what `session.run(model.loss)` or `session.run(model.predictions_lookup)` under
 * `{model.is_train: True}` evaluate when `train_op` is not among the fetches (models.py:183-192: the loss and the likelihoods are
 * plain tensors of the graph; the UPDATE_OPS and the optimizer hang off train_op only, models.py:194-200).  Same batch contract as
 * coper_train_step; dropout with the masks the NEXT coper_train_step will draw (the step counter is not advanced), batch
 * statistics when batch_norm_train_stats -- and nothing written: no variable, no BN moving statistic, no optimizer slot.
 * loss_out: device float[1] or NULL; pred_out: device float [B, L] logits (predictions_lookup; [B, num_ent] with lookup == NULL)
 * or NULL; h_out: device float [B, d] (predicted_e2_emb in training mode) or NULL.  Inference caches stay valid. */
COPER_API int coper_train_forward(coper_handle* h, const int64_t* e1, const int64_t* rel, const int32_t* lookup,
                                  const float* labels, int64_t B, int64_t L, float* loss_out, float* pred_out, float* h_out,
                                  void* stream);
/* 1-vs-all training from SPARSE labels, at any number of entities: coper_train_step(lookup == NULL) / coper_train_forward(lookup ==
 * NULL) with the dense e2_multi [B, num_ent] replaced by the id lists it is built from (the reference stores them that way and
 * densifies them for TensorFlow only, data.py:318-322).  Everything not said here is the contract of those two calls: dropout
 * counters, BN statistics, the side streams, stale inference caches, pred_out as [B, num_ent] logits, what is and is not written.
 *   lab_indptr device int64 [n_rows + 1], lab_idx device int64: a CSR table of global entity ids, STRICTLY ASCENDING within a row
 *     (the tail_indptr / tail_idx of coper_sample_train_batch's records is one);  lab_row device int64 [B]: the label row of sample
 *     b is table row lab_row[b] -- the same row may occur several times in a batch, in any order.  lab_row == NULL: row b, and
 *     n_rows must equal B (a plain per-batch CSR).  A row may be empty.
 *   Labels are binary: 1.0 at the listed entities, 0.0 elsewhere; label_smoothing_epsilon and the + 1 / num_ent of models.py:450
 *     apply on top, by the expression the dense-label call uses.
 *   An entry of lab_idx outside [0, num_ent) and a lab_row outside [0, n_rows) are never dereferenced or written through: such an
 *     entry is treated as ABSENT (a bad lab_row is an empty row), no error is raised.  lab_indptr itself is trusted.  A row that is
 *     not ascending yields unspecified 0 / 1 labels for that row, nothing worse.
 * Neither [B, num_ent] matrix exists: the scorer is walked in chunks of entity columns (coper_train_config.one_vs_all_chunk) --
 * logits, loss, d(pred_bias), d(ent_emb) rows and the chunk's share of dh per chunk, shares added in ascending chunk order (no float
 * atomics: the step is as repeatable as the dense-label one).  So neither the 512 MiB cap of the dense-label call nor B * L <= 2^31 - 1
 * applies.  With one chunk (num_ent <= the chunk width) every launch but the loss kernel is the dense-label call's, and so is every
 * gradient bit. */
COPER_API int coper_train_step_csr(coper_handle* h, const int64_t* e1, const int64_t* rel, const int64_t* lab_indptr,
                                   const int64_t* lab_idx, const int64_t* lab_row, int64_t n_rows, int64_t B, float* loss_out,
                                   void* stream);
COPER_API int coper_train_forward_csr(coper_handle* h, const int64_t* e1, const int64_t* rel, const int64_t* lab_indptr,
                                      const int64_t* lab_idx, const int64_t* lab_row, int64_t n_rows, int64_t B, float* loss_out,
                                      float* pred_out, float* h_out, void* stream);
/* The step in three calls: backward | export | apply.  coper_train_step stays what it is; these split it where a caller wants an
 * update from several batches (accumulation) or from several replicas (data-parallel training: all-reduce between export and apply).
 * The one object that crosses the boundary is the FLAT GRADIENT VECTOR: one device float buffer that holds every trainable leaf's
 * gradient, which the caller may add to, all-reduce or keep.
 *
 * coper_train_backward / coper_train_backward_csr: the arguments, routes, refusals and side streams of coper_train_step /
 *   coper_train_step_csr, and everything they do up to the optimizer: the loss, the BN moving-statistics update, the dropout counter
 *   advanced by one -- and the gradients, which stay in the handle's gradient buffers ("pending").  No variable, optimizer slot or
 *   beta power is touched, and the handle stays prepared: evaluation between backward and apply needs no coper_prepare and changes
 *   nothing that apply or export read (the batch's relation counts are kept apart, as for coper_train_grad).  The one thing such an
 *   evaluation sees stale is BN: its folded scale and shift come from the moving statistics as the last coper_prepare found them,
 *   one momentum step per backward behind the tensors.  Call coper_prepare where that matters.
 * coper_train_grads_layout: where leaf `leaf_name` lies in the flat vector (*offset, *n floats) and the vector's length *total.  The
 *   trainable leaves in coper_param_spec order, each starting at a multiple of 64 floats.  leaf_name == NULL: *total alone.  Any
 *   output may be NULL.
 * coper_train_grads_export: flat = g, or flat += g when accumulate != 0, over all leaves in one launch on `stream`.  Rows of the
 *   looked-up dense table whose relation the backward's batch did not hold are exported as zeros (with accumulate they add
 *   nothing); the pad behind every leaf is written as 0.  flat: device, 16-byte aligned, cap >= total floats; else COPER_EINVAL.
 *   No atomics: one thread owns an element, in either form.
 * coper_train_apply: the optimizer phase alone -- squared global norm, clip, AMSGrad; the beta powers advance, inference caches go
 *   stale.  flat == NULL (n ignored): the pending gradients of the last coper_train_backward.  Otherwise the gradient is read from
 *   `flat` in place (16-byte aligned, n == total; else COPER_EINVAL), every row present, and no backward is needed.  `scale`
 *   multiplies the gradient before the clip: the norm, and what coper_train_grad reports as global_norm afterwards, is that of
 *   scale * g; the element factor scale * clip / max(norm, clip) is formed once, in double (scale == 1: the bits of the fused step).
 *   The mean over M accumulated micro-batches on W replicas is scale = 1 / (M W) on the all-reduced sum.
 * State: apply consumes the pending gradients.  coper_train_apply(flat == NULL) without a coper_train_backward since the last
 *   coper_train_apply, coper_train_step*, coper_train_forward* or coper_train_init is COPER_ESTATE: those calls zero the gradient
 *   buffers (a half-zeroed gradient is never applied).  coper_train_powers' `step` counts backward passes (the dropout counter), the
 *   beta powers count updates.
 * Deterministic mode: every launch these calls add has one defined order, and coper_train_backward + coper_train_apply(NULL, 1), or
 *   + coper_train_grads_export + coper_train_apply(flat, 1), leave the bits of coper_train_step in every output.  In the default mode
 *   the split step's norm is summed in another order than the fused step's (whose GEMM epilogues add the dense weights' squares). */
COPER_API int coper_train_backward(coper_handle* h, const int64_t* e1, const int64_t* rel, const int32_t* lookup,
                                   const float* labels, int64_t B, int64_t L, float* loss_out, void* stream);
COPER_API int coper_train_backward_csr(coper_handle* h, const int64_t* e1, const int64_t* rel, const int64_t* lab_indptr,
                                       const int64_t* lab_idx, const int64_t* lab_row, int64_t n_rows, int64_t B, float* loss_out,
                                       void* stream);
COPER_API int coper_train_grads_layout(coper_handle* h, const char* leaf_name, int64_t* offset, int64_t* n, int64_t* total);
COPER_API int coper_train_grads_export(coper_handle* h, float* flat, int64_t cap, int32_t accumulate, void* stream);
COPER_API int coper_train_apply(coper_handle* h, const float* flat, int64_t n, double scale, void* stream);
/* Diagnostics: 1 when the next step will scale the dense weights' operand packing by the maximum the last optimizer pass recorded as
 * it wrote them (no pass over the weights), 0 when it will scan them (before the first update; after coper_set_param of a TRAINABLE
 * leaf -- registering a BN moving statistic again leaves it at 1: it says nothing about the weights; looked-up dense tables, which
 * are not packed, report 0); -COPER_ESTATE without a training state, -COPER_EINVAL for a null handle. */
COPER_API int coper_train_wmax_carried(const coper_handle* h);
/* Diagnostics: copies the (unclipped) gradient of the last step for a trainable leaf into `out` (device float
 * buffer of `cap` elements; may be NULL), returns its length in *n, and in *global_norm (optional, host) the
 * global gradient norm of the last step (synchronises).  The looked-up dense table's rows of relations the last batch did not hold are
 * not written by a step -- optimizer and norm skip them by the batch's relation counts -- and are handed out as the zeros they stand for
 * by those same counts, which the step keeps a copy of: evaluation passes, coper_encode or coper_reserve in between do not change
 * what this call returns. */
COPER_API int coper_train_grad(coper_handle* h, const char* leaf_name, float* out, int64_t cap, int64_t* n,
                               double* global_norm, void* stream);

/* Optimizer state, for checkpoints (the reference's tf.train.Saver stores the slots `<var>/AMSGrad`, `/AMSGrad_1`,
 * `/AMSGrad_2` = m, v, v_hat of utils/amsgrad.py:117-119 and the non-slot variables beta1_power / beta2_power,
 * amsgrad.py:108-113).  `which`: 0 m, 1 v, 2 v_hat; `buf`: device float buffer of `cap` elements (may be NULL to
 * query *n); set == 0 copies slot -> buf, set != 0 copies buf -> slot, stream-ordered.  Powers: get with non-NULL
 * outputs, set with non-NULL inputs; `step` is the dropout counter of the next step. */
COPER_API int coper_train_slot(coper_handle* h, const char* leaf_name, int32_t which, float* buf, int64_t cap, int32_t set,
                               int64_t* n, void* stream);
COPER_API int coper_train_powers(coper_handle* h, const double* set_beta1_power, const double* set_beta2_power,
                                 const int64_t* set_step, double* beta1_power, double* beta2_power, int64_t* step);

/* Deferred rows: an opt-in mode of the SAMPLED step (coper_train_step / coper_train_forward with a lookup) in which every launch touches
 * O(B L d) bytes of ent_emb, pred_bias, their gradients and their slots, and none that scale with num_ent.  The optimizer stays the
 * reference's dense AMSGrad (utils/amsgrad.py:161-189 decays m and v of every row every step): for a row with zero gradient that update
 * is a closed form -- a row (p, m, v, v_hat) current at update t0 and without gradient at updates t0+1 .. t0+k becomes
 *     v_hat' = max(v_hat, beta2 v)      m' = beta1^k m      v' = beta2^k v      p' = p - C m / (sqrt(v_hat') + epsilon)
 *     C = sum_{j=1..k} lr(t0+j) beta1^j,   lr(t) = learning_rate sqrt(1 - beta2^t) / (1 - beta1^t)
 * (C and the powers in double, from the state's beta powers; terms below 2^-53 of the sum are dropped, by a bound that follows beta1)
 * -- so a row is brought current only when something reads it: the rows a batch names, in front of its forward pass; every row before
 * inference, export or a checkpoint.  This is a deferred, EXACT row update, not the "lazy" optimizer of other libraries (which skips
 * the decay).  Against the dense step the results differ by float32 rounding only: p is rounded once per gap instead of once per
 * update, m and v take one rounded power, and the scorer's backward always takes the float-atomic route (the one large tables take).
 * With the mode off every launch and every bit is what it was.
 *
 * coper_train_defer_rows(h, enable, stream): after coper_train_init (COPER_ESTATE without a training state); enable is 0 or 1
 *   (COPER_EINVAL otherwise); COPER_EUNSUPPORTED on a deterministic = 1 state (the unique-row list and the atomic scorer backward are
 *   unordered).  Enabling allocates the row state -- an int32 "current as of update" word per row, a claim bitmap of num_ent bits, two id
 *   lists of B (L + 1) int32 that grow with the batch -- and zeroes d(ent_emb) / d(pred_bias) whole, once.  Disabling first brings every
 *   row current on `stream`; the next step is the dense one.
 * coper_train_rows_deferred(h): 1 or 0; -COPER_ESTATE without a training state, -COPER_EINVAL for a null handle.
 * coper_train_sync_rows(h, stream): one pass over num_ent that brings every row of ent_emb, pred_bias and their three slots current.
 *   Idempotent (a row that is current is not written: a second call changes no bit); a no-op with the mode off.
 * coper_train_row_stats(h, &rows_last_step, &rows_behind, &max_gap, stream): the unique (clamped) rows the last coper_train_step /
 *   coper_train_forward named; the rows that are not current and the largest number of updates one is behind, from one scan of the step
 *   words.  Any output may be NULL; zeros with the mode off.  Synchronises `stream`: for tests and diagnostics.
 *
 * With the mode on
 *   - these calls bring every row current themselves before they read or replace the tables, so explicit syncing is only ever an
 *     optimisation: coper_prepare; coper_train_slot (get and set) of ent_emb / pred_bias; coper_set_param of those two leaves and
 *     coper_train_powers when it sets a power (neither has a stream: the pass runs on the null stream between two device
 *     synchronisations, so not under stream capture; coper_set_param syncs through the pointers registered BEFORE the call, which must
 *     still be live).  coper_train_grad needs nothing: the dense gradient buffers stay and hold the whole gradient of the last step
 *     (the rows of the step before are re-zeroed at the start of the next call instead of the whole buffers).
 *   - these are refused with COPER_EUNSUPPORTED, coper_last_error says why, the handle stays usable: 1-vs-all steps, dense or CSR (every
 *     row has a gradient); coper_train_backward*, coper_train_grads_export, coper_train_apply (the flat vector is dense by contract:
 *     the mode's split step is coper_train_rows_backward / _export / _import / _apply, "Deferred rows: the step in calls" below).
 *   - the registered ent_emb / pred_bias TENSORS are current only after a sync (or one of the calls above): a raw read of them in
 *     between sees rows as of their last use.  Rows named by a step are current when it returns.
 *   - coper_train_forward brings the rows of its batch current too (it reads them) and advances nothing.
 *   - with the profile enabled (coper_profile_enable) the training step files counts, no times, under these names for
 *     coper_profile_read: "train.zero.<leaf>" per whole-buffer zeroing of a leaf's gradient (ent_emb, pred_bias, rel_emb and the static
 *     conv leaves), "train.sumsq.leaves" / "train.amsgrad.leaves" the tensors k_tr_sumsq / k_tr_amsgrad ran over, and
 *     "train.rows.rezero|claim|catch_up|sumsq|update|sync" per launch of a row kernel.
 *
 * On an entity-sharded state ("Entity-sharded training" below) the switch is accepted BETWEEN STEPS: in any phase of the
 *   four-call step other than "forward expected" it returns COPER_ESTATE, the text names the call expected next.  The mode is ENABLED
 *   before the state's first step (after coper_train_init_sharded; checkpointed slots and powers may be loaded before or after): on a
 *   sharded state that has made a step, enabling returns COPER_EUNSUPPORTED as it always did there (not built; a new
 *   coper_train_init_sharded on the handle starts a state that can take it).  Disabling is served at any step boundary.  No ordered-rows switch
 *   is needed (the sharded sampled call is always ordered).  The row state is per LOCAL row: a word and a claim bit per owned row, the
 *   two lists of B (L + 1) entries; coper_train_sync_rows, coper_train_row_stats and the calls above that sync by themselves work over
 *   the handle's own rows.  What the four calls do in the mode is said there; their two kernels of their own file
 *   "train.rows.gather_current" and "train.rows.list_owned" per launch with the profile enabled.
 * coper_train_rows_updates(h): the updates made since the mode was enabled (what the step words count in; ranks of one sharded table
 *   must agree on it); 0 with the mode off; -COPER_ESTATE without a training state, -COPER_EINVAL for a null handle. */
COPER_API int coper_train_defer_rows(coper_handle* h, int32_t enable, void* stream);
COPER_API int coper_train_rows_deferred(const coper_handle* h);
COPER_API int64_t coper_train_rows_updates(const coper_handle* h);
COPER_API int coper_train_sync_rows(coper_handle* h, void* stream);
COPER_API int coper_train_row_stats(coper_handle* h, int64_t* rows_last_step, int64_t* rows_behind, int64_t* max_gap, void* stream);

/* Ordered rows: an opt-in switch on a deterministic = 1 training state that builds the sparse table gradient of a SAMPLED batch
 *     dE[lookup[b,l]] += ds[b,l] h[b]        dbias[lookup[b,l]] += ds[b,l]
 * with one writer per row and one order of addends, at any num_ent: the B L lookup ids (clamped as everywhere: outside [0, num_ent) is
 * row 0) are sorted by a stable radix sort into ascending (id, b, l); the sorted run of an id is its segment; one wave per segment forms
 *     acc = fmaf(ds[b,l], h[b][k], acc)   from acc = 0.f, over the segment's entries in ascending (b, l)
 * per element k -- and acc = fmaf(ds[b,l], 1.f, acc) for dbias -- and stores it with `=` onto the zeroed row.  ent_emb_size % 4 == 0 takes
 * 16-byte accesses, anything else the scalar route with the same results.  A segment is never split, so its sum is a function of the
 * batch alone: not of a grid, a capacity or an occupancy.  The segment heads are the batch's unique rows (the e1 ids included) in
 * ascending id.  The sort tile (COPER_ORDER_SORT_TILE entries) and the stretch of the ordered norm (COPER_ORDER_SUMSQ_ROWS list
 * positions per partial sum) are constants of the kernels; neither reaches a result.
 *
 * coper_train_order_rows(h, enable, stream): after coper_train_init (COPER_ESTATE without a training state; coper_train_init clears the
 *   switch); enable is 0 or 1 (COPER_EINVAL otherwise); COPER_EUNSUPPORTED on a deterministic = 0 state (the rest of that step is
 *   unordered, so nothing could be promised); disabling while deferred rows is on is COPER_ESTATE (disable deferred rows first).
 *   Switching clears what a split step left pending, as coper_train_defer_rows does.  Nothing is launched; the sort's workspace
 *   (four int32 arrays of B (L + 1), the segment offsets and the tile histograms) grows with the batch.
 * coper_train_rows_ordered(h): 1 or 0; -COPER_ESTATE without a training state, -COPER_EINVAL for a null handle.
 *
 * With the switch on (and for this switch only, the three sentences of the sections around it read as follows)
 *   - SAMPLED steps, backwards and forwards (coper_train_step, coper_train_backward, coper_train_forward with a lookup) are served at
 *     any B * num_ent: the 512 MiB refusal of the deterministic mode does not apply.  The scorer backward of a sampled batch ALWAYS takes
 *     the route above, whatever num_ent is -- one arithmetic for every table size.  Its bits are NOT those of the dense-S route that
 *     deterministic = 1 takes without the switch (a GEMM on split operands): the promise is reproducibility, not equality with the
 *     other route.  1-vs-all batches (dense or CSR labels) keep the launches and the bits of deterministic = 1.  The 16-byte alignment
 *     refusal stays.
 *   - coper_train_defer_rows(h, 1, ...) is accepted on the deterministic state: the row list of a call is the segment heads -- ascending
 *     id, not an unordered append -- the scorer backward is the route above instead of float atomics, and the norm of the listed rows is
 *     summed in partial sums of COPER_ORDER_SUMSQ_ROWS list positions that a fold adds in a fixed order, beside the small leaves'
 *     share.  Every call of the mode then runs under the determinism contract of the deterministic mode: step, forward, sync, slot
 *     reads, coper_train_rows_backward | _export | _import | _apply.  From the same build, configuration, variables, slots, powers, step
 *     counter, row words and batch arrays every output has the same bits: call after call, between handles, and between handles with
 *     different histories (a row list or workspace that grew earlier from a larger batch).
 *   - coper_train_rows_export writes its block in ascending row id; after imports the pending list is sorted ascending again before
 *     anything order-sensitive reads it (the norm of coper_train_rows_apply, an export).  The replicas of a data-parallel run import the
 *     same blocks in the same order and apply the same small vector: they end byte-identical in every variable, slot, power and row word,
 *     not merely equal to rounding.
 *   - not promised: equality across permutations of a batch, across builds, or across GPU models.
 *   - cost, as measured on an MI355X at B = 512, L = 1000 (profiles/train_ordered.json): the sort is 29 us per digit pass,
 *     heads 17 us, the reduce 44 us at FB15k-237 (135 us at 1M entities), the ordered norm 22 - 72 us; a sampled step is 1.00 (FB15k-237)
 *     / 0.89 (WN18RR) of deterministic = 1 without the switch and 1.22 / 1.25 of the default mode; with deferred rows 0.73 - 0.83 of the
 *     default mode's deferred step (no float atomics).  A segment is one wave's serial chain: a hub id in every position costs B L fmas.
 *   - with the profile enabled the launches file counts under "train.order.sort" (three per digit pass), "train.order.heads" (two),
 *     "train.order.reduce" and, with deferred rows, "train.order.sumsq"; a sampled step files none under "train.rows.claim". */
#define COPER_ORDER_SORT_TILE 2048
#define COPER_ORDER_SUMSQ_ROWS 64
COPER_API int coper_train_order_rows(coper_handle* h, int32_t enable, void* stream);
COPER_API int coper_train_rows_ordered(const coper_handle* h);

/* Deferred rows: the step in calls.  The split step of the mode: backward | export | import | apply, for gradient accumulation and
 * data-parallel replicas of a model whose tables are too large to exchange whole.  Two objects cross the boundary:
 *   the SMALL FLAT VECTOR: the rules of coper_train_grads_layout (coper_param_spec order, every leaf at a multiple of 64 floats, pads 0)
 *     over the trainable leaves EXCEPT ent_emb and pred_bias;
 *   the ROW BLOCK for those two: ids int32 [row_cap] and vals float [row_cap, rs], rs = (ent_emb_size + 1 + 3) & ~3 floats.  Columns
 *     [0, d) of vals[i] hold row ids[i] of d(ent_emb), column d holds d(pred_bias)[ids[i]], the pad columns are 0.  With vals 16-byte
 *     aligned every row is, and ent_emb_size % 4 == 0 then takes 16-byte accesses (anything else: the scalar route, same results).
 *     The ids of a block are distinct and lie in [0, num_ent).  An entry < 0 or >= num_ent is PADDING: never dereferenced, written
 *     through or listed.  A block that carries an id twice gets an unspecified sum of the two for that row, nothing worse.
 *
 * coper_train_rows_layout(h, leaf_name, &offset, &n, &total, &row_stride): where `leaf_name` lies in the small vector, the vector's
 *   length and rs.  leaf_name == NULL: *total and *row_stride alone; "ent_emb" / "pred_bias": COPER_EINVAL (they travel as blocks).
 *   Any output may be NULL.  A function of the model: the same with the mode on or off (after coper_train_init: COPER_ESTATE before).
 * coper_train_rows_backward: the arguments of coper_train_step, and the mode's sampled step up to the optimizer -- re-zero, claim,
 *   catch-up, forward, backward.  The loss, the BN moving statistics and the dropout counter move; no variable, slot or beta power is
 *   touched; the handle stays prepared (as coper_train_backward).  The gradients stay PENDING on the handle: the small leaves in their
 *   gradient buffers, the tables as the claimed row list plus the rows of the dense gradient buffers, as after a step.
 *   lookup == NULL (1-vs-all): COPER_EUNSUPPORTED.  Mode off: COPER_ESTATE.
 * coper_train_rows_export(h, small, small_cap, accumulate, ids, vals, row_cap, count, stream): small = g or small += g (accumulate != 0)
 *   over the small leaves in one launch (no atomics; 16-byte aligned, small_cap >= total); the pending list's rows gathered into the
 *   block: ids[i] the row, vals[i] a bit-for-bit copy of its gradient row and bias gradient, ids[count .. row_cap) = -1, *count (a
 *   DEVICE int32; may be NULL) the list's length.  row_cap below the host-known bound of the pending rows -- min(B (L + 1), num_ent)
 *   after a backward, min(num_ent, entries imported since `first`) after imports -- is COPER_EINVAL before anything is launched; the
 *   host is never synchronised.  ids / vals may be NULL together (the small vector alone), small may be NULL (the block alone).
 *   Nothing is consumed: the pending state stays.  Nothing pending for a part that is asked for: COPER_ESTATE.
 * coper_train_rows_import(h, ids, vals, n, first, stream): adds a block of n entries to the handle's pending TABLE gradient.
 *   first != 0 starts a new pending gradient: the rows of the current list are re-zeroed, their claim bits cleared, the list emptied
 *   (what a step does to the list of the call before).  Rows the list does not hold yet are claimed, appended and brought current
 *   (once: a current row is skipped).  vals are added to the rows of the dense gradient buffers with one writer per element per call and
 *   no float atomics: blocks add up in call order, the sum of an element has one defined order.  The list grows by the host-known bound
 *   and keeps its content (a host synchronisation of `stream` when it grows, as a step that grows it).  first == 0 with no table
 *   gradient pending: COPER_ESTATE.  n == 0 is allowed.
 * coper_train_rows_apply(h, small, n, scale, stream): the optimizer alone.  The squared norm from the small leaves and the listed
 *   rows; AMSGrad on the small leaves (read from `small` in place: 16-byte aligned, n == total, else COPER_EINVAL; small == NULL: the
 *   pending gradients of the last coper_train_rows_backward) and on the listed rows; the update counter of the rows, the beta powers
 *   and their log2 advance as in the mode's fused step.  The table part always comes from the handle's pending rows, left there by
 *   the backward or by imports.  `scale` as in coper_train_apply.  Nothing pending: COPER_ESTATE.  Consumes what is pending.
 *
 * State (as "The step in three calls"): coper_train_step*, coper_train_forward*, coper_train_init, coper_train_defer_rows that
 *   switches the mode, and coper_train_rows_apply clear what is pending; a refused call clears nothing.  coper_prepare between backward
 *   and apply is allowed and changes nothing the apply reads.  coper_train_grad after a backward or after imports returns the dense
 *   pending gradient as it stands; coper_train_row_stats' rows_last_step the length of the pending list (after imports: the union of
 *   the blocks' rows).  With the profile enabled the new launches file counts under "train.rows.export" and "train.rows.import".
 *   Deterministic states cannot enable the mode, so these calls are COPER_ESTATE there.  The replicas of a data-parallel run add the
 *   same blocks in the same order and so hold the same table gradient byte for byte; the mode's norm is summed by unordered atomics, so
 *   their variables agree to rounding, not to the bit. */
COPER_API int coper_train_rows_layout(coper_handle* h, const char* leaf_name, int64_t* offset, int64_t* n, int64_t* total,
                                      int64_t* row_stride);
COPER_API int coper_train_rows_backward(coper_handle* h, const int64_t* e1, const int64_t* rel, const int32_t* lookup,
                                        const float* labels, int64_t B, int64_t L, float* loss_out, void* stream);
COPER_API int coper_train_rows_export(coper_handle* h, float* small, int64_t small_cap, int32_t accumulate, int32_t* ids, float* vals,
                                      int64_t row_cap, int32_t* count, void* stream);
COPER_API int coper_train_rows_import(coper_handle* h, const int32_t* ids, const float* vals, int64_t n, int32_t first, void* stream);
COPER_API int coper_train_rows_apply(coper_handle* h, const float* small, int64_t n, double scale, void* stream);

/* Entity-sharded training: 1-vs-all from sparse labels, or sampled batches, with the entity table split over G handles (DESIGN 6.7,
 * 6.8).  Rank g holds rows
 * [shard_lo, shard_hi) of ent_emb / pred_bias (coper_config), their gradients and their AMSGrad slots, and nothing of the other rows.
 * The encoder runs replicated on the whole batch; the scorer (the chunk loop of coper_train_step_csr over the handle's own rows), the
 * table's optimizer pass and the table's memory divide by G.  The caller moves three small things per step between the ranks: the
 * [B, d] input rows, the [G, B, d] shares of dh with G doubles of loss, and G doubles of squared norm.
 *
 * coper_train_init_sharded(h, cfg): coper_train_init, but any [shard_lo, shard_hi) of a COPER_ROLE_BOTH handle is accepted ([0, num_ent):
 *   a world of one); gradients and slots of the two tables are allocated for the handle's rows only.  Needs cfg->deterministic == 1
 *   (COPER_EUNSUPPORTED otherwise): the replicas of the encoder stay equal with no exchange only because that mode makes h, every
 *   small-leaf gradient and the BN moving statistics a function of their inputs.  coper_train_init itself still refuses shard handles.
 * coper_train_sharded(h): 1 or 0; -COPER_ESTATE without a training state, -COPER_EINVAL for a null handle.
 * coper_train_shard_gather(h, e1, B, rows_out, stream): rows_out [B, d] = the table rows of the ids this handle holds, zero rows for
 *   the others -- one addend of e1_rows below (each element has one non-zero addend: the sum over ranks is exact).  Reads the
 *   registered table as it stands, prepared or not; no part of the state machine.
 * The step, four calls in this order -- forward | score_csr OR score_lookup | backward | apply; a step may use another label form
 * than the step before (any other order: COPER_ESTATE, the text names the call, or the two calls, expected next):
 * coper_train_shard_forward(h, e1, rel, e1_rows, B, h_out, stream): the train-mode encoder up to h on the whole batch.  The input
 *   images are the rows of e1_rows (device float [B, d]: the sum over ranks of coper_train_shard_gather / coper_gather_entities),
 *   never the table's.  e1 and rel (device int64 [B]) are copied: the later calls name no ids.  h_out: optional device float [B, d].
 *   Zeroes the gradients, moves the BN moving statistics as a step does.
 * coper_train_shard_score_csr(h, lab_indptr, lab_idx, lab_row, n_rows, B, dh_part, loss_part, stream): labels as coper_train_step_csr
 *   (global ids; entries outside the shard are absent for this rank).  Walks the own rows in chunks of one_vs_all_chunk columns (local
 *   column c is entity shard_lo + c; the label-smoothing term uses the global num_ent), stores this shard's d(pred_bias) and
 *   d(ent_emb) rows, and hands out dh_part (device float [B, d]: the chunk shares added in ascending chunk order) and loss_part
 *   (device double [1]: the unnormalised sum).
 * coper_train_shard_score_lookup(h, lookup, labels, B, L, dh_part, loss_part, stream): the sampled form, valid exactly where
 *   coper_train_shard_score_csr is.  lookup (device int32 [B, L], GLOBAL ids) and labels (device float [B, L]) are the arrays
 *   coper_train_step takes, the same on every rank; ids outside [0, num_ent) count as row 0 and so belong to the shard that holds it.
 *   B must be the forward call's, L >= 1, B (L + 1) and num_ent must fit 31 bits (COPER_EINVAL).  An entry (b, l) is OWNED when
 *   shard_lo <= id < shard_hi after the clamp.  For the owned entries, and only for them: s = h[b] . E[id - lo] + pred_bias[id - lo] by
 *   the per-row chain of the whole-table kernel of the same route (the fused scorer where d % 4 == 0, 16 <= d <= 1024, L <= 8192;
 *   k_tr_score_loss otherwise), t = (1 - eps) label + 1 / num_ent with the GLOBAL num_ent, the loss term and
 *   ds = (sigmoid(s) - t) / (B L): ds[b, l] is the whole-table step's value bit for bit on any sharding.  dh_part[b] = sum of
 *   ds[b, l] E[id - lo] over the owned l in the whole-table kernel's order with the other shards' entries removed (a sample with no
 *   owned entry: an exact zero row); loss_part[0] the unnormalised sum in double, per-sample shares in ascending b.  d(ent_emb) and
 *   d(pred_bias) of the own rows by the ordered-rows route (coper_train_order_rows, which this call needs no switch for): a stable
 *   sort of the batch's ids into ascending (id, b, l), a wave per owned row, fmaf from 0.f in ascending (b, l), stored with `=` onto
 *   the rows the forward call zeroed -- no float atomics.  An entry of another shard costs no row read, no store and no loss term.
 * coper_train_shard_backward(h, dh_parts, loss_parts, G, loss_out, sumsq_part, stream): dh = dh_parts[0] + dh_parts[1] + ... in
 *   ascending g (device float [G, B, d]), the loss the same way in double (device double [G]; loss_out: optional device float [1], the
 *   batch loss: the mean over the labels of the score call that ran, B num_ent or B L).  Then the encoder's backward; the conv backward's d(img) rows are added to the OWNED e1 rows only (one writer per row,
 *   ascending b, onto what the score call stored; a row of another shard is dropped without a store).  Advances the dropout counter.
 *   sumsq_part: device double [1], the squared norm of this shard's d(ent_emb) and d(pred_bias), summed in one fixed order.
 * coper_train_shard_apply(h, sumsq_parts, G, stream): global squared norm = the small leaves' + sumsq_parts[0 .. G) in index order
 *   (device double [G], G <= 63); clip and AMSGrad over the small leaves and the own rows; the beta powers advance, inference caches
 *   go stale.
 * Bits: every output of a sharded step is the same across runs, handles and processes; the replicated leaves and their slots are
 *   byte-identical on every rank.  Where every shard is exactly one chunk (the last one ragged) and the global norm is <= clip_norm,
 *   loss, variables, slots and BN statistics are those of coper_train_step_csr on a deterministic whole-table handle with the same
 *   one_vs_all_chunk; otherwise only the association of a float / double sum differs.  Sampled steps: a shard [0, num_ent) with the
 *   global norm <= clip_norm leaves the bits of coper_train_step on a deterministic whole-table handle with ordered rows on (the
 *   norm itself to the last bits of a double sum), also where sampled and 1-vs-all steps alternate; on ANY sharding d(pred_bias)
 *   and every row of d(ent_emb) that no e1 of the batch names are that handle's bit for bit (ds and the segment sums are functions
 *   of the batch alone; the rows e1 names also take the conv backward's share, which depends on the association of dh).
 * On a sharded state coper_train_step*, coper_train_backward*, coper_train_forward*, coper_train_grads_export, coper_train_apply,
 *   coper_train_rows_backward / _export / _import / _apply and coper_train_order_rows return COPER_EUNSUPPORTED (the row calls with the
 *   deferred-rows mode off: COPER_ESTATE, as on every state); coper_train_grad / coper_train_slot of the two tables
 *   hand out the local rows, global_norm the global one.  Null pointers, G < 1, B <= 0: COPER_EINVAL.
 * Deferred rows on a shard (coper_train_defer_rows above, enabled before the state's first step): sampled steps whose table work follows the
 *   batch, not the shard's |E| / G rows.  The four calls keep their signatures and the exchanges stay the same three:
 *   - coper_train_shard_gather returns every owned row AS OF THE CURRENT UPDATE although the table may hold it several updates behind:
 *     the closed-form catch-up is applied in registers and only rows_out is written (e1 has duplicates: catching up in place would
 *     race) -- bit for bit the row a sync would leave; the table, the slots and the words keep their bytes; a row with gap 0 is
 *     returned as it stands, a row of another shard is a zero row.  Still no part of the state machine.
 *   - coper_train_shard_forward re-zeroes the gradient rows the step before listed (and clears their claim bits) instead of the two
 *     buffers whole; the small leaves are zeroed as ever.
 *   - coper_train_shard_score_lookup sorts all B (L + 1) ids FIRST; the unique ids are ascending, so the owned ones are one contiguous
 *     run: that run, as local rows, is the step's list (an empty run: count 0, dh_part an exact zero, no word written).  The listed
 *     rows are brought current in the table, then the scorer and the segment sums run as with the mode off.  The owned e1 rows are on
 *     the list (their ids are in the sort), so they are current before the backward call adds the conv share to them.
 *   - coper_train_shard_score_csr returns COPER_EUNSUPPORTED (a 1-vs-all step has a gradient in every row); the phase stays "score
 *     expected", coper_train_shard_score_lookup may follow.
 *   - coper_train_shard_backward: sumsq_part is the listed rows' squared norm (every other gradient row is zero), in partial sums of
 *     COPER_ORDER_SUMSQ_ROWS list positions folded in one fixed order.
 *   - coper_train_shard_apply: AMSGrad over the small leaves; the listed rows by the row update, which reads the same slots (slot 0,
 *     then the G shares in index order) and writes the rows' words; the mode's update counter advances.
 *   A shard [0, num_ent) in the mode leaves the bits of coper_train_step on a deterministic whole-table handle with ordered rows and
 *   deferred rows on (global norm <= clip_norm; the norm itself to the last bits of a double sum).  After a sync, a row that no step
 *   named equals that handle's row bit for bit on any sharding (a caught-up row is a function of its own words, the gap and the powers).
 *   With the mode off a sharded step launches what it launched before the mode existed and leaves the same bits.
 * Forward-only calls: coper_train_forward / coper_train_forward_csr restricted to the handle's rows -- the loss, the
 *   train-mode logits and h of a batch with nothing written.  Each is ONE call, accepted only between steps (when the state machine
 *   expects coper_train_shard_forward; in any other phase COPER_ESTATE, the text names the call expected next) and the phase does not
 *   move.  One exchange in front (e1_rows, formed as for a step), at most two small ones behind (the G loss doubles; pred_part).
 *   coper_train_shard_forward_lookup(h, e1, rel, e1_rows, lookup, labels, B, L, loss_part, pred_part, h_out, stream)
 *   coper_train_shard_forward_csr(h, e1, rel, e1_rows, lab_indptr, lab_idx, lab_row, n_rows, B, loss_part, pred_local, h_out, stream)
 *   - the arguments of coper_train_shard_forward and of the score call of the same label form, with their checks and their clamping of
 *     ids (e1 and rel are read, not kept).  The train-mode encoder runs on the whole batch from e1_rows as coper_train_forward runs it:
 *     the dropout masks of the NEXT step, batch statistics when batch_norm_train_stats is set, the moving statistics left alone.  The
 *     scorer is the score call's, by the same plan: the per-row chains and loss terms of the step that would follow.
 *   - loss_part (required): device double [1], this shard's unnormalised sum as the score calls hand it out; the batch loss is the sum
 *     over ranks divided by B L (sampled) or B num_ent (1-vs-all).
 *   - pred_part (optional): device float [B, L], the logit of every OWNED entry (the fma chain of coper_train_forward's pred_out) and an
 *     exact +0.0f everywhere else: every element has one non-zero addend over the ranks, their sum is exact.
 *   - pred_local (optional): device float [B, n_local], row stride n_local: the logits of the handle's own columns, local column c is
 *     entity shard_lo + c.  Nothing logit-sized needs to be exchanged.
 *   - h_out (optional): device float [B, d].
 *   - nothing is written: no variable, BN moving statistic, gradient buffer or optimizer slot; the dropout counter, what a step left
 *     for coper_train_grad (the global norm included), every deferred-rows word, claim bit and row list stay; the handle stays
 *     prepared.  The workspaces are free between steps and serve as scratch.  A shard [0, num_ent) returns the bits of
 *     coper_train_forward* on a deterministic whole-table handle with ordered rows; on any sharding the summed pred_part and h are
 *     that handle's bit for bit, the loss to the association of a double sum.
 *   - deferred rows: coper_train_shard_forward_csr returns COPER_EUNSUPPORTED.  coper_train_shard_forward_lookup scores every owned row
 *     AS OF THE CURRENT UPDATE without writing the table: the scorer's row load applies the closed-form catch-up to ent_emb's row and
 *     its pred_bias word in registers (as coper_train_shard_gather does for the input rows; gap 0: the row as it stands).  No sort, no
 *     list, no catch-up launch: the list of the step before keeps the re-zero it is owed.  Stronger than coper_train_forward on a
 *     whole-table handle, which catches rows up in place: a row caught up in two stages is rounded twice, and a monitoring call on a
 *     shard changes no later bit of training.  (The fused scorer keeps 9 bytes more per entry in LDS there: L <= 8192 still fits.)
 * Not built: entering the deferred-rows mode on a state that has already stepped; the row-block split step (coper_train_rows_*) on a shard; sorting the owned entries alone; the default
 *   (non-deterministic) mode; splitting the encoder's batch over ranks (the phase cuts it needs are those of "Synchronised batch
 *   statistics" below: not wired into the sharded calls); dense [B, num_ent]
 *   labels; overlap of the exchanges with compute. */
COPER_API int coper_train_init_sharded(coper_handle* h, const coper_train_config* cfg);
COPER_API int coper_train_sharded(const coper_handle* h);
COPER_API int coper_train_shard_gather(coper_handle* h, const int64_t* e1, int64_t B, float* rows_out, void* stream);
COPER_API int coper_train_shard_forward(coper_handle* h, const int64_t* e1, const int64_t* rel, const float* e1_rows, int64_t B,
                                        float* h_out, void* stream);
COPER_API int coper_train_shard_score_csr(coper_handle* h, const int64_t* lab_indptr, const int64_t* lab_idx, const int64_t* lab_row,
                                          int64_t n_rows, int64_t B, float* dh_part, double* loss_part, void* stream);
COPER_API int coper_train_shard_score_lookup(coper_handle* h, const int32_t* lookup, const float* labels, int64_t B, int64_t L,
                                             float* dh_part, double* loss_part, void* stream);
COPER_API int coper_train_shard_backward(coper_handle* h, const float* dh_parts, const double* loss_parts, int32_t G, float* loss_out,
                                         double* sumsq_part, void* stream);
COPER_API int coper_train_shard_apply(coper_handle* h, const double* sumsq_parts, int32_t G, void* stream);
COPER_API int coper_train_shard_forward_lookup(coper_handle* h, const int64_t* e1, const int64_t* rel, const float* e1_rows,
                                               const int32_t* lookup, const float* labels, int64_t B, int64_t L, double* loss_part,
                                               float* pred_part, float* h_out, void* stream);
COPER_API int coper_train_shard_forward_csr(coper_handle* h, const int64_t* e1, const int64_t* rel, const float* e1_rows,
                                            const int64_t* lab_indptr, const int64_t* lab_idx, const int64_t* lab_row, int64_t n_rows,
                                            int64_t B, double* loss_part, float* pred_local, float* h_out, void* stream);

/* Synchronised batch statistics: the backward in phases.  G data-parallel ranks each hold B samples of one batch of
 * B_global = G B samples (even shards; this rank's are samples [sample_offset, sample_offset + B) of it).  With
 * batch_norm_train_stats on, coper_train_backward normalises every shard by its own statistics; these calls take the statistics of
 * Conv1BN (over B_global Ho Wo positions) and FCBN (over B_global samples) over the WHOLE batch, in the forward formulas and in both BN
 * backward formulas.  After the caller's usual sum of the flat gradients over the ranks and coper_train_apply(flat, 1 / G), every rank
 * has made ONE step on the whole batch: its gradient, and its moving statistics (equal on every rank, nothing to average).
 *
 * The step is coper_train_sync_begin (or _csr) and four coper_train_sync_next.  Each call runs launches on the caller's stream up to
 * the next point where a batch-wide sum is needed, writes this rank's n doubles to part_out (a device buffer of part_cap doubles) and
 * returns n in *n_out -- a host value computed from the configuration, nothing is read back and no call synchronises the host once the
 * workspaces hold the shape.  The caller all-gathers the ranks' parts IN RANK ORDER and hands the [G][n] buffer to the next
 * coper_train_sync_next, which adds them in ascending g: every rank derives the same bits from the same buffer, no all-reduce order
 * enters.  When a call returns, everything it handed out is ordered on the caller's stream (the state's side streams are joined).
 *   begin:   zeroing, the conv filters, the conv; the column sums of Conv1BN's input            hands out 2 conv_num_channels
 *   next 1:  Conv1BN with the batch's statistics, ReLU, dropout, the dense layer; FCBN's column sums      2 ent_emb_size
 *   next 2:  FCBN, the scorer, the loss, the scorer's backward; FCBN's backward sums                      2 ent_emb_size
 *   next 3:  FCBN's backward, the dense layer's, the generators' chains; Conv1BN's backward sums          2 conv_num_channels
 *   next 4:  Conv1BN's backward, the conv's, the filters'                                                 0: the step is complete
 * *n_out == 0: the handle is exactly where coper_train_backward / _csr (rows = 0) or coper_train_rows_backward (rows = 1; the
 * deferred-rows mode is required) leaves it: gradients pending for coper_train_grads_export | _apply (coper_train_rows_export | _import |
 * _apply), the dropout counter moved once, the moving statistics updated.  With batch_norm_train_stats off there is nothing to
 * exchange: begin runs the whole backward and returns *n_out = 0.  coper_train_sync_part_len: the largest n of a step,
 * 2 * max(conv_num_channels, ent_emb_size).  coper_train_sync_phase: 0 no step open, 1 .. 4 the exchange the state waits for
 * (negative: -COPER_EINVAL for a NULL handle, -COPER_ESTATE without a training state).
 *   - loss_out receives the mean over THIS rank's labels (in next 2), as coper_train_backward's.
 *   - The gradients of the two layers' gamma and beta are this rank's share (its own sums): the caller's sum over ranks completes them.
 *   - Dropout masks are a function of the element's position in the WHOLE batch: sample sample_offset + b draws what sample
 *     sample_offset + b of one handle's B_global-sample step draws, so the G shards draw that step's masks.
 *   - The batch's buffers (e1, rel, lookup, labels, the label lists) are read by later phases: they stay valid and unchanged until the
 *     step is complete or abandoned.  A world of one (G = 1, its own part handed back) leaves the bits of coper_train_backward in
 *     deterministic mode.
 *   - Any step-shaped call while a step is open (coper_train_step*, _backward*, _forward*, _rows_backward, another begin) abandons it,
 *     as a pending coper_train_backward is dropped: each zeroes the accumulators first.  coper_train_grads_export / _apply /
 *     _rows_export / _rows_apply in the middle of a step return COPER_ESTATE.  A coper_train_sync_next that fails leaves no step open.
 * Refused: no training state, or coper_train_sync_next with no step open: COPER_ESTATE.  rows not 0 or 1; B_global no multiple of B or
 *   sample_offset + B > B_global; part_cap below the call's n; NULL or misaligned (8 bytes) buffers; G < 1; (sample_offset + B)
 *   features past the 32-bit dropout counter: COPER_EINVAL.  rows = 1 outside the deferred-rows mode: COPER_ESTATE; rows = 0 inside it,
 *   and an entity-sharded state: COPER_EUNSUPPORTED.  A generator with hidden layers (context_rel_out / context_rel_conv) AND
 *   context_rel_use_batch_norm AND batch statistics on: COPER_EUNSUPPORTED -- its hidden BN layers take statistics over the batch as
 *   well, and synchronising them is deliberately not built (hidden layers without context BN are served).
 * Left out: a synchronised coper_train_forward; statistics across micro-batches; overlap of the exchanges with compute; graph capture
 *   of the phase calls. */
COPER_API int coper_train_sync_begin(coper_handle* h, const int64_t* e1, const int64_t* rel, const int32_t* lookup, const float* labels,
                                     int64_t B, int64_t L, int64_t B_global, int64_t sample_offset, int32_t rows, double* part_out,
                                     int64_t part_cap, int64_t* n_out, float* loss_out, void* stream);
COPER_API int coper_train_sync_begin_csr(coper_handle* h, const int64_t* e1, const int64_t* rel, const int64_t* lab_indptr,
                                         const int64_t* lab_idx, const int64_t* lab_row, int64_t n_rows, int64_t B, int64_t B_global,
                                         int64_t sample_offset, double* part_out, int64_t part_cap, int64_t* n_out, float* loss_out,
                                         void* stream);
COPER_API int coper_train_sync_next(coper_handle* h, const double* parts_in /* [G][n] of the last n_out */, int32_t G, double* part_out,
                                    int64_t part_cap, int64_t* n_out, void* stream);
COPER_API int coper_train_sync_phase(const coper_handle* h);
COPER_API int64_t coper_train_sync_part_len(const coper_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* COPER_HIP_H_ */
