/* mfas_hip.h — C ABI of the MI355X-native MFAS inner candidate-training engine.
 *
 * The reference (jperezrua/mfas) has no native/FFI layer: its hot path is Python calling PyTorch.
 * These entry points are what a binding for that path replaces (reference file:line cited per
 * function).  Plain pointers and sizes only; every tensor pointer is a DEVICE pointer owned by the
 * caller unless stated otherwise; functions return 0 on success or a negative MFAS_E* code and never
 * throw across the boundary.  One population handle is driven by one host thread on one HIP stream.
 */
#ifndef MFAS_HIP_H
#define MFAS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFAS_OK 0
#define MFAS_EINVAL -1   /* bad argument / unsupported hyper-parameter combination */
#define MFAS_EHIP -2     /* a HIP runtime call failed; see mfas_last_error() */
#define MFAS_ENOMEM -3

#define MFAS_MAX_CELLS 4 /* max_fusions (main_searchable_ntu.py:39) */
#define MFAS_MAX_TAPS 8  /* tap slots per modality (NTU uses 4+4, AV-MNIST 5+3, MM-IMDB 2+4) */

#define MFAS_DT_F32 0
#define MFAS_DT_BF16 1
#define MFAS_DT_F16 2

/* The `args` fields the path reads (models/search/ntu_searchable.py:28-84,200-292) plus the Adam
 * constants fixed at ntu_searchable.py:65 (weight_decay=1e-4, torch defaults otherwise). */
typedef struct mfas_hyper {
    int32_t R;          /* args.inner_representation_size */
    int32_t C;          /* args.num_outputs */
    int32_t B;          /* args.batchsize */
    int32_t bn;         /* args.batchnorm */
    int32_t alphas;     /* args.alphas */
    int32_t multitask;  /* args.multitask: argmax over central+visual+skeleton logits */
    double drpt;        /* args.drpt (<=1e-10: no Dropout module) */
    double wd, beta1, beta2, adam_eps, bn_eps, bn_momentum;
    int32_t s_sizes[MFAS_MAX_TAPS]; /* first-modality tap widths (skeleton: ntu_searchable.py:291; audio:
                                     * avmnist_searchable.py:290-292); 0 = unused slot.  Any width >= 1: tables store
                                     * each row padded with zeros to a multiple of 16 elements. */
    int32_t v_sizes[MFAS_MAX_TAPS]; /* second-modality tap widths (visual: ntu_searchable.py:292) */
    /* Head loss / dev metric.  0: CrossEntropyLoss + top-1 accuracy (NTU, ntu_searchable.py:31).
     * 1: multi-label WeightedCrossEntropyWithLogits (models/central/mm_imdb.py:655-673) + F1 'samples' of
     *    sigmoid(logits) > f1_threshold (models/search/train_searchable/mmimdb.py:86,105). */
    int32_t loss_mode;
    int32_t allow_plain_cell; /* 1: [Linear, nl] cells (no BN, no Dropout) are legal (avmnist_searchable.py:276-285); the
                               * NTU searchable leaves that case undefined (ntu_searchable.py:274-284) */
    double f1_threshold; /* th_fscore, mmimdb.py:16 (0.3) */
    int32_t tap_bits;    /* hint: element size of the feature tables this population will train on (16: bf16 / f16 taps, the
                          * layout north_star prescribes; 32: f32; 0: unknown = any).  With 16 the engine may size resident
                          * feature units for 16-bit staging (up to 1024 columns each); training such a population on f32
                          * tables is refused with MFAS_EINVAL. */
    int32_t order_per_candidate; /* 0: one sample order per epoch shared by the whole population (lockstep: `order` of
                          * mfas_population_train holds [epochs][N_train]); 1: every candidate walks its OWN permutations — the
                          * reference draws a fresh DataLoader(shuffle=True) order per candidate and epoch
                          * (models/searchable.py:248-250, train_searchable/ntu.py:35) — `order` then holds [K][epochs][N_train]. */
} mfas_hyper;

/* Pooled feature table = what Visual/Skeleton.forward + GlobalPooling2D hand to the fusion net
 * (models/central/ntu.py:35-50,129-183; ntu_searchable.py:211-225) for N samples, plus labels
 * (datasets/ntu.py:254). */
typedef struct mfas_table {
    const void* s[MFAS_MAX_TAPS]; /* (N, ceil16(width)) row-major, zero padded */
    const void* v[MFAS_MAX_TAPS];
    const float* vlogit; /* (N, C) unimodal logits for multitask, or NULL */
    const float* slogit;
    const int32_t* label; /* (N) in [0, C); loss_mode 0 */
    const float* multilabel; /* (N, C) 0/1 targets; loss_mode 1 (else NULL) */
    int64_t N;
    int32_t dtype; /* MFAS_DT_* of s[]/v[] */
    int32_t _pad;
} mfas_table;

/* Per-epoch statistics train_ntu_track_acc accumulates (train_searchable/ntu.py:72-79). */
typedef struct mfas_epoch_stats {
    double train_loss_sum; /* sum over samples of the CE loss (running_loss) */
    double dev_loss_sum;
    int64_t train_corrects; /* running_corrects (loss_mode 0) */
    int64_t dev_corrects;   /* loss_mode 0: correct predictions; loss_mode 1: round(2^32 * sum over samples of F1) */
} mfas_epoch_stats;

typedef struct mfas_population mfas_population; /* opaque; owns its device workspace */

const char* mfas_last_error(void);
int mfas_version(void);
/* "mfas-src-digest:<16 hex>": sha256 prefix of the sources (the csrc .hip / .hip.h files and this header) the loaded library
 * was compiled from; __graft_entry__.build() rebuilds when it differs from the tree and tests assert it matches. */
const char* mfas_source_digest(void);

/* Replaces the model/optimizer construction half of train_sampled_models' population loop
 * (ntu_searchable.py:38-72): K candidates, confs[k][cell][{ske_tap, vis_tap, nonlinearity}],
 * n_cells[k] rows used.  drop_seeds[k] seeds candidate k's dropout stream (NULL: 0..K-1).
 * chunk_cols: feature-column chunk per workgroup (0 = auto). */
int mfas_population_create(const mfas_hyper* hp, const int32_t* confs /* K*4*3 */,
                           const int32_t* n_cells /* K */, const uint32_t* drop_seeds, int32_t K,
                           int32_t device, void* hip_stream, int32_t chunk_cols,
                           mfas_population** out);
void mfas_population_destroy(mfas_population* pop);

/* Number of floats of candidate k's central parameters in reference state_dict order:
 * alphas.i.alpha_x (L), then per cell fusion_layers.i.0.weight (R x K_i row-major), .0.bias (R),
 * [.2.weight, .2.bias, .2.running_mean, .2.running_var (R each) if bn], then
 * central_classifier.weight (C x R), central_classifier.bias (C)   (ntu_searchable.py:191-200). */
int64_t mfas_population_param_count(const mfas_population* pop, int32_t k);

/* Load / read back candidate k's parameters (device float buffers in the order above).
 * plane 0 = parameters, 1 = Adam exp_avg, 2 = Adam exp_avg_sq, 3 (get only; mfas_population_set_state writes it) = the kept
 * best-epoch parameters of a snapshot_best schedule driven through mfas_population_train_from (MFAS_EINVAL when candidate k keeps
 * none).  set() also zeroes the Adam state and the step counter (a fresh torch.optim.Adam, ntu_searchable.py:65). */
int mfas_population_set_params(mfas_population* pop, int32_t k, const float* flat);
int mfas_population_get_params(mfas_population* pop, int32_t k, int32_t plane, float* flat);

/* Device-side PyTorch-default-shaped init (U(+-1/sqrt(fan_in)), BN gamma=1/beta=0/rm=0/rv=1,
 * alpha = 0.1*noise) from the hash generator documented in oracle/np_oracle.py:init_params. */
int mfas_population_init(mfas_population* pop, const uint32_t* seeds /* K, host */);

/* (new, round 4) The reference's OWN initial parameters, drawn on the device: what `searchable_type(args, conf)` — the model
 * construction at ntu_searchable.py:44 (nn.Linear.reset_parameters per cell and for the classifier, then alpha ~ N(mean, std),
 * ntu_searchable.py:202-204) — draws from torch's CPU generator after torch.manual_seed(seeds[k]): at::mt19937 and
 * uniform_real_distribution<float> run per candidate on the GPU, bit for bit the numbers of the host path (the Python mirror checks
 * that once per process against torch itself and falls back to mfas_population_set_params otherwise).
 * seeds: HOST uint64[K].  bounds: HOST float[K][2 * (MFAS_MAX_CELLS + 1)] = per cell {weight bound, bias bound} (unused cells: any),
 * then the classifier's {weight bound, bias bound}: Tensor.uniform_(-bound, bound).  BatchNorm starts at its defaults; Adam state
 * is zeroed (as mfas_population_set_params does). */
int mfas_population_init_torch_streams(mfas_population* pop, const uint64_t* seeds, const float* bounds, double alpha_mean,
                                       double alpha_std);

/* Replaces train_ntu_track_acc (train_searchable/ntu.py:14-89) for the whole population in lockstep:
 * for each epoch: train over `train` in the given sample order (order: device int32 [epochs][N_train],
 * NULL = sequential), then evaluate `dev`.  step_scalars: HOST float2 per train step
 * {lr_t/(1-beta1^t), sqrt(1-beta2^t)} (scheduler.py:25-46 + torch Adam bias corrections).
 * max_steps >= 0 stops after that many train steps in all, counted across epochs (an epoch that starts is cut short; later
 * epochs do not run; debug/known-answer tests; dev evaluation is skipped).  stats: HOST [K][epochs].  status: HOST [K], 1 =
 * non-finite loss seen.
 * snapshot_best != 0 keeps the best-dev-epoch parameters and restores them at the end (:82-86).
 * Every call starts from zeroed Adam moments and step count (a freshly constructed optimizer); a schedule that has to stop and go
 * on is driven through mfas_population_train_from below. */
int mfas_population_train(mfas_population* pop, const mfas_table* train, const mfas_table* dev,
                          const int32_t* order, const float* step_scalars, int32_t epochs,
                          int64_t max_steps, int32_t snapshot_best, mfas_epoch_stats* stats,
                          int32_t* status);

/* ---- Resume: stop after an epoch and go on later — in the same handle, in another population, from a file -------------------
 * What train_ntu_track_acc keeps on its stack for the length of one call (train_searchable/ntu.py:17-18: best_model_sd = a copy
 * of the initial state_dict, best_acc = 0; :82-86: strict '>' replaces both, the best state is loaded at the end) and what
 * torch.optim.Adam keeps in its state (exp_avg, exp_avg_sq, step) is kept in the population between calls instead: planes 1 / 2,
 * the kept best-epoch plane 3, and a per-candidate PROGRESS RECORD {epochs of the schedule that are complete, the schedule's
 * batches per epoch nb, best dev metric so far, whether the schedule keeps the best epoch}.  The step counter needs no storage:
 * step t of epoch e is e * nb + t for the step scalars, the dropout stream, the sample order and the statistics slot alike, and
 * nothing in the step buffers crosses an epoch boundary — a schedule run in segments is BIT-IDENTICAL to the one-call run. */

/* Epochs [first_epoch, last_epoch) of a schedule of `epochs` epochs.  order, step_scalars and stats are indexed exactly as in
 * mfas_population_train and sized for the WHOLE schedule; stats columns outside the segment come back zero.
 * first_epoch == 0 does what mfas_population_train does at entry: zeroes the Adam moments, sets every best metric to the best
 * threshold and the kept best parameters to a copy of the initial ones (:17-18), clears status.  first_epoch > 0 zeroes nothing
 * (status is sticky across segments) and requires every candidate's progress record to say that exactly first_epoch epochs of a
 * schedule with the same nb and the same snapshot_best are complete — otherwise MFAS_EINVAL (the message names both numbers) and
 * nothing is changed.  snapshot_best restores the best parameters (:86) only when last_epoch == epochs: an unfinished schedule is
 * left with its LIVE parameters in plane 0 and the kept best in plane 3.  There is no max_steps here.
 * mfas_population_train itself is unchanged; it RESETS the record (0 epochs complete). */
int mfas_population_train_from(mfas_population* pop, const mfas_table* train, const mfas_table* dev, const int32_t* order,
                               const float* step_scalars, int32_t epochs, int32_t first_epoch, int32_t last_epoch,
                               int32_t snapshot_best, mfas_epoch_stats* stats, int32_t* status);

/* Write ONE plane of candidate k from a device float buffer in the state_dict order above and touch nothing else: plane 1 / 2 =
 * Adam exp_avg / exp_avg_sq, 3 = the kept best-epoch parameters (the candidate's record then says its schedule keeps the best
 * epoch).  Plane 0 stays with mfas_population_set_params (which zeroes the moments: write them AFTER it).  Asynchronous on the
 * population's stream like set_params: keep `flat` alive until the stream has been synchronised. */
int mfas_population_set_state(mfas_population* pop, int32_t k, int32_t plane, const float* flat);

/* Candidate k's progress record and status word (HOST pointers).  get: every pointer may be NULL.  set: a NULL pointer leaves
 * that entry as it is; epochs_done = 0 makes the candidate a fresh one (its record no longer keeps a best epoch). */
int mfas_population_get_progress(mfas_population* pop, int32_t k, int64_t* epochs_done, int64_t* nb, double* best_metric,
                                 int32_t* status);
int mfas_population_set_progress(mfas_population* pop, int32_t k, const int64_t* epochs_done, const int64_t* nb,
                                 const double* best_metric, const int32_t* status);

/* Candidate ks of `src` into slot kd of `dst` with everything it trains on: W, m, v, the kept best, the BatchNorm running
 * statistics, the progress record and the status word.  Device to device on dst's stream through the flat state_dict order — the
 * two populations' layouts may differ (chunk size, resident or not, wide or not); no host copy, and the only synchronisation is
 * that of src's stream when it is not dst's.  MFAS_EINVAL when the two candidates' configurations, or the hyper-parameters that
 * define a candidate's parameters (R, C, bn, alphas, tap widths), differ.  The dropout seed belongs to the SLOT: create dst with
 * the seed the moved candidate trained under. */
int mfas_population_move(mfas_population* dst, int32_t kd, mfas_population* src, int32_t ks);

/* Replaces Searchable_Skeleton_Image_Net.forward in eval mode (ntu_searchable.py:206-247) for
 * candidate k on rows [row0, row0+nrows) of a table: writes logits (nrows, C) (device, row-major);
 * and test_ntu_track_acc (train_searchable/ntu.py:92-125) when corrects != NULL (HOST int64). */
int mfas_population_forward(mfas_population* pop, int32_t k, const mfas_table* tab, int64_t row0,
                            int64_t nrows, float* logits, int64_t* corrects);

/* Scores M candidates of the population on every row of a table, one by one AND together, in one call: the population form of
 * test_ntu_track_acc (train_searchable/ntu.py:92-125; main_found_ntu.py lists five found configurations).  No reference counterpart
 * for the ensemble.  Every member runs in eval mode exactly as the dev pass of mfas_population_train does (the same kernel, the same
 * statistics path: member_stats ARE the dev pass's dev_loss_sum / dev_corrects for that table).
 *   plane:    0 = the live parameters, 3 = the kept best-epoch parameters of an unfinished snapshot_best schedule (MFAS_EINVAL when
 *             a member keeps none, as mfas_population_get_params).
 *   members:  HOST [M] candidate indices, repeats allowed; NULL = 0..K-1 (M must then be K).
 *   weights:  HOST [M], each finite and >= 0, sum > 0; NULL = uniform.  Normalised on the host in double, then rounded to float.
 *   combine:  a member's SCORE row z is its logits (multitask: (logits + vlogit) + slogit in float32, what the dev pass compares);
 *             its PROBABILITY row is softmax(z - max z) (loss_mode 1: sigmoid(z)).
 *             0: the ensemble's probabilities are sum_m w_m * p_m, summed in list order; 1: they are the probability row of
 *             sum_m w_m * z_m.
 *   decision: loss_mode 0: the FIRST maximum of the ensemble's probabilities (ties to the lower class, like the dev pass);
 *             loss_mode 1: probability > f1_threshold, F1 'samples' in 32.32 fixed point like the dev pass.
 *   loss:     loss_mode 0: -log max(p[label], 2^-126) per row; loss_mode 1 with combine 1: the weighted BCE of the mean score;
 *             loss_mode 1 with combine 0: REPORTED AS 0 (a mean of probabilities has no score to take the BCE of).
 *   scratch_bytes: device scratch for the members' logits of one block of rows (0 = 64 MiB; at least one row of M * C floats): the
 *             table is walked in row blocks of that size.  The ensemble's outputs are bit-identical for every value.
 *   member_stats: HOST [M] or NULL (train_* = 0).  member_preds: DEVICE int32 [M][N] or NULL, every member's own decision
 *             (loss_mode 0 only).  scores: DEVICE float (N, C) or NULL, the ensemble's probabilities.  ensemble_stats: HOST [1] or
 *             NULL: dev_loss_sum / dev_corrects of the ensemble (train_* = 0).
 * Nothing a later train call reads is touched (parameters, moments, kept best, progress, status, statistics, the launch record):
 * the call works in an arena of its own on the population's stream and synchronises once, for the final copy of the statistics.
 * MFAS_EINVAL, with a message naming the value, and nothing changed: a member index outside [0, K); M <= 0; members == NULL with
 * M != K; a negative or non-finite weight or a zero weight sum; plane not 0 / 3; combine not 0 / 1; member_preds with loss_mode 1;
 * scratch_bytes below one row; a table mfas_population_forward refuses. */
int mfas_population_evaluate(mfas_population* pop, const mfas_table* tab, int32_t plane, const int32_t* members,
                             const float* weights, int32_t M, int32_t combine, int64_t scratch_bytes,
                             mfas_epoch_stats* member_stats, int32_t* member_preds, float* scores,
                             mfas_epoch_stats* ensemble_stats);

/* mfas_population_evaluate with a per-class report: the same twelve parameters, unchanged in order and meaning, then three DEVICE
 * arrays, any of which may be NULL.  Slot s of an array is member s of the list for s < M and the ensemble for s = M.
 *   confusion:    int64 [(M+1)][C][C], loss_mode 0 only: [s][t][q] = the rows with label t that slot s decided as q (a member's
 *                 decision is member_preds' bit for bit, the ensemble's the first maximum of `scores`; a NaN in class 0 decides 0).
 *   rank_hist:    int64 [(M+1)][C], loss_mode 0 only: [s][r] = the rows whose label has rank r in slot s's score row (a member's
 *                 score row, the ensemble's probabilities).  The rank is the number of classes that precede the label in the order
 *                 "score descending, NaN last, equal scores by lower class first"; its running sum up to k-1 is the top-k count.
 *                 Rank 0 coincides with "decided correctly" on every row whose class-0 score is not NaN.
 *   label_counts: int64 [(M+1)][C][3], loss_mode 1 only: per class (true positives, predicted positives, actual positives); a
 *                 member predicts a class when sigmoid(z) > f1_threshold, the ensemble when its probability does, and a class is
 *                 actual when multilabel > 0.5.
 * The call zeroes the arrays it was given on the population's stream, then adds integers only: the arrays depend neither on the run
 * nor on scratch_bytes.  Every other output is bit-identical to mfas_population_evaluate's, and with all three NULL the call IS that
 * one.  MFAS_EINVAL, naming the argument, nothing changed: confusion or rank_hist with loss_mode 1; label_counts with loss_mode 0;
 * a report of more than 65534 members; everything mfas_population_evaluate refuses. */
int mfas_population_evaluate_report(mfas_population* pop, const mfas_table* tab, int32_t plane, const int32_t* members,
                                    const float* weights, int32_t M, int32_t combine, int64_t scratch_bytes,
                                    mfas_epoch_stats* member_stats, int32_t* member_preds, float* scores,
                                    mfas_epoch_stats* ensemble_stats, int64_t* confusion, int64_t* rank_hist,
                                    int64_t* label_counts);

/* Replaces Searchable_Skeleton_Image_Net.forward in TRAIN mode (ntu_searchable.py:206-247 with model.train(True)) for
 * candidate k on ONE batch = rows [row0, row0+nrows) of a table, nrows <= hyper.B: batch-statistics BatchNorm (the running
 * statistics are updated, as any train-mode forward does), dropout from the candidate's stream at `step_index`; writes
 * logits (nrows, C) (device).  No gradient is produced: the train loop (forward + backward + Adam) is mfas_population_train. */
int mfas_population_forward_train(mfas_population* pop, int32_t k, const mfas_table* tab, int64_t row0, int32_t nrows,
                                  int32_t step_index, float* logits);

/* (new, round 3) The autograd half of that forward: the gradients of an EXTERNAL loss of the same batch with respect to every
 * central parameter (loss.backward() on the logits of Searchable_Skeleton_Image_Net.forward under model.train(True),
 * /root/reference/models/search/ntu_searchable.py:206-247, for callers that write their own training loop).  The batch is run
 * again in train mode with the same dropout stream (`step_index`) and batch statistics, `dlogits` (DEVICE, nrows x C float32
 * = dL/dlogits) takes the place of the loss gradient, and each parameter's gradient is left in its Adam first-moment slot:
 * read it with mfas_population_get_params(pop, k, 1, flat).  Parameters are not changed.  Candidate k's Adam moment slots are
 * ZEROED at entry (the gradient is accumulated into the first-moment slot from 0, whatever the handle trained before) and are
 * scratch afterwards, like the BN running statistics: the optimizer state of candidate k does not survive this call — use a
 * population kept for the purpose (the Python mirror builds one per call). */
int mfas_population_backward(mfas_population* pop, int32_t k, const mfas_table* table, int64_t row0, int32_t nrows,
                             int32_t step_index, const float* dlogits);

/* mfas_population_backward, and the gradients of the same loss with respect to the feature TAPS of the batch as well: the reference's
 * module is an ordinary nn.Module whose inputs get gradients (Searchable_Skeleton_Image_Net.forward under model.train(True),
 * models/search/ntu_searchable.py:206-247 of the reference, behind a backbone, adapter or projection that learns).  Everything
 * mfas_population_backward does, this call does identically — parameter gradients in the first-moment slots, moments scratch, running
 * statistics moved.  In addition, for every non-NULL ds[j] / dv[j] it writes d loss / d tap as a row-major (nrows, width) float32
 * array with leading dimension s_sizes[j] / v_sizes[j]: the sum over the cells i of candidate k that select the tap, ascending i, of
 * scale_i * dy_i * W_i[:, tap columns], scale_i = sigmoid(alpha_i) for S and 1 - sigmoid(alpha_i) for V with alphas, 1 without (one
 * k_tap_grad launch behind the backward chain, before the call's one synchronise; fixed summation order: the same bits on every run,
 * whichever other taps are requested).  A requested tap no cell of candidate k selects receives zeros.  ds / dv are HOST arrays of
 * MFAS_MAX_TAPS DEVICE pointers; either array may be NULL, and with no pointer set the call IS mfas_population_backward.
 * MFAS_EINVAL, naming the slot, with nothing launched and nothing changed: a non-NULL pointer for a slot of width 0; and everything
 * mfas_population_backward refuses.  One candidate and one batch per call; float32 output only. */
int mfas_population_backward_taps(mfas_population* pop, int32_t k, const mfas_table* table, int64_t row0, int32_t nrows,
                                  int32_t step_index, const float* dlogits,
                                  float* const* ds /* HOST [MFAS_MAX_TAPS] of DEVICE (nrows, s_sizes[j]) or NULL */,
                                  float* const* dv /* likewise, v_sizes[j] */);

/* Timing of the dominant kernel (fused cell sweep) over the last train() call, measured with HIP
 * events on the population's stream: number of launches, summed milliseconds, and the algorithmic
 * HBM bytes of one update+forward launch (24*P_tiles + feature bytes). */
int mfas_population_sweep_profile(const mfas_population* pop, int64_t* launches, double* total_ms,
                                  double* bytes_per_launch);
int mfas_population_set_profiling(mfas_population* pop, int32_t on);

/* (new) The step schedule this population was laid out for, so that a measurement can name the kernel it
 * timed: info[0] = 1 persistent step loop (k_president: resident units + resident chain, one launch per epoch) / 0 launch per phase (k_step / k_chain);
 * info[1] = feature units resident in registers; info[2] = their workgroups; info[3] = units per resident workgroup;
 * info[4] = 1 when the resident lean chain owns OUT/HEAD; info[5] = bit 0: lean chain (R <= 16), bit 1: the WIDE path (k_chain_wide +
 * k_sweep_wide, launch per phase, the batch walked in tiles: batchsize > 64, more classes than the batch-resident softmax takes, or a
 * step beyond the LDS; info[0] = 0 and info[6] = 1 then), bits 8..15: compute units one
 * candidate's general chain runs on in the same-group launch (round 6, chain_split; 1 otherwise); info[6] = candidate groups of the
 * launch-per-phase schedule (2 = fused A/B launches, 1 = chain and sweep back to back, -1 = one launch per step holding the chain
 * AND the sweep of the same candidates, released cell by cell through per-cell flags); info[7] = candidates. */
int mfas_population_schedule(const mfas_population* pop, int32_t info[8]);

/* The kernel builds the LAST mfas_population_train / mfas_population_train_from call of this population launched, as the library
 * recorded them where it made the launches: "k_step<1,1,4,0,1>:7 k_chain<1,0>:8 ..." — one item per distinct build, the kernel
 * family with the instantiation's template arguments, a colon and the number of launches; items sorted by name, separated by one
 * space, NUL-terminated, truncated to `cap`.  Families and their arguments: k_step<MB,NT,WPE,LEAN,NS>, k_step_same<MB,NT,NS>,
 * k_chain<MB,LEAN>, k_chain_wide, k_sweep_wide<NT>, k_president<MB,NTR,X16,NU,PLAIN> (MB: 16-row batch tiles; NT: nontemporal W/m/v
 * streaming; WPE: waves per SIMD the build is bounded for; LEAN: the R <= 16 chain; NS: workgroups per candidate chain; NTR: tiles
 * per wave of a resident unit; X16: 16-bit staging; NU: units per resident workgroup; PLAIN: 0 general chain, 1 search default,
 * 2 BatchNorm alone).  The name and the function pointer of a launch come from one template instantiation, so the record names
 * what ran, not what the plan implies.  A call that is refused leaves the previous record; a call that passes its checks starts an
 * empty one; a resident call that falls back to launch per phase keeps both parts.  The dev pass (k_eval), the packers and the
 * single-batch entry points (forward_train / backward) are not recorded.  Tests use it to assert a build by name; no reference
 * counterpart. */
int mfas_population_launch_record(const mfas_population* pop, char* buf, int32_t cap);

/* (new, round 3) The same decision WITHOUT creating a population — a pure query, nothing is allocated or launched: would
 * mfas_population_create(hp, confs, n_cells, ..., K, device, ..., chunk_cols) take the resident persistent schedule (every
 * chain and every feature unit resident on its own CU slot, W/m/v in registers, one launch per epoch)?  The host plans
 * resident ROUNDS with it (a share of a train_sampled_models call — /root/reference/models/search/ntu_searchable.py:38-94 trains
 * the configurations one after the other — that is too large for one resident population is trained as several).
 * info[0] = 1 resident persistent schedule / 0 launch per phase; info[1] = resident feature units; info[2] = their workgroups;
 * info[3] = units per resident workgroup; info[4] = feature-column chunk; info[5] = bit 0: lean chain (R <= 16, C <= 64, B <= 32),
 * bit 1: the wide path (no resident form at any K);
 * info[6] = compute units of the device; info[7] = K. */
int mfas_population_plan(const mfas_hyper* hp, const int32_t* confs, const int32_t* n_cells, int32_t K, int32_t device,
                         int32_t chunk_cols, int32_t info[8]);

/* (new) Streaming ceiling of this device for the sweep's access pattern: three planes of `bytes_per_plane` are
 * read-modify-written in 1 KiB tiles with nontemporal 16 B/lane accesses and no compute; returns GB/s (read + write). */
int mfas_stream_probe(int64_t bytes_per_plane, int32_t iters, double* gb_per_s);

/* Replaces GlobalPooling2D.forward (models/auxiliary/aux_models.py:54-64; applied at ntu_searchable.py:224-225): mean over
 * the `inner` trailing elements of each of the rows = B*C contiguous rows of a backbone tap (B, C, ...) -> out[rows].
 * x / out are device pointers of dtype MFAS_DT_* ; f32 accumulation.  The step that builds an mfas_table from raw taps. */
int mfas_global_pool(const void* x, int32_t dtype, int64_t rows, int64_t inner, void* out, int32_t out_dtype,
                     void* hip_stream);

/* (new, round 4) Profiler ranges (roctx markers; no-ops when the marker library is not loadable): mfas_population_train opens one
 * range per call and one per epoch itself; the host side brackets each train_sampled_models call
 * (/root/reference/models/search/ntu_searchable.py:23-102) with these.  Always return MFAS_OK. */
int mfas_range_push(const char* name);
int mfas_range_pop(void);

/* (new, round 6) The library's environment switches (A/B and debugging aids; INTEGRATION.md lists them) as parsed from the CURRENT
 * environment: "name=value name=value ..." in declaration order, NUL-terminated, truncated to `cap`.  The library parses them in ONE
 * place, when a population is created or planned (the reference has no counterpart: its knobs are the argparse flags of
 * /root/reference/main_searchable_ntu.py:16-63, mirrored by mfas_hyper); a population keeps the set it was created under.  An empty
 * environment yields the defaults the test suites run ("hooks=0": the product library parses no test hook). */
int mfas_tuning_describe(char* buf, int32_t cap);

/* ---- The search controller's surrogate (models/search/surrogate.py:15-60, 133-157): Linear(n_in, E) + Sigmoid -> one LSTM(E, H)
 * layer over the cells (h0 = c0 = 0, gates i, f, g, o) -> Linear(H, 1) + Sigmoid, trained with MSELoss and torch.optim.Adam.
 * Stateless: no handle, the caller owns every buffer, the calls run on the calling thread's current device.  Parameters (and both
 * Adam moments) are ONE flat float32 device buffer each, in state_dict order: embedding.0.weight (E x n_in), embedding.0.bias (E),
 * lstm.weight_ih_l0 (4H x E), lstm.weight_hh_l0 (4H x H), lstm.bias_ih_l0 (4H), lstm.bias_hh_l0 (4H), hid2val.weight (1 x H),
 * hid2val.bias (1).  MFAS_EINVAL (the message names the value; nothing is launched, no HIP call is made): n_in outside 1..8, E or H
 * outside 16..128, L outside 1..MFAS_MAX_CELLS, n < 1, n_buckets < 1, epochs < 1, a scratch smaller than the scratch query says, a
 * null pointer, a beta outside [0, 1), eps < 0. */
typedef struct mfas_surrogate_shape { int32_t n_in, E, H, _pad; } mfas_surrogate_shape;
int64_t mfas_surrogate_param_count(const mfas_surrogate_shape* shape); /* 81301 for {3, 100, 100} */
/* Bytes of device scratch a train call needs when no bucket has more than max_L cells or max_n rows (16-byte aligned; its contents
 * mean nothing between calls; a larger buffer changes no result). */
int64_t mfas_surrogate_scratch_bytes(const mfas_surrogate_shape* shape, int32_t max_L, int64_t max_n);
/* train_simple_surrogate (surrogate.py:133-157): `epochs` passes over the buckets in list order, one Adam step per bucket (two
 * launches: the tiles' partial gradients, then their sum in tile order + Adam; no atomics, so a call is bit-reproducible), ONE
 * synchronisation at the end for last_loss = the loss the LAST step computed, before its update.  *step: Adam steps taken so far
 * (0 with zeroed moments for a fresh optimizer), advanced by epochs * n_buckets; a run split into several calls is bit-identical
 * to the one-call run. */
int mfas_surrogate_train(const mfas_surrogate_shape* shape, float* params, float* exp_avg, float* exp_avg_sq,
                         int64_t* step /* HOST, in/out */,
                         const float* const* x /* HOST array of DEVICE (L_b, n_b, n_in) */, const float* const* y /* ... DEVICE (n_b) */,
                         const int32_t* L /* HOST */, const int64_t* n /* HOST */, int32_t n_buckets, int32_t epochs,
                         double lr, double beta1, double beta2, double eps, double weight_decay,
                         void* scratch, int64_t scratch_bytes, void* hip_stream, float* last_loss /* HOST */);
/* The forward alone, through the same device code as the train step's: x DEVICE (L, n, n_in) -> pred DEVICE (n).  Asynchronous on
 * hip_stream.  The forward keeps nothing outside LDS: scratch is not touched (NULL / 0 is fine). */
int mfas_surrogate_forward(const mfas_surrogate_shape* shape, const float* params, const float* x, int32_t L, int64_t n,
                           float* pred /* DEVICE (n) */, void* scratch, int64_t scratch_bytes, void* hip_stream);

/* snapshot_best bookkeeping: a dev metric must EXCEED `threshold` to replace the kept parameters (best_acc = 0,
 * train_searchable/ntu.py:18; best_f1 = init_f1, train_searchable/mmimdb.py:18).  Default 0.  If no epoch exceeds it the
 * INITIAL parameters are restored, like the reference's best_model_sd (ntu.py:17,86). */
int mfas_population_set_best_threshold(mfas_population* pop, double threshold);

/* loss_mode 1: per-class positive weights of WeightedCrossEntropyWithLogits (HOST float[C]; default all 1). */
int mfas_population_set_pos_weight(mfas_population* pop, const float* pos_weight);

#ifdef __cplusplus
}
#endif
#endif /* MFAS_HIP_H */
