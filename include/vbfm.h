/* include/vbfm.h -- C-ABI of libvbfm.so, the MI355X-native VB factorization-machine learner.
 *
 * Drop-in boundary for the reference's learner seam: the abstract `fm_learn`
 * (src/libfm/src/fm_learn.h:38-265) as specialised by `fm_learn_vb` /
 * `fm_learn_vb_simultaneous` (src/libfm/src/fm_learn_vb.h:25-793,
 * src/libfm/src/fm_learn_vb_simultaneous.h:15-309) and selected by `-method vb` in
 * src/libfm/libfm.cpp:306-311. The reference has no FFI; the entry points below are what
 * a host (the libFM-compatible CLI in host/, or any C/ctypes caller) binds in place of
 * `new fm_learn_vb_simultaneous()` + `init()` + `learn(train, test)`.
 *
 * Conventions
 *  - plain C types only; every array is caller-owned host memory unless a name says
 *    `_device`; the library copies what it needs and never keeps a caller pointer.
 *  - every function returns 0 on success, nonzero on failure; the message is then in
 *    vbfm_last_error(ctx) (or vbfm_last_error(NULL) for failures without a context).
 *    The reference signals errors by throwing `const char*` / `std::string`, which main()
 *    prints as "ERROR: <msg>" (src/libfm/libfm.cpp:521-525); a host maps a nonzero return
 *    to exactly that.
 *  - one host thread per context; calls are synchronous (they return after the device
 *    work they enqueue has completed), like the reference's single-threaded learner.
 *  - arithmetic is IEEE fp64 for all state, fp32 for design-matrix values and targets
 *    (FM_FLOAT, src/fm_core/fm_data.h:25), uint32 row / feature ids.
 */
#ifndef VBFM_H_
#define VBFM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: vbfm_synth_generate's model_seed / row_offset, vbfm_synth_multihot, VBFM_LAYOUT_ENTRY,
 *    vbfm_iter_stats::ms_test_predict, checkpoints, vbfm_comm_info, vbfm_device_count and the
 *    per-level step entry points.
 * 3: vbfm_config's placement budget (place_candidates, place_budget_bytes) and vbfm_setup_info.
 * 4: vbfm_exchange_info; RCCL communicators are non-blocking with a deadline (VBFM_COMM_TIMEOUT_S).
 * A binding checks vbfm_abi_version() against the value it was built for and refuses a mismatch
 * (struct sizes and argument lists differ). */
#define VBFM_ABI_VERSION 4

typedef struct vbfm_ctx vbfm_ctx;

/* vbfm_config::task (-task r | c, libfm.cpp:137-143) */
#define VBFM_TASK_REGRESSION 0
#define VBFM_TASK_CLASSIFICATION 1

/* == sparse_entry<float> (src/util/fmatrix.h:36-39): 8 bytes, id then value. In a
 * transposed (column) matrix `id` is the row index. */
typedef struct {
	uint32_t id;
	float value;
} vbfm_entry;

/* A data set as the reference's learner sees it: the transposed copy `data_t` built by
 * Data::create_data_t (src/libfm/src/Data.h:457-509) -- column j lists its rows in
 * ascending order -- plus the targets (Data::target). */
typedef struct {
	uint32_t num_rows;        /* Data::num_cases */
	uint32_t num_feature;     /* data_t->getNumRows(): max feature id + 1 */
	uint64_t nnz;
	const uint64_t *col_ptr;  /* [num_feature + 1] */
	const vbfm_entry *col_ent;/* [nnz] */
	const float *target;      /* [num_rows] */
} vbfm_csc;

/* Learner configuration: the fields main() sets on the model and learner before init()
 * (src/libfm/libfm.cpp:215-274, 306-311, 331-334). */
typedef struct {
	int32_t k0;               /* -dim k0: use bias w0 */
	int32_t k1;               /* -dim k1: use 1-way interactions w */
	int32_t num_factor;       /* -dim k2 */
	uint32_t num_attribute;   /* D = max(train.num_feature, test.num_feature) + 1 (libfm.cpp:215) */
	uint32_t num_attr_groups; /* DataMetaInfo::num_attr_groups (1 without -meta) */
	const uint32_t *attr_group; /* [num_attribute] group of each attribute, or NULL = all 0 */
	float min_target;         /* train.min_target (libfm.cpp:333) */
	float max_target;         /* train.max_target (libfm.cpp:332) */
	int32_t device;           /* HIP device ordinal */
	int32_t task;             /* VBFM_TASK_REGRESSION, or VBFM_TASK_CLASSIFICATION (-task c: binary targets,
	                             probit link) which the MCMC / ALS learner provides; the VB and online VB
	                             entry points refuse a classification context */
	/* Placement search of the level-ordered store's two record buffers (no reference counterpart;
	 * DESIGN.md §5b): the scattered record writes of a level run up to ~20 % faster or slower
	 * depending on where the driver placed the buffers, so at store build (>= 2e6 rows) the library
	 * scores candidate buffers on level 0's pattern and keeps the two fastest. Results do not depend
	 * on it (bit for bit). Zero-initialised fields take the defaults.
	 *   place_candidates:   buffers scored, the store's own two included (0 = default: 64 for a
	 *                       store under 2 GB of records, 16 above; 1 or 2 = no search);
	 *   place_budget_bytes: device memory the search may hold at once on top of the store -- the
	 *                       records' stash, a reference buffer and the fresh candidates (0 = default,
	 *                       VBFM_PLACE_BUDGET_DEFAULT).
	 * The search also never takes more than half of the device memory free when it starts (a quarter
	 * with several ranks); when that leaves room for fewer candidates it scores fewer, or none: it
	 * never fails the store. VBFM_PLACE=0 / VBFM_PLACE_TRIES=n / VBFM_PLACE_BUDGET_GB=x in the
	 * environment override the two fields. vbfm_setup_info reports what the search held and took. */
	int32_t place_candidates;
	uint64_t place_budget_bytes;
} vbfm_config;
/* 96 GiB: 16 candidates at C4 (6.4 GB buffers). Fast regions can first appear past the first
 * ~50 GB of allocations (profiles/r06_placement/README.md, calls 1 and wide_search) */
#define VBFM_PLACE_BUDGET_DEFAULT ((uint64_t)96 << 30)

/* Variational and hyper parameters (fm_learn_vb.h:36-46). Arrays are caller-allocated. */
typedef struct {
	double *mu_w, *sigma_w;         /* [D]   mu_w_dash, sigma_w_dash            */
	double *mu_v, *sigma_v;         /* [k*D] mu_v_dash[f][j], sigma_v_dash[f][j] */
	double *hyp_sigma_w;            /* [G]   sigma_w(g)                          */
	double *hyp_sigma_v;            /* [G*k] sigma_v(g, f), row-major [g][f]     */
	double alpha, sigma_0, mu_0_dash, sigma_0_dash;
} vbfm_params;

/* What one pass of the reference's iteration loop reports
 * (fm_learn_vb_simultaneous.h:86-222, fm_learn_vb.h:646-681). */
typedef struct {
	double rmse, mae;           /* test, on predictions clipped to the train range */
	double train_quirk;         /* the "Train=" value: sqrt(mean(clip(e)^2)) */
	double free_energy;         /* F; valid only if free_energy_valid */
	int32_t free_energy_valid;  /* 0 when update_all returned early on a NaN/inf alpha */
	int32_t num_levels;         /* dependency levels of the train schedule */
	double alpha, sigma_0, mu_0_dash, sigma_0_dash;
	uint32_t nan_mu_w, nan_sigma_w, inf_mu_w;
	uint32_t nan_mu_v, nan_sigma_v, inf_mu_v;
	uint32_t nan_alpha, inf_alpha;
	/* device time of the phases of this iteration (hipEvents on the context stream), ms */
	double ms_w0, ms_w, ms_qcache, ms_v, ms_hyper, ms_test, ms_total;
	/* with vbfm_set_profiling(ctx, 1): summed device time of the individual kernel launches
	 * (an event pair around every launch), and the launch counts */
	double ms_vlevel_kernels, ms_wlevel_kernels, ms_qcache_kernels;
	int32_t n_vlevel_launches, n_wlevel_launches, n_qcache_launches;
	uint64_t nnz_train;         /* nnz of this shard's train data */
	/* device time of the test prediction itself; it runs on a second stream under the
	 * hyper-parameter step (ms_test then covers only what follows it: metrics, train quirk) */
	double ms_test_predict;
} vbfm_iter_stats;

/* ---- lifecycle ---------------------------------------------------------------------- */
int vbfm_create(vbfm_ctx **out, const vbfm_config *cfg);   /* fm_learn_vb::init (fm_learn_vb.h:685-743) */
void vbfm_destroy(vbfm_ctx *ctx);
const char *vbfm_last_error(const vbfm_ctx *ctx);
int vbfm_abi_version(void);
/* HIP devices visible to this process (0 without a GPU). No reference counterpart: the
 * reference is single-threaded on the host; the multi-rank CLI (-devices) maps ranks to
 * ordinals with it. It initialises the HIP runtime: call it only in the process that will
 * use the GPU (never before a fork). */
int vbfm_device_count(int32_t *n);

/* ---- data (DataSubset hand-over, fm_learn_vb::learn, fm_learn_vb.h:746-786) ----------- */
int vbfm_set_train(vbfm_ctx *ctx, const vbfm_csc *train);
int vbfm_set_test(vbfm_ctx *ctx, const vbfm_csc *test);
/* Field-structured synthetic data generated directly in HBM (tests/synth.py defines it):
 * rows x n_fields one-hot fields of ids_per_field ids each. which: 0 = train, 1 = test.
 * seed draws the rows, model_seed the planted model (bias + rank-2 interaction) that the
 * train set, the test set and every rank's shard share; the rows generated are rows
 * [row_offset, row_offset + num_rows) of the one-rank data set (a row shard). */
int vbfm_synth_generate(vbfm_ctx *ctx, int32_t which, uint32_t num_rows, uint32_t n_fields,
                        uint32_t ids_per_field, uint64_t seed, int32_t xmode, uint64_t model_seed,
                        uint64_t row_offset);
/* Multi-hot rows WITHOUT field structure (tests/synth.py generate_multihot defines it): row R
 * holds lo..hi (<= 64) distinct ids out of num_features, one per stratum of the id range, and
 * the same planted model; the levels of such data miss rows, so the sweeps take the
 * column-gather layout. Rows [row_offset, row_offset + num_rows) of the one-rank data set. */
int vbfm_synth_multihot(vbfm_ctx *ctx, int32_t which, uint32_t num_rows, uint32_t num_features, uint32_t lo,
                        uint32_t hi, uint64_t seed, int32_t xmode, uint64_t model_seed, uint64_t row_offset);
/* Binary targets from a device-generated set (no reference counterpart): target = target >=
 * threshold ? +1 : -1 on the device; *positives (may be NULL) receives the number of +1 rows of
 * this rank's set. The set's target range becomes [-1, 1]. Binarizing the train set of an MCMC /
 * ALS context drops its row caches (they hold yhat - the old target): vbfm_mcmc_init_caches follows. */
int vbfm_synth_binarize(vbfm_ctx *ctx, int32_t which, float threshold, uint64_t *positives);
/* Copy back the device copy of a data set (parity of the device transpose / generator). */
int vbfm_get_csc(vbfm_ctx *ctx, int32_t which, uint64_t *col_ptr /*[nf+1]*/, vbfm_entry *col_ent /*[nnz]*/,
                 float *target /*[rows]*/);
int vbfm_get_shape(vbfm_ctx *ctx, int32_t which, uint32_t *num_rows, uint32_t *num_feature, uint64_t *nnz);
/* level of each train feature (1-based; [train.num_feature]) and the number of levels */
int vbfm_get_levels(vbfm_ctx *ctx, uint32_t *level, uint32_t *num_levels);

/* ---- parameters ----------------------------------------------------------------------- */
int vbfm_set_params(vbfm_ctx *ctx, const vbfm_params *p);
int vbfm_get_params(vbfm_ctx *ctx, vbfm_params *p);

/* Bench-scale random init on the device: mu_w_dash, mu_v_dash = 0.1 * N(0,1) from a
 * counter-based generator (splitmix64 + Box-Muller; NOT the reference's glibc stream),
 * sigma_* = .02, hyper parameters and scalars at their fm_learn_vb::init values. */
int vbfm_init_params_device(vbfm_ctx *ctx, uint64_t seed);

/* The reference's initial draws -- exactly what vbfm_init_params_host + vbfm_set_params
 * produce (srand(seed); fm.v, fm.w ~ N(0, init_stdev); mu_w_dash, mu_v_dash = 0.1 N(0,1);
 * glibc rand() with Leva normals) -- generated on the device: the glibc stream split into
 * chunks by jump-ahead, Leva's rejection as a stream compaction. fm_v [k*D] (f-major) and
 * fm_w [D] receive the model draws (v_file.txt) when not NULL. */
int vbfm_init_params_replay(vbfm_ctx *ctx, uint32_t seed, double init_stdev, double *fm_v, double *fm_w);

/* ---- learning (fm_learn_vb_simultaneous::_learn, fm_learn_vb_simultaneous.h:18-259) ---- */
int vbfm_init_caches(vbfm_ctx *ctx);                     /* :37-44 */
int vbfm_iterate(vbfm_ctx *ctx, vbfm_iter_stats *out);   /* one pass of :75-258 */
int vbfm_get_test_pred(vbfm_ctx *ctx, double *pred /*[test rows]*/); /* pred_this (clipped) */

/* ---- the steps of update_all (fm_learn_vb.h:383-501), for step-level parity ---------- */
int vbfm_step_w0(vbfm_ctx *ctx);                  /* update_w0, :504-525 */
int vbfm_step_w(vbfm_ctx *ctx);                   /* the w sweep, :390-406 / :527-574 */
int vbfm_step_qcache(vbfm_ctx *ctx, int32_t f);   /* zero + add_main_q, :411-418 / :354-381 */
int vbfm_step_v(vbfm_ctx *ctx, int32_t f);        /* the v sweep of factor f, :420-438 / :577-644 */
/* One dependency level of a sweep, for localising a parity miss below one
 * sweep: level l (0-based, in order 0..L-1, L from vbfm_get_levels) of the w sweep, or of factor
 * f's v sweep (its q-cache is made current at level 0). After level l the caches and parameters
 * equal the reference's after its update_w / update_v of every feature of levels 0..l, features
 * of a level in ascending id order (fm_learn_vb.h:390-406, 409-440; ref_driver levels). Same
 * kernels as the whole sweep; one rank or the two-pass split (VBFM_DEFER=0), not the deferred
 * split or feature shards. vbfm_get_rows / vbfm_get_params read the state between two levels;
 * other steps are refused until the sweep's last level has run. */
int vbfm_step_w_level(vbfm_ctx *ctx, int32_t level);
int vbfm_step_v_level(vbfm_ctx *ctx, int32_t f, int32_t level);
int vbfm_step_hyper(vbfm_ctx *ctx, int32_t *early_return); /* :446-498 */
int vbfm_free_energy(vbfm_ctx *ctx, double *F);   /* :646-681 (value only, no file) */
/* row caches: e (cache[].e), t/q/z of cache_t, q of cache (the factor q-cache) */
int vbfm_get_rows(vbfm_ctx *ctx, double *e, double *t, double *q, double *tq, double *tz);
int vbfm_get_test_e(vbfm_ctx *ctx, double *e /*[test rows]*/);

/* Layout of the row caches in HBM during the sweeps (no reference counterpart: the
 * reference keeps cache[] / cache_t[] in row order, fm_learn_vb.h:17-21,746-786).
 *   VBFM_LAYOUT_AUTO   (default) level-ordered when every dependency level holds each train
 *                      row exactly once (field-structured one-hot data), else column-gather;
 *   VBFM_LAYOUT_COLUMN row order, columns gather their rows;
 *   VBFM_LAYOUT_LEVEL  records kept in the current level's column order and streamed
 *                      (vbfm_set_layout fails at the first sweep when the data does not
 *                      allow it). Results are identical up to the summation order of the
 *                      data-set sums (w0, alpha, free energy).
 *   VBFM_LAYOUT_ENTRY  for levels that miss rows (multi-hot rows without fields): one slot per
 *                      train entry in the level order, a row's record in the slot of the entry
 *                      its next level sweeps; levels stream their runs and move each record to
 *                      its row's next slot (nnz x 64 B of HBM; one rank). AUTO picks it
 *                      where LEVEL does not apply and it fits (VBFM_ESTORE=0: COLUMN instead).
 * Set before vbfm_set_train; VBFM_LAYOUT=auto|column|level|entry in the environment overrides.
 * vbfm_get_layout reports the layout in use (COLUMN, LEVEL or ENTRY) once the train set is known. */
#define VBFM_LAYOUT_AUTO 0
#define VBFM_LAYOUT_COLUMN 1
#define VBFM_LAYOUT_LEVEL 2
#define VBFM_LAYOUT_ENTRY 3
int vbfm_set_layout(vbfm_ctx *ctx, int32_t layout);
int vbfm_get_layout(vbfm_ctx *ctx, int32_t *layout);

/* per-launch event timing of the sweep kernels inside vbfm_iterate (off by default) */
int vbfm_set_profiling(vbfm_ctx *ctx, int32_t on);   /* on > 1: time every on-th launch of a kind */

/* ---- checkpoint / resume ----------------------------------------------------------------
 * No reference counterpart: the reference always starts from its initial draws
 * (num_complete_iter = 0, fm_learn_vb_simultaneous.h:20) and keeps no state on disk. The VB
 * learner's state between two vbfm_iterate calls -- {mu, sigma} of w and v, the hyper
 * parameters, alpha, sigma_0, mu_0_dash, sigma_0_dash and this rank's train row caches -- goes
 * to one file. vbfm_load_state, on a context created with the same configuration, rank and
 * train data (checked: shape and a fingerprint of the train CSC and targets; the test set is
 * free), replaces vbfm_init_caches and the run continues bit for bit. iter: the caller's
 * iteration count, stored and returned. An MCMC / ALS context (vbfm_mcmc_init) writes its
 * chain instead -- the RNG (mode, seed, completed iterations, the reference stream's position),
 * the parameters, hyper-priors, w0, alpha, the test predictions and their running sum, the
 * train row caches -- and vbfm_load_state on a context initialised the same way (vbfm_mcmc_init
 * with the same method and RNG mode; it replaces vbfm_mcmc_init_caches) continues the chain bit
 * for bit. An online context (vbfm_online_init with the same -batch) saves between epochs:
 * parameters, natural parameters, step sizes, the rand() stream and the last permutation. */
int vbfm_save_state(vbfm_ctx *ctx, const char *path, uint32_t iter);
int vbfm_load_state(vbfm_ctx *ctx, const char *path, uint32_t *iter);

/* ---- the factor sweep alone (the metric's timed unit: q-cache + v sweep, all factors) -- */
int vbfm_factor_sweep(vbfm_ctx *ctx, double *ms_device);

/* ---- multi-GPU: row-sharded exact mode over RCCL ----------------------------------------
 * Each rank owns a slice of the train rows; per dependency level the per-feature
 * sufficient statistics are all-reduced, so every rank computes identical posteriors. */
int vbfm_comm_unique_id(uint8_t out[128]);
int vbfm_comm_init(vbfm_ctx *ctx, int32_t nranks, int32_t rank, const uint8_t uid[128]);

/* The same row- / feature-sharded modes with a caller-supplied exchange instead of RCCL:
 * every all-reduce of the path stages its buffer in host memory and calls
 * fn(user, buf, count, dtype, op), which must all-reduce buf in place across the ranks and
 * return 0 (non-zero: the call fails with "host exchange failed"). dtype: VBFM_X_F64 /
 * VBFM_X_U32 / VBFM_X_U8; op: VBFM_X_SUM / VBFM_X_MAX. Test transport (e.g. a gloo
 * all-reduce from Python): it lets several ranks share one GPU, which RCCL refuses, so the
 * multi-rank kernels run on a one-GPU box exactly as over RCCL, minus the collective itself. */
#define VBFM_X_F64 0
#define VBFM_X_U32 1
#define VBFM_X_U8 2
#define VBFM_X_SUM 0
#define VBFM_X_MAX 1
typedef int (*vbfm_exchange_fn)(void *user, void *buf, uint64_t count, int32_t dtype, int32_t op);
int vbfm_comm_init_host(vbfm_ctx *ctx, int32_t nranks, int32_t rank, vbfm_exchange_fn fn, void *user);
/* The communicator as RCCL reports it (ncclCommCount / ncclCommUserRank): transport 0 = none
 * (one rank), 1 = RCCL, 2 = host exchange (nranks / rank as given to vbfm_comm_init_host). */
int vbfm_comm_info(vbfm_ctx *ctx, int32_t *nranks, int32_t *rank, int32_t *transport);
/* Failure handling of the exchange (no reference counterpart: the reference is one process).
 * vbfm_comm_init creates a non-blocking RCCL communicator (ncclCommInitRankConfig, blocking = 0).
 * Wherever the library waits for work that holds a collective -- the communicator's set-up, an
 * RCCL call that returns ncclInProgress, a stream synchronisation after an all-reduce -- it polls
 * ncclCommGetAsyncError and a deadline of VBFM_COMM_TIMEOUT_S seconds (default 300) instead of
 * blocking. On an RCCL error or a missed deadline it aborts the communicator (ncclCommAbort) and
 * the call fails; vbfm_last_error names the rank, the phase, factor and level of the exchange and
 * the cause, and every later call that exchanges fails with the same message. A host exchange
 * (vbfm_comm_init_host) fails when the caller's function returns non-zero; its transport owns the
 * timeout. VBFM_COMM_BLOCKING=1 creates a blocking communicator instead (no deadline). */
/* The exchanges of the last vbfm_iterate / vbfm_mcmc_iterate (since vbfm_comm_init before the
 * first): every all-reduce of the path counted with its payload, and its time -- RCCL: an event
 * pair on the stream that runs it around every all-reduce vbfm_set_profiling's stride samples
 * (device time from the call's enqueue to its completion: the wait for the slowest rank
 * included), scaled to all calls; host exchange: the host wall time of every call (copies
 * included). Zero without a communicator. */
typedef struct {
	int32_t transport;        /* as vbfm_comm_info */
	int32_t n_timed;          /* all-reduces timed */
	uint64_t n_calls;         /* all-reduces issued */
	uint64_t bytes;           /* their payload per rank */
	double ms_timed;          /* summed time of the timed ones */
	double ms_estimated;      /* ms_timed / n_timed * n_calls (host exchange: = ms_timed) */
	double timeout_s;         /* the deadline in force (0: blocking communicator or none) */
} vbfm_exchange_stats;
int vbfm_exchange_info(vbfm_ctx *ctx, vbfm_exchange_stats *out);
/* The level store's record-buffer placement (VBFM_PLACE): the score (ms, level 0's pattern to and
 * from a reference buffer) of each candidate record buffer, [0] and [1] being the pair allocated
 * first, and in kept[0], kept[1] the indices of the two buffers kept (records, alternate).
 * *count = 0 when no placement was tuned. ms holds up to *count on entry (in: capacity). */
int vbfm_placement_info(vbfm_ctx *ctx, float *ms, int32_t *count, int32_t *kept);
/* What setting up the train set cost (no reference counterpart; the reference's load and
 * create_data_t are the host's, Data.h:106-283, 457-509): host wall seconds of the last
 * vbfm_set_train (copy to the device + the device CSR build) and of the first sweep's set-up of that
 * train set -- the dependency levels, the row store (level / entry store, long-column segments,
 * split-form payloads) and, inside it, the placement search with the device memory it held at its
 * peak and the candidates it scored (0: no search). Zero until the step has run. */
typedef struct {
	double s_set_train;       /* vbfm_set_train / vbfm_synth_generate of the train set */
	double s_schedule;        /* dependency levels */
	double s_store;           /* row store build, the placement search included */
	double s_placement;       /* ... of which the placement search */
	uint64_t place_bytes;     /* device memory the search held at its peak */
	int32_t place_candidates; /* buffers scored (0: no search) */
	int32_t place_kept[2];    /* the two kept, as vbfm_placement_info's kept */
} vbfm_setup_stats;
int vbfm_setup_info(vbfm_ctx *ctx, vbfm_setup_stats *out);

/* Partition of the VB sweep over ranks (set before vbfm_set_train).
 *   VBFM_SHARD_ROWS (default): the exact row-sharded mode above.
 *   VBFM_SHARD_FEATURES: the north star's feature-column partition. Every rank holds ALL train
 *     rows; the columns of every dependency level are split into num_shards contiguous chunks
 *     and each rank sweeps its chunk; after the w sweep and after every factor pass the ranks'
 *     changes of the e / t row caches, their partial q-caches of the next factor and their
 *     updated parameters are summed with one ncclAllReduce each. Shards do not see each
 *     other's updates within a pass (Jacobi across shards), so results differ from the
 *     reference's sequential sweep when num_shards > 1 (exact for num_shards = 1). Without a
 *     communicator num_shards > 1 runs the shards one after another in this process (same
 *     arithmetic; for tests). num_shards = 0: one shard per rank. VB learner only. */
#define VBFM_SHARD_ROWS 0
#define VBFM_SHARD_FEATURES 1
int vbfm_set_shard_mode(vbfm_ctx *ctx, int32_t mode, int32_t num_shards);

/* ---- online VB learner (-method vb_online, OVBFM) -------------------------------------
 * Replaces fm_learn_vb_online + fm_learn_vb_online_simultaneous (src/libfm/src/
 * fm_learn_vb_online.h, fm_learn_vb_online_simultaneous.h:20-290; selected at
 * src/libfm/libfm.cpp:312-320). vbfm_online_init turns a context made by vbfm_create that holds
 * its train and test sets into the online learner: the VB learner's initial draws (host or
 * device replay, the same values), then fm_learn_vb_online::init (natural parameters, step
 * sizes, col_count). Each vbfm_online_epoch is one iteration of _learn's loop: a
 * std::random_shuffle of the rows on the reference's rand() stream, num_batch mini-batches
 * (row r in batch ceil(shuffle[r] / ceil(N / num_batch))), update_all on each batch in turn,
 * then the test RMSE. num_attribute follows the online CLI: largest feature id of train and
 * test + 1 (find_max_feature, libfm.cpp:167-170, 528-600). One GPU. A num_batch that leaves a
 * batch empty is refused (the reference divides by its zero size). */
#define VBFM_ONLINE_INIT_HOST 0    /* draws on the host (glibc restatement) */
#define VBFM_ONLINE_INIT_REPLAY 1  /* the same draws on the device (vbfm_init_params_replay) */
typedef struct {
	uint32_t num_batch;       /* -batch (libfm.cpp:320; default 50) */
	uint32_t seed;            /* srand(seed) (libfm.cpp:123-124) */
	double init_stdev;        /* -init_stdev (draws of fm.v / fm.w that precede the learner's) */
	int32_t init_mode;        /* VBFM_ONLINE_INIT_* */
	double *fm_v;             /* [k*D] f-major or NULL: receives the fm.v draws (v_file.txt, fm_model.h:98) */
} vbfm_online_config;

typedef struct {
	double rmse, mae;                              /* test, clipped (:206-245) */
	double free_energy_first, free_energy_last;    /* "free energy" of batch 1 and batch num_batch (:143-146) */
	double alpha, sigma_0, mu_0_dash, sigma_0_dash;
	uint32_t nan_mu_w, nan_sigma_w, inf_mu_w;
	uint32_t nan_mu_v, nan_sigma_v, inf_mu_v;
	uint32_t nan_alpha, inf_alpha;
	uint32_t num_batch;
	int32_t num_levels;
	/* device time: regrouping into batches, the batches' update_all, test; ms */
	double ms_regroup, ms_batches, ms_test, ms_total;
	/* ... and the batches' phases summed over the epoch: batch CSR + predictions, update_w0,
	 * the w sweep, the factor sweeps, the hyper-parameters + free energy */
	double ms_predict, ms_w0, ms_w, ms_v, ms_hyper;
	uint32_t n_vlevel_launches;   /* level launches of the factor sweeps */
	uint64_t nnz_train;
	uint32_t n_lord_batches;      /* batches swept on their level-ordered store (complete levels) */
	uint32_t n_pad_batches;       /* ... of which with the padded layout of levels >= 1 (fills the
	                               * struct's tail padding: its size is unchanged) */
} vbfm_online_stats;

int vbfm_online_init(vbfm_ctx *ctx, const vbfm_online_config *cfg);
int vbfm_online_epoch(vbfm_ctx *ctx, vbfm_online_stats *out);
/* the learner's own state: natural parameters ([D], [k*D] f-major as vbfm_params), step sizes
 * new_wj / new_vj [D], scalars {alpha, sigma_0, mu_0_dash, sigma_0_dash, natural_mu_0_dash,
 * natural_sigma_0_dash, new_w0, t_w0}; NULL arrays are skipped. vbfm_get_params and
 * vbfm_get_test_pred serve the online learner as the VB one. */
int vbfm_online_get_state(vbfm_ctx *ctx, double *nat_mu_w, double *nat_sigma_w, double *nat_mu_v,
                          double *nat_sigma_v, double *new_wj, double *new_vj, double scalars[8]);

/* ---- MCMC / ALS learner (-method mcmc | als) -------------------------------------------
 * Replaces fm_learn_mcmc / fm_learn_mcmc_simultaneous (src/libfm/src/fm_learn_mcmc.h,
 * src/libfm/src/fm_learn_mcmc_simultaneous.h), regression and binary classification, without
 * relation blocks.
 * vbfm_mcmc_init turns a context made by vbfm_create into an MCMC/ALS learner; the data
 * hand-over (vbfm_set_train / vbfm_set_test / vbfm_synth_generate), vbfm_comm_init and the
 * level schedule are the VB learner's. State is the model's point values fm.w0 / fm.w /
 * fm.v and the hyper-priors; the row cache holds e = yhat - y (the MCMC sign, :76-80). */
#define VBFM_RNG_REFERENCE 0  /* every draw from the reference's stream: srand(seed), glibc
                                 rand(), Leva normals, Marsaglia-Tsang gammas (random.h),
                                 consumed in the reference's order: the draws the reference
                                 makes on the same inputs */
#define VBFM_RNG_DEVICE 1     /* hyper-prior draws from that stream; the per-attribute
                                 normals of draw_w / draw_v from a counter-based generator
                                 keyed (seed, iteration, factor, attribute), identical on
                                 every shard; fm.w / fm.v initialised on the device.
                                 normal(seed, stream, j) is Box-Muller on the 53-bit uniforms
                                 of splitmix64(seed * K1 + stream * K2 + 2j) and (+ 1). Stream
                                 ids: a sweep's is iteration * (k + 1) + (0 for w, f + 1 for
                                 v_f); bits 63 and 62 are reserved -- bit 63 | iteration keys
                                 the row draws of task c, bit 62 | 21 initialises fm.v (v_f[j]
                                 takes j * k + f) and bit 62 | 22 fm.w -- so no two share a
                                 stream */

typedef struct {
	int32_t do_sample;        /* fm_learn_mcmc::do_sample: 1 mcmc, 0 als (libfm.cpp:131-135, 303) */
	int32_t do_multilevel;    /* fm_learn_mcmc::do_multilevel (libfm.cpp:304) */
	int32_t rng;              /* VBFM_RNG_* */
	uint32_t seed;            /* srand(seed) (libfm.cpp:123-124) */
	double init_stdev;        /* -init_stdev: fm.v, fm.w ~ N(0, init_stdev) (fm_model.h:97, libfm.cpp:298) */
	const double *regular;    /* -regular values: 0, 1, 3 or 1 + 2*num_attr_groups of them (libfm.cpp:367-411) */
	int32_t num_regular;
} vbfm_mcmc_config;

typedef struct {
	double *w;                /* [D]   fm.w */
	double *v;                /* [k*D] fm.v[f][j] */
	double *w_mu, *w_lambda;  /* [G]   fm_learn_mcmc::w_mu, w_lambda */
	double *v_mu, *v_lambda;  /* [G*k] v_mu(g, f), v_lambda(g, f), row-major [g][f] */
	double w0, alpha, reg0;   /* fm.w0, fm_learn_mcmc::alpha, fm.reg0 */
} vbfm_mcmc_params;

typedef struct {
	double rmse_all, mae_all;   /* test, on the running mean of the clipped predictions: "Test=" */
	double rmse_this, mae_this; /* test, this iteration's predictions */
	double train_rmse;          /* "Train=" (fm_learn_mcmc_simultaneous.h:153-162) */
	double alpha, w0;
	uint32_t nan_alpha, inf_alpha, nan_w0, inf_w0, nan_w, inf_w, nan_v, inf_v;
	uint32_t nan_w_mu, inf_w_mu, nan_w_lambda, inf_w_lambda, nan_v_mu, inf_v_mu, nan_v_lambda, inf_v_lambda;
	uint32_t rng_skipped;       /* VBFM_RNG_REFERENCE: attributes whose draw / no-draw decision
	                               (the reference draws no normal for a zero or non-finite
	                               variance) differed from the host's, i.e. 0 while the stream
	                               is the reference's; VBFM_RNG_DEVICE: such attributes */
	int32_t num_levels;
	/* device time of the phases (hipEvents), ms; per-launch sums with vbfm_set_profiling */
	double ms_hyper, ms_w, ms_v, ms_predict, ms_total;
	double ms_vlevel_kernels;
	int32_t n_vlevel_launches;
	uint64_t nnz_train;
} vbfm_mcmc_stats;

int vbfm_mcmc_init(vbfm_ctx *ctx, const vbfm_mcmc_config *cfg);  /* fm_learn_mcmc::init (fm_learn_mcmc.h:1092-1151),
                                                                    parameter draws and -regular (libfm.cpp:123-124, 273-304, 367-411) */
int vbfm_mcmc_set_params(vbfm_ctx *ctx, const vbfm_mcmc_params *p);
int vbfm_mcmc_get_params(vbfm_ctx *ctx, vbfm_mcmc_params *p);      /* NULL arrays are skipped */
int vbfm_mcmc_init_caches(vbfm_ctx *ctx);                          /* _learn prologue, fm_learn_mcmc_simultaneous.h:64-81 */
int vbfm_mcmc_iterate(vbfm_ctx *ctx, vbfm_mcmc_stats *out);        /* one pass of :83-304: draw_all, re-predict, evaluate */
/* fm_learn_mcmc::predict (fm_learn_mcmc.h:355-381): sampling -> pred_sum_all / num_iter,
 * else the last iteration's predictions; clipped to the train target range */
int vbfm_mcmc_get_test_pred(vbfm_ctx *ctx, int32_t num_iter, double *pred /*[test rows]*/);
/* Binary classification (vbfm_config::task = VBFM_TASK_CLASSIFICATION; the augmented probit
 * sampler of fm_learn_mcmc_simultaneous.h:82-89, 176-221, 262-301). Targets are < 0 or >= 0. The
 * sweeps are regression's on a latent target: after every re-prediction each train row's e becomes
 * yhat - s, s from N(yhat, 1) truncated to the target's side of 0 -- its expectation (als), a draw
 * from the reference's stream row by row after draw_all's draws (mcmc, VBFM_RNG_REFERENCE; one rank
 * only) or a draw of the counter-based generator keyed (seed, iteration, global row, attempt)
 * (mcmc, VBFM_RNG_DEVICE; row shards must be contiguous in rank order). Test predictions are
 * Phi(yhat) with the reference's polynomial erf (random.h:47-69). vbfm_mcmc_stats then holds 0 in
 * train_rmse, rmse_* and mae_*; vbfm_mcmc_class_info returns the last iteration's figures
 * (_evaluate_class, :383-401: accuracy, and the mean log10-likelihood with p clamped to
 * [0.01, 0.99]; ll_all, which the reference leaves uninitialised, is computed on the running mean).
 * MAP@5 of the reference's "#Iter=" line is not reproduced (it reads a fixed side file).
 * vbfm_mcmc_get_test_pred clips to [0, 1]. */
typedef struct {
	double acc_train;           /* "Train=": correct train rows / rows, on this iteration's yhat */
	double acc_this, acc_all;   /* test: this iteration's Phi(yhat); the running mean ("Test=") */
	double ll_this, ll_all;
	uint64_t n_train_correct, n_test_correct_this, n_test_correct_all;   /* the counts, over all ranks */
	uint32_t nonfinite_rows;    /* train rows whose yhat was NaN or +-inf (their e is NaN) */
	uint32_t capped_rows;       /* VBFM_RNG_DEVICE: rows whose 64 rejection attempts all failed (p <= 2^-64
	                               each) and that took the truncated expectation */
} vbfm_mcmc_class_stats;
int vbfm_mcmc_class_info(vbfm_ctx *ctx, vbfm_mcmc_class_stats *out);   /* fails on a regression context */
/* the v draws of all factors alone (q-cache + draw_v sweeps, :501-621), for the bench */
int vbfm_mcmc_factor_sweep(vbfm_ctx *ctx, double *ms_device);

/* ---- host side of the reference's CLI path (loader, RNG init) -------------------------- */
typedef struct {
	uint32_t num_rows, num_feature;
	uint64_t nnz;
	float min_target, max_target;
	float *target;                  /* [num_rows] */
	uint64_t *row_ptr; vbfm_entry *row_ent;   /* CSR in file order   (Data.h:233-278) */
	uint64_t *col_ptr; vbfm_entry *col_ent;   /* transposed copy     (Data.h:457-509) */
} vbfm_host_data;
/* Data::load (Data.h:106-283): libfm text, or the binary triple <name>.x/.xt/.y
 * (fmatrix.h:46-52, matrix.h:296-312) when those files exist. Text is parsed in parallel
 * (VBFM_LOADER_THREADS, default min(cores, 16)) with the reference's sscanf semantics; the
 * transpose (Data::create_data_t) is a parallel stable counting sort. */
int vbfm_load_data(const char *filename, vbfm_host_data *out);
/* The reference's binary triple of a loaded data set: <base>.x (CSR rows in file order),
 * <base>.xt (the transposed copy) and <base>.y, as tools/convert + tools/transpose write them
 * (fmatrix.h:67-86, matrix.h:280-293). vbfm_load_data(<base>) then reads it back. */
int vbfm_save_data(const char *basename, const vbfm_host_data *d);
void vbfm_free_host_data(vbfm_host_data *d);
/* srand(seed) then the reference's draw order: fm.v (k*D) ~ N(0, init_stdev)
 * (fm_model.h:97), fm.w (D) (libfm.cpp:307), mu_w_dash (D), mu_v_dash (k*D) as 0.1*N(0,1)
 * (fm_learn_vb.h:709-711); sigma_* and hyper parameters at their init values.
 * fm_v / fm_w may be NULL (they are drawn either way, to keep the stream aligned). */
int vbfm_init_params_host(uint32_t seed, double init_stdev, int32_t num_factor, uint32_t num_attribute,
                          uint32_t num_attr_groups, vbfm_params *out, double *fm_v, double *fm_w);

/* ---- model files and scoring (additive to ABI 4: new functions and structs only) --------
 * No reference counterpart: the reference predicts only the test set attached while training
 * (libfm.cpp:514-519) and keeps no model on disk. A model file holds the parameters a prediction
 * reads and nothing else -- no row caches, no hyper-parameters, no attribute groups, no data
 * fingerprint -- so it loads without the train set (a checkpoint, vbfm_save_state, does not).
 * Little-endian: an 88-byte header (magic "VBFMMD01", format version, kind, k0, k1, num_factor,
 * num_attribute, min_target, max_target, the caller's iteration count, the scalars, the payload's
 * byte count and a 64-bit checksum of the payload), then the payload as the library stores it:
 * VB kinds {mu, sigma} pairs of w [D] and of v [j*k + f]; ALS / MCMC w [D] and v [j*k + f].
 * Written to <path>.tmp, fsync'ed and renamed. A reader checks magic, version, kind, that
 * D * k * entry size does not overflow, that the header's sizes equal the file's size exactly and
 * the checksum, all before any allocation that grows with the file. */
#define VBFM_MODEL_VB 0
#define VBFM_MODEL_VB_ONLINE 1
#define VBFM_MODEL_ALS 2
#define VBFM_MODEL_MCMC_DRAW 3   /* ONE draw of the chain (fm.w0 / fm.w / fm.v as they are when the model is taken:
                                    the last draw after the last iteration), not the chain average the MCMC
                                    learner's -out reports: that is VBFM_MODEL_MCMC_CHAIN ("chains of draws" below) */
#define VBFM_MODEL_MCMC_CHAIN 4  /* S draws of the chain in one model: scored as their average, with the spread */
typedef struct {
	int32_t kind, k0, k1, num_factor;
	uint32_t num_attribute;
	float min_target, max_target;
	uint32_t iter;
	int32_t has_variance;     /* 1 for the VB kinds (the file holds sigma: T_n can be scored) */
	double w0_or_mu0;         /* VB kinds: mu_0_dash; ALS / MCMC: w0 */
	double sigma_0_dash;      /* VB kinds; 0 otherwise */
	double alpha;
} vbfm_model_info;
/* Host-only (no GPU needed; failures in vbfm_last_error(NULL)). vbfm_model_file_info validates the
 * whole file. The writer takes vb (VB kinds: mu_w, sigma_w, mu_v, sigma_v) or mc (ALS / MCMC: w, v);
 * the reader fills caller-allocated arrays of whichever struct matches the file's kind, NULL
 * pointers and NULL arrays skipped. vbfm_params / vbfm_mcmc_params hold v as [f][j], the file as
 * [j][f]: both convert. has_variance, and the scalars of the kind's struct, come from info. */
int vbfm_model_file_info(const char *path, vbfm_model_info *out);
int vbfm_model_write_host(const char *path, const vbfm_model_info *info, const vbfm_params *vb,
                          const vbfm_mcmc_params *mc);
int vbfm_model_read_host(const char *path, vbfm_model_info *info, vbfm_params *vb, vbfm_mcmc_params *mc);
/* The task of a model (VBFM_TASK_*). vbfm_model_info cannot grow, so the task travels beside it: in
 * the file it is the header word that was reserved (0 = regression: every earlier file reads as
 * before). The earlier reader ignored that word, so a classification model is written with format
 * version 3, which an earlier library refuses (2 was never written and stays refused); regression
 * files keep version 1 byte for byte.
 * vbfm_model_write_host writes a regression model; only the ALS / MCMC kinds take task c. */
int vbfm_model_file_task(const char *path, int32_t *task);   /* host-only; validates the whole file */
int vbfm_model_write_host_task(const char *path, const vbfm_model_info *info, const vbfm_params *vb,
                               const vbfm_mcmc_params *mc, int32_t task);
/* A chain file (VBFM_MODEL_MCMC_CHAIN, either task) holds S >= 1 draws. vbfm_model_info cannot grow, so
 * the draw count travels beside it, as the task does: in the file it is an 8-byte extension of the
 * header (draw count, a reserved word), and the file has format version 4, which an earlier library
 * refuses rather than reading it as one draw; every file of the other kinds stays byte for byte what
 * it was. In the info of a chain w0_or_mu0 and alpha are the LAST draw's, has_variance is 0 (the file
 * holds no sigma; the spread across draws is scored, see vbfm_score). Payload, as the library stores
 * it: the S {w0, alpha} pairs in draw order, then cw [j*S + s], then cv [(j*S + s)*k + f] (feature-
 * major, the draws of one feature adjacent). The reader checks magic, version, kind, S >= 1, that
 * the reserved word is 0, that
 * S * D * (k + 1) * 8 does not overflow 64 bits, that the sizes equal the file's size exactly and the
 * checksum before any allocation that grows with the header. vbfm_model_file_info and
 * vbfm_model_file_task accept a chain file; vbfm_model_read_host refuses it and names
 * vbfm_model_read_host_draw; vbfm_model_write_host(_task) refuses the kind. */
int vbfm_model_file_draws(const char *path, uint32_t *draws);   /* host-only; validates the whole file; 1 for every other kind */
/* draws[s], s = 0 .. S-1 in chain order: w [D], v [k*D] as [f][j], w0, alpha (the other fields are not read) */
int vbfm_model_write_host_chain(const char *path, const vbfm_model_info *info, int32_t task, uint32_t S,
                                const vbfm_mcmc_params *draws /*[S]*/);
/* draw s of a chain file into mc (NULL arrays skipped; v as [f][j]; w0 and alpha are the draw's); s >= S
 * and a file of another kind are refused */
int vbfm_model_read_host_draw(const char *path, uint32_t s, vbfm_model_info *info, vbfm_mcmc_params *mc);

/* A model on a device: the tables the scoring kernels read. Failures of a call that has a model
 * are in vbfm_model_last_error(m), those without in vbfm_last_error(NULL). */
typedef struct vbfm_model vbfm_model;
/* the context's parameters as they are now (VB, online VB, MCMC / ALS context); with several ranks
 * only rank 0 writes (the parameters are replicated), the others return 0 */
int vbfm_model_save(vbfm_ctx *ctx, const char *path, uint32_t iter);
int vbfm_model_from_ctx(vbfm_model **out, vbfm_ctx *ctx);   /* device-to-device snapshot on ctx's device */
int vbfm_model_load(vbfm_model **out, const char *path, int32_t device);
int vbfm_model_info_get(const vbfm_model *m, vbfm_model_info *out);
int vbfm_model_task(const vbfm_model *m, int32_t *task);
int vbfm_model_num_draws(const vbfm_model *m, uint32_t *draws);   /* S of a chain model, 1 for every other kind */
/* w0 and alpha of draw s (s < vbfm_model_num_draws; NULL pointers skipped); a model of another kind: s = 0,
 * the info's w0_or_mu0 and alpha */
int vbfm_model_draw_scalars(const vbfm_model *m, uint32_t s, double *w0, double *alpha);
const char *vbfm_model_last_error(const vbfm_model *m);
void vbfm_model_destroy(vbfm_model *m);

/* rows to score, CSR in host memory: row r's entries are row_ent[row_ptr[r] .. row_ptr[r + 1]),
 * in any order: a row's terms are summed in ascending id (entries of one id in the order given),
 * the order of the reference's transposed copy (Data.h:457-509) and of a context's predictions */
typedef struct {
	uint32_t num_rows;
	uint64_t nnz;
	const uint64_t *row_ptr;    /* [num_rows + 1] */
	const vbfm_entry *row_ent;  /* [nnz] */
} vbfm_csr;
#define VBFM_ORDER_AUTO 0    /* the context's rule: exact while nnz * k <= 5e7, else group */
#define VBFM_ORDER_EXACT 1   /* the reference's summation order (factor-major, entries ascending) */
#define VBFM_ORDER_GROUP 2   /* the lane-group kernel: per-factor sums in entry order, the factors
                                summed by a fixed butterfly (bit-identical to the wave kernels) */
typedef struct {
	int32_t order;         /* VBFM_ORDER_* */
	int32_t clip;          /* 1: mean clipped to [min_target, max_target] as pred_this is; a model of task c:
	                          1 = the probability Phi(yhat) as pred_this is, 0 = the raw yhat */
	int32_t unknown_ids;   /* ids >= num_attribute: 0 refuse (the message names the first such row and its
	                          smallest unknown id), 1 skip the entry */
	uint64_t chunk_bytes;  /* device memory per staged chunk of host rows, 0 = default (VBFM_SCORE_CHUNK_DEFAULT) */
} vbfm_score_opts;
#define VBFM_SCORE_CHUNK_DEFAULT ((uint64_t)64 << 20)
typedef struct {
	uint32_t n_chunks;
	uint64_t skipped_entries;
	double ms_copy, ms_kernel;   /* device time of the chunks' copies to the device / of their kernels, summed */
	double ms_total;             /* host wall time of the call */
} vbfm_score_stats;
/* mean[r] = predict_data_and_write_to_eterms (fm_learn_vb.h:70-203) of row r on the model's
 * parameters -- for ALS / MCMC kinds on the point values (MCMC_DRAW: that one draw's prediction,
 * not the chain average: a MCMC_CHAIN model scores that, see "chains of draws" below). var (NULL, or
 * [rows]) = the reference's T_n (predict_t_and_write_to_qterms, fm_learn_vb.h:207-312), refused for the
 * ALS and MCMC_DRAW kinds, for a MCMC_CHAIN model the spread across its draws; the predictive variance of
 * y is T_n + 1 / alpha (alpha is in the info; the addition is the caller's). o == NULL: all defaults
 * (auto order, clipped, refuse). vbfm_score never needs the
 * rows in device memory at once: it cuts them into chunks of whole rows of at most chunk_bytes (a
 * larger row is a chunk by itself), staged through two pinned host and two device buffers, chunk
 * i + 1's copy under chunk i's kernel; results are bit-identical whatever the chunk size. */
int vbfm_score(vbfm_model *m, const vbfm_csr *rows, const vbfm_score_opts *o, double *mean, double *var,
               vbfm_score_stats *st);
/* the same for the train (which = 0) or test (1) set a context holds in device memory (synthetic
 * sets included); the context must be on the model's device */
int vbfm_score_device(vbfm_model *m, vbfm_ctx *ctx, int32_t which, const vbfm_score_opts *o, double *mean,
                      double *var, vbfm_score_stats *st);

/* ---- chains of draws (additive to ABI 4: new functions and opaque structs only) -------------------
 * The MCMC learner reports pred_sum_all / num_iter, the mean over its draws of the per-draw predictions
 * (fm_learn_mcmc_simultaneous.h:152-186, 238-245; fm_learn_mcmc.h:355-381); no reference counterpart
 * keeps the draws. A chain collector keeps S draws of a sampling MCMC context in device memory,
 * feature-major with the draws of a feature adjacent (cw [j*S + s], cv [(j*S + s)*k + f], and w0 [s],
 * alpha [s] beside them), and turns them into a model of kind VBFM_MODEL_MCMC_CHAIN or into its file.
 *
 * vbfm_score / vbfm_score_device of a chain model (signatures and options as for every kind). For draw
 * s, in the order added, yhat_s(r) is exactly -- bit for bit: the same expressions, summation order and
 * skip of unknown ids -- what vbfm_score returns with clip = 0 for a MCMC_DRAW model holding draw s under
 * the same order, and
 *     p_s = clip(yhat_s, min_target, max_target)   regression, clip = 1
 *     p_s = Phi(yhat_s)                            task c, clip = 1 (the learner's link)
 *     p_s = yhat_s                                 clip = 0
 *     sum = 0;  for s = 0 .. S-1: sum = sum + p_s;                      mean[r] = sum / S
 *        (clip = 1: then min / max to [min_target, max_target], task c [0, 1], as vbfm_mcmc_get_test_pred)
 *     m = 0; M2 = 0;  for s = 0 .. S-1: d = p_s - m;  m = m + d / (s + 1);  M2 = M2 + d * (p_s - m)
 *                                                                       var[r] = M2 / S
 * both loops in draw order, every operation rounded on its own (no contraction), so a plain float64
 * restatement reproduces mean and var bit for bit from the per-draw scores, whatever the chunk size and
 * the launch geometry. var is 0 for S = 1. With every iteration of a run kept, scoring the attached
 * test rows reproduces vbfm_mcmc_get_test_pred bit for bit. The predictive variance of y in regression
 * is var + mean_s(1 / alpha_s); the addition is the caller's (vbfm_model_draw_scalars has the alphas).
 * vbfm_candidates_create / vbfm_recommend refuse a chain model ("ranking a chain of draws" below has the
 * entry points that take one).
 *
 * vbfm_chain_create: capacity draws of ctx's shape on ctx's device; only a sampling MCMC context
 * (vbfm_mcmc_config::do_sample = 1) is accepted -- ALS is deterministic, a chain of it is one point.
 * The bytes needed, capacity * D * (k + 1) * 8 plus the scalars, are checked against the device's free
 * memory before anything is allocated; the refusal names both figures. vbfm_chain_add copies the
 * context's fm.w0 / fm.w / fm.v and alpha as they are now into the next slot (one kernel on the
 * context's stream); it is refused beyond the capacity and from a context of another (D, k, k0, k1,
 * task). With several ranks the parameters are replicated: every rank may collect, vbfm_chain_save
 * writes on rank 0 only and returns 0 on the others, as vbfm_model_save does; it takes no further
 * device memory that grows with the draws (a full collector is read as it is, a partly filled one
 * through a 64 MiB piece), only host memory for the payload. vbfm_model_from_chain copies the draws
 * collected so far device to device into a model that does not depend on the collector afterwards:
 * a SECOND copy of them, n * D * (k + 1) * 8 bytes more, checked against the free memory before it is
 * allocated and refused with both figures -- a collector of more than half the free memory is saved,
 * destroyed and loaded instead. Failures of a call that has a chain are in vbfm_chain_last_error(ch), those
 * without in vbfm_last_error(NULL). */
typedef struct vbfm_chain vbfm_chain;
int vbfm_chain_create(vbfm_chain **out, vbfm_ctx *ctx, uint32_t capacity);
int vbfm_chain_add(vbfm_chain *ch, vbfm_ctx *ctx);
int vbfm_chain_count(const vbfm_chain *ch, uint32_t *n);
int vbfm_chain_save(vbfm_chain *ch, const char *path, uint32_t iter);
int vbfm_model_from_chain(vbfm_model **out, const vbfm_chain *ch);
void vbfm_chain_destroy(vbfm_chain *ch);
const char *vbfm_chain_last_error(const vbfm_chain *ch);

/* ---- candidate sets and recommendation (additive to ABI 4: new functions and structs only) ----
 * No reference counterpart. The best topn of M candidate rows for each of B context rows, a pair
 * (c, j) valued as the model's mean of ONE row that holds c's entries and j's entries -- without
 * building that row. With base_r the unclipped mean of row r alone (vbfm_score's, clip = 0, lane-group
 * order) and Q_r[f] the per-factor sum of row r (entries in ascending id, as vbfm_score orders them):
 *     dot = 0;  for f = 0 .. k - 1:  dot = fma(Q_c[f], Q_j[f], dot)
 *     raw(c, j) = (base_c + base_j - (k0 ? w0 : 0)) + dot          (w0 = mu_0_dash for the VB kinds)
 * VB kinds use the means, ALS / MCMC the point values (MCMC_DRAW: that draw; a MCMC_CHAIN model is
 * refused). Every pair is
 * computed by exactly this expression and the ranking is a total order -- larger raw first, equal raw
 * by smaller candidate index -- so idx, score and count are bit-identical whatever the chunk size and
 * the launch geometry. A pair whose raw is not finite is never returned (nonfinite_pairs counts them).
 * The returned score is raw; with clip = 1 what vbfm_score would return for the model's task (clipped
 * to the target range; a model of task c: Phi(raw)), applied to the survivors only; the ranking is
 * always on raw. The identity holds for any entries (repeated ids, ids shared by c and j); raw differs
 * from vbfm_score of the merged row by the rounding of a reordered fp64 sum. Variances (T_n) are not
 * ranked. Limits: topn <= VBFM_REC_MAX_TOPN, num_factor <= 256; anything beyond is refused. */
#define VBFM_REC_MAX_TOPN 128
/* The candidates' sums on the model's device, prepared once and reused across vbfm_recommend calls.
 * unknown_ids as vbfm_score_opts. A candidate set belongs to the model handle it was made from
 * (another handle is refused) and must be destroyed before that model: destroying the model first is
 * the caller's error. Failures are in vbfm_model_last_error(m). */
typedef struct vbfm_candidates vbfm_candidates;
int vbfm_candidates_create(vbfm_candidates **out, vbfm_model *m, const vbfm_csr *rows, int32_t unknown_ids);
uint32_t vbfm_candidates_count(const vbfm_candidates *c);
void vbfm_candidates_destroy(vbfm_candidates *c);
typedef struct {
	int32_t topn;          /* 1 .. VBFM_REC_MAX_TOPN */
	int32_t clip;          /* as vbfm_score_opts::clip, on the returned scores only */
	int32_t unknown_ids;   /* of the context rows: 0 refuse, 1 skip the entry */
	uint64_t chunk_bytes;  /* device memory per staged chunk of context rows, 0 = VBFM_SCORE_CHUNK_DEFAULT */
} vbfm_recommend_opts;
typedef struct {
	uint32_t n_chunks;
	uint64_t pairs;             /* B * M */
	uint64_t nonfinite_pairs;   /* pairs whose raw was NaN or +-inf */
	uint64_t excluded_hits;     /* pairs that beat their context's N-th best when met and were on its exclusion
	                               list (the other excluded pairs are never looked up; depends on the geometry) */
	double ms_prepare, ms_pairs, ms_merge;   /* device time of the chunks' row preparation, pair and merge kernels, summed */
	double ms_total;            /* host wall time of the call */
} vbfm_recommend_stats;
/* contexts: host CSR, staged in chunks of whole rows as vbfm_score stages its rows. exclude: excl_ptr
 * NULL, or per context a sorted (ascending) list of candidate indices never to return: context r's
 * are excl_idx[excl_ptr[r] .. excl_ptr[r + 1]); an index >= the candidate count or an unsorted list
 * fails the call, naming the row. Results: idx [B * topn] (-1 beyond count), score [B * topn] (NaN
 * beyond count), count [B]: the entries returned for each context, best first. */
int vbfm_recommend(vbfm_model *m, const vbfm_candidates *c, const vbfm_csr *contexts, const uint64_t *excl_ptr,
                   const uint32_t *excl_idx, const vbfm_recommend_opts *o, int32_t *idx, double *score,
                   uint32_t *count, vbfm_recommend_stats *st);

/* ---- ranking by mean + beta * sd (additive to ABI 4: new functions and structs only) ---------------
 * The same ranking on an upper (beta > 0) or lower (beta < 0) confidence bound of the pair's row, for
 * the kinds with has_variance (VBFM_MODEL_VB, VBFM_MODEL_VB_ONLINE); ALS, MCMC_DRAW and MCMC_CHAIN models
 * are refused with a message that names the kind. The reference's T_n (predict_t_and_write_to_qterms,
 * fm_learn_vb.h:207-312) is, per factor, built from Z[f] = sum sigma_v x^2 and P[f] = sum mu_v^2 x^2 over
 * the row's entries as 1/2 Z^2 + Z P; every other term is a sum over entries. So for one row holding c's
 * and j's entries
 *     T(c u j) = T_c + T_j - [k0] sigma_0_dash + sum_f ( Z_c[f] (Z_j[f] + P_j[f]) + P_c[f] Z_j[f] )
 * for any entries, repeated and shared ids included. Rows are prepared by the lane-group scorer:
 * base_r, Q_r[f] and raw(c, j) are exactly those of vbfm_recommend above; tb_r is the T_n vbfm_score
 * returns for row r alone (group order); Z_r[f], P_r[f] the scorer's per-factor sums of row r (entries in
 * ascending id); U_j[f] = Z_j[f] + P_j[f], rounded once when the candidate set is prepared. Then
 *     t = 0;  for f = 0 .. k - 1:  t = fma(Z_c[f], U_j[f], t);  t = fma(P_c[f], Z_j[f], t)
 *     T(c, j)   = (tb_c + tb_j - (k0 ? sigma_0_dash : 0)) + t
 *     sd(c, j)  = sqrt(max(T(c, j) + (noise ? 1 / alpha : 0), 0))
 *     key(c, j) = fma(beta, sd(c, j), raw(c, j))
 * Every pair's raw, T and key are formed by exactly these expressions, whatever tile, slice or chunk the
 * pair falls in, and the ranking is the total order above applied to key (larger first, equal key by
 * smaller candidate index), so all results are bit-identical whatever the chunk size and the launch
 * geometry. A pair whose raw or T is not finite (or whose key overflows) is never returned and is counted
 * in nonfinite_pairs. beta is any finite double (NaN and +-inf are refused); beta = 0 is vbfm_recommend's
 * ranking. Returned for each survivor, best first: idx; key; score = raw, or with clip = 1 what
 * vbfm_recommend returns for it; var = T(c, j) without the noise term -- as with vbfm_score, adding
 * 1 / alpha is the caller's. T differs from vbfm_score's var of the merged row by the rounding of a
 * reordered fp64 sum. Limits as vbfm_recommend.
 *
 * vbfm_candidates_create_var makes a candidate set that also holds Z, U and tb of its rows: three
 * times the device memory of vbfm_candidates_create's (checked against the free memory before anything
 * is allocated; the refusal names both figures). Such a set is also valid for vbfm_recommend, with the
 * same bits; vbfm_recommend_ucb refuses a set made by vbfm_candidates_create. */
int vbfm_candidates_create_var(vbfm_candidates **out, vbfm_model *m, const vbfm_csr *rows, int32_t unknown_ids);
typedef struct {
	int32_t topn;          /* the four fields of vbfm_recommend_opts */
	int32_t clip;
	int32_t unknown_ids;
	uint64_t chunk_bytes;
	double beta;           /* finite */
	int32_t noise;         /* 1: sd is of y (T + 1 / alpha), 0: of the model's mean (T) */
} vbfm_recommend_ucb_opts;
/* contexts, exclusions, idx and count as vbfm_recommend; key, score, var [B * topn] (NaN beyond count),
 * each may be NULL. st: nonfinite_pairs has the meaning above. */
int vbfm_recommend_ucb(vbfm_model *m, const vbfm_candidates *c, const vbfm_csr *contexts, const uint64_t *excl_ptr,
                       const uint32_t *excl_idx, const vbfm_recommend_ucb_opts *o, int32_t *idx, double *key,
                       double *score, double *var, uint32_t *count, vbfm_recommend_stats *st);

/* ---- ranking a chain of draws (additive to ABI 4: new functions and structs only) -------------------
 * Top-N from a VBFM_MODEL_MCMC_CHAIN model: the pairs ranked on the mean over the S draws of the pair's
 * raw value -- what the MCMC learner reports, before the link -- plus beta times its spread across the
 * draws. Every other entry point above goes on refusing a chain model; these two refuse every other
 * kind (the message names it and points to vbfm_candidates_create / vbfm_recommend). For context row c,
 * candidate row j and draw s = 0 .. S - 1, in the order the draws were added:
 *     dot_s = 0;  for f = 0 .. k - 1:  dot_s = fma(Q_{c,s}[f], Q_{j,s}[f], dot_s)
 *     raw_s = ((base_{c,s} + base_{j,s}) - (k0 ? w0_s : 0)) + dot_s
 * base_{r,s} is the unclipped yhat_s of row r alone as the chain scorer forms it in group order (bit for
 * bit vbfm_score(clip = 0, VBFM_ORDER_GROUP) of a MCMC_DRAW model holding draw s), Q_{r,s}[f] that
 * scorer's per-factor sum (entries in ascending id); so raw_s is bit for bit what vbfm_recommend returns
 * with clip = 0 for the one-draw model of draw s. The moments are shifted by raw_0 and formed in draw
 * order, every operation rounded on its own; invS = 1.0 / S is rounded once on the host:
 *     a = 0;  b = 0;  for s = 1 .. S - 1:  d = raw_s - raw_0;  a = a + d;  b = fma(d, d, b)
 *     am   = a * invS
 *     mean = raw_0 + am
 *     var  = max((b - a * am) * invS, 0)
 *     sd   = sqrt(var + (noise ? na : 0))
 *     key  = fma(beta, sd, mean)
 * na is the mean over the draws of 1 / alpha_s: summed in draw order, then divided by S, once on the
 * host. Every pair is formed by exactly these expressions, whatever tile, slice or chunk it falls in,
 * and the ranking is the total order on key (larger first, equal keys by smaller candidate index), so
 * idx, key, score, var and count are bit-identical whatever the chunk size and the launch geometry. A
 * pair whose mean, var or key is not finite is never returned and is counted in nonfinite_pairs (a
 * non-finite raw_s of any draw makes a, and so mean, non-finite). S = 1, or S identical draws: a = 0,
 * mean = raw_0, var = 0, and with noise = 0 key is raw_0: vbfm_recommend's results of that draw, bit
 * for bit. Returned for each survivor, best first: idx; key; var (the spread of the raw values,
 * without the noise term); score = mean with clip = 0, and with clip = 1 what vbfm_score returns for
 * the chain on the pair's row ("chains of draws" above): sum = sum + p_s in draw order with
 * p_s = clip(raw_s, min_target, max_target), task c Phi(raw_s); then sum / S; then the min / max to the
 * target range, task c [0, 1]. The ranking is always on the raw mean (ranking on clipped values would
 * tie every saturated pair). beta is any finite double; beta = 0 with noise = 0 ranks on the chain
 * mean; noise = 1 is refused for a model of task c. Limits as vbfm_recommend.
 *
 * vbfm_candidates_create_chain makes the set vbfm_recommend_chain takes (it refuses any other, and
 * vbfm_recommend / vbfm_recommend_ucb refuse this one): every draw's sums and bases, S * (k + 1) *
 * Mpad * 8 bytes with Mpad the candidate count rounded up to 128, checked against the free memory
 * before anything is allocated; the refusal names both figures. vbfm_candidates_count and
 * vbfm_candidates_destroy serve it too. A chunk of context rows also holds its prepared sums,
 * S * (k + 1) * 8 bytes a row, so vbfm_recommend_chain cuts the contexts so that staged rows plus those
 * fit chunk_bytes (at least 8 rows a chunk while there are that many; a larger row is a chunk by
 * itself). */
int vbfm_candidates_create_chain(vbfm_candidates **out, vbfm_model *m, const vbfm_csr *rows, int32_t unknown_ids);
typedef struct {
	int32_t topn;          /* the four fields of vbfm_recommend_opts */
	int32_t clip;
	int32_t unknown_ids;
	uint64_t chunk_bytes;
	double beta;           /* finite */
	int32_t noise;         /* 1: sd is of y (var + the draws' mean of 1 / alpha), 0: of the raw value across the draws */
} vbfm_recommend_chain_opts;
/* contexts, exclusions, idx, count and the stats as vbfm_recommend; key, score, var [B * topn] (NaN
 * beyond count), each may be NULL. */
int vbfm_recommend_chain(vbfm_model *m, const vbfm_candidates *c, const vbfm_csr *contexts, const uint64_t *excl_ptr,
                         const uint32_t *excl_idx, const vbfm_recommend_chain_opts *o, int32_t *idx, double *key,
                         double *score, double *var, uint32_t *count, vbfm_recommend_stats *st);

/* ---- ranking held-out candidates (additive to ABI 4: new functions and structs only) ----------------
 * No reference counterpart. The three calls above return at most VBFM_REC_MAX_TOPN entries; held-out
 * evaluation (HR@N, NDCG@N, MRR, AUC) needs the exact position of given candidates -- the positives of
 * a context -- among ALL candidates. vbfm_rank_positives returns it, under the total order of the call
 * that `ranking` names: VBFM_RANKING_MEAN vbfm_recommend, VBFM_RANKING_UCB vbfm_recommend_ucb (beta,
 * noise), VBFM_RANKING_CHAIN vbfm_recommend_chain (beta, noise).
 *
 * For context c a candidate j is RANKABLE when it is not on c's exclusion list and its pair is ok for
 * the ranking: MEAN raw(c, j) finite; UCB raw, T and key finite; CHAIN mean, var and key finite --
 * the conditions under which that call would return the pair. key(c, j) is formed by that call's very
 * expressions (raw; or key of "ranking by mean + beta * sd"; or key of "ranking a chain of draws"),
 * the sums in the same order, and the order is the same: larger key first, equal keys by smaller index.
 *
 * Input: contexts, excl_ptr / excl_idx exactly as vbfm_recommend takes them (non-decreasing lists,
 * repeats allowed, a repeated index counts once); pos_ptr [B + 1] / pos_idx [P]: context r's positives
 * are the candidate indices pos_idx[pos_ptr[r] .. pos_ptr[r + 1]), strictly ascending, < M, none of
 * them on r's exclusion list. Output:
 *     key [P]     key(c, p) of positive p of context c, in pos_idx order; NaN when the pair is not ok
 *     rank [P]    the rankable candidates j of c that are before p in the order (key(c, j) larger, or
 *                 equal with j < p); -1 when p's own pair is not ok. The other positives of c count
 *                 like any candidate (their keys are returned: the caller can take them out)
 *     ranked [B]  the rankable candidates of c (also for a context without positives)
 * The defining property: rank[p] is the position of p in the list the ranking's call would return were
 * topn unbounded. If 0 <= rank[p] < topn <= VBFM_REC_MAX_TOPN, that call (same exclusions, clip = 0)
 * returns idx[c][rank[p]] == pos_idx[p], with the bits of key[p] as its score (vbfm_recommend) or key
 * (the other two), and its count[c] is min(topn, ranked[c]). Every output is an integer or the bits of
 * the one pair expression, so all of them are identical whatever the chunk size, the slice count, the
 * context tile and the number of passes (a wave holds 8 positives of a context; a context with more is
 * passed over again, stats passes).
 *
 * Refused before any device work, the message naming the offender: a null argument; ranking outside
 * the three; pos_ptr not starting at 0 or not monotone; a positive >= M (row and index named); a
 * positive list that is not strictly ascending; a positive that is on its context's exclusion list
 * (row and index named); unknown_ids outside 0 / 1; the model and candidate-set refusals of the
 * ranking's own call (a chain model or set with MEAN / UCB, any other with CHAIN, a model without
 * variances or a set of vbfm_candidates_create with UCB, a set of another model, noise = 1 on a chain
 * of task c); beta not finite; noise outside 0 / 1; beta != 0 or noise != 0 with VBFM_RANKING_MEAN;
 * num_factor > 256. The exclusion lists are checked as vbfm_recommend checks them. */
#define VBFM_RANKING_MEAN 0
#define VBFM_RANKING_UCB 1
#define VBFM_RANKING_CHAIN 2
typedef struct {
	int32_t ranking;       /* VBFM_RANKING_* */
	int32_t unknown_ids;   /* of the context rows: 0 refuse, 1 skip the entry */
	uint64_t chunk_bytes;  /* as vbfm_recommend_opts */
	double beta;           /* UCB, CHAIN: finite; MEAN: 0 */
	int32_t noise;         /* UCB, CHAIN: as those calls' opts; MEAN: 0 */
} vbfm_rank_positives_opts;
typedef struct {
	uint32_t n_chunks;
	uint64_t pairs;                /* B * M */
	uint64_t nonfinite_pairs;      /* pairs that are not ok, excluded ones included */
	uint64_t positives;            /* P */
	uint64_t nonfinite_positives;  /* positives of rank -1 */
	uint32_t passes;               /* the most passes a chunk took: ceil(its longest positive list / 8), at least 1 */
	double ms_prepare, ms_keys, ms_count, ms_finish;   /* device time of the chunks' row preparation, listed-pair, counting and finish kernels, summed */
	double ms_total;               /* host wall time of the call */
} vbfm_rank_positives_stats;
/* key, rank: [P], required when P > 0; ranked: [B]; st may be NULL. Failures are in vbfm_model_last_error(m). */
int vbfm_rank_positives(vbfm_model *m, const vbfm_candidates *c, const vbfm_csr *contexts, const uint64_t *excl_ptr,
                        const uint32_t *excl_idx, const uint64_t *pos_ptr, const uint32_t *pos_idx,
                        const vbfm_rank_positives_opts *o, double *key, int64_t *rank, uint32_t *ranked,
                        vbfm_rank_positives_stats *st);

/* ---- fold-in: new attributes into a VB model (additive to ABI 4: new functions and structs only) ------
 * No reference counterpart. A model m of a VB kind (VBFM_MODEL_VB, VBFM_MODEL_VB_ONLINE) with D attributes
 * and k factors is extended by attributes it has never seen -- a user who signed up after training --
 * from support rows that mention them, everything the model knows held fixed. With all other parameters
 * frozen the prediction of a row holding ONE new attribute j (value x) is linear in j's (w, v_1..v_k):
 *     yhat_r = base_r + x w + x sum_f A_r[f] v[f]
 * so the VB update of those k + 1 parameters is the reference's own update_w / update_v
 * (fm_learn_vb.h:527-644) restricted to attribute j, different new attributes do not interact, and each
 * is a small independent problem over the rows that mention it.
 *
 * Input: support rows (vbfm_csr) with float target[num_rows]. An entry with id < D is frozen, one with
 * id >= D is new; a valid row holds EXACTLY ONE new entry (id j, value x_r) and j < D_out, where D_out is
 * num_attribute_out or, if that is 0, the largest new id + 1 (D for no rows). A row with no new entry, with
 * two, or with j >= D_out fails the call; the message names the first such row and the id.
 *
 * Frozen sums of row r: exactly what the lane-group scorer produces for the row with its new entry left
 * out (vbfm_score with unknown_ids = skip, VBFM_ORDER_GROUP, the row preparation of vbfm_recommend_ucb):
 * base_r the unclipped mean, A_r[f] = sum mu_v x, B_r[f] = sum sigma_v x^2 over the frozen entries in
 * ascending id.
 *
 * Priors (precisions): the model file holds no hyper-parameters, so lambda_w and lambda_v[f] are given
 * (prior_w > 0, prior_v[k]) or derived as the reference's hyper step does (fm_learn_vb.h:474-498) over the
 * ids [prior_lo, prior_hi) of the model as its one group (0, 0: [0, D)), n = prior_hi - prior_lo:
 *     lambda_w = n / sum_i (mu_w_i^2 + sigma_w_i)      lambda_v[f] = n / sum_i (mu_v_if^2 + sigma_v_if)
 * so that new users can take the user block's prior. The sums are formed on the device in a fixed order
 * (256 strided partial sums, each in ascending id, then a fixed tree): the same model gives the same
 * bits every time. With k1 = 0 lambda_w is neither read nor derived (prior_used[0] = 0).
 *
 * The sweep for one new attribute j over its rows R_j in the caller's order; alpha, mu_0_dash and every
 * frozen parameter stay fixed:
 *     w = 0; v[f] = 0; s_w = 1 / lambda_w; s_v[f] = 1 / lambda_v[f];  e_r = target_r - base_r
 *     for pass = 1 .. passes:
 *       if k1:  S = sum x_r^2;  M = sum x_r (e_r + x_r w)
 *               s' = 1 / (lambda_w + alpha S);  w' = s' alpha M;  guards (update_w, :545-565)
 *               e_r += x_r (w - w');  w = w';  s_w = s'
 *       for f = 0 .. k - 1:
 *               h = A_r[f];  h1 = B_r[f]
 *               S = sum x_r^2 (h^2 + h1);  M = sum x_r h (e_r + x_r v[f] h)
 *               s' = 1 / (lambda_v[f] + alpha S);  v' = s' alpha M;  guards (update_v, :600-619)
 *               e_r += x_r h (v[f] - v');  v[f] = v';  s_v[f] = s'
 *       if tol > 0 and the largest |new - old| mean of this pass <= tol: stop this column
 * The guards are the reference's: a non-finite s' keeps the old sigma; a non-finite mean keeps the old
 * one, skips its e update and is counted in nonfinite_updates (its |new - old| is 0). h is the frozen sum
 * itself: the reference's q - x mu is the same number without the rounding of adding and subtracting the
 * attribute's own term. t, tq and tz are not kept: only alpha's update reads them, and alpha is fixed.
 * An id in [D, D_out) without a row gets {0, 1 / lambda}. With k1 = 0 the new w entries are {0, 0} (the
 * scorer never reads them). The sums S and M are formed by a group of lanes (the rows across the lanes,
 * a fixed butterfly): a column's result depends on its rows, the lane width and nothing else -- not the
 * chunk size, the grid or its neighbours -- and differs from a row-order fp64 sum by the rounding of a
 * reordered sum.
 *
 * The extended model *out is a new handle, independent of m: same kind, task, scalars, alpha and iter,
 * num_attribute = D_out, entries [0, D) byte-identical to m's. Every consumer takes it unchanged:
 * vbfm_score, vbfm_candidates_create[_var], vbfm_recommend[_ucb], vbfm_model_write. m is not changed.
 * Rows with several new attributes (new user x new item), refitting ids the model has, ALS / MCMC models
 * and updating alpha or the hyper-parameters are out of scope.
 *
 * Refused, with a message that names the offender and *out = NULL: a null argument; a model that is not
 * of a VB kind (the message names the kind); passes < 1; num_factor > 256; a given prior that is not
 * finite or not positive (prior_w < 0 included; prior_w = 0 derives); a prior id range that is empty or
 * not inside [0, D); a derived prior that is not finite. Failures are in vbfm_model_last_error(m). */
typedef struct {
	int32_t passes;               /* >= 1 */
	double tol;                   /* 0: run every pass */
	double prior_w;               /* 0: derive; else finite and > 0 */
	const double *prior_v;        /* [k] or NULL: derive */
	uint32_t prior_lo, prior_hi;  /* 0, 0: [0, D) */
	uint32_t num_attribute_out;   /* 0: largest new id + 1 */
	int32_t lanes;                /* 0: auto; else a width of the table in csrc/vbfm_fold.hip: 4, 8, 16, 32, 64 or
	                                 256 (one workgroup per column) (tests, tuning) */
	uint64_t chunk_bytes;         /* 0: VBFM_SCORE_CHUNK_DEFAULT; staged rows plus their prepared planes */
} vbfm_fold_opts;
typedef struct {
	uint32_t new_attributes;      /* D_out - D */
	uint32_t with_rows;           /* of those, the ones some row mentions */
	uint32_t longest_column;      /* rows */
	uint32_t passes_max;          /* the largest pass count a column ran */
	uint32_t not_converged;       /* tol > 0: columns with rows that ran every pass without meeting tol */
	uint64_t rows, nonfinite_updates;
	uint32_t n_chunks;
	int32_t lanes;                /* the width used */
	double ms_prepare, ms_fold;   /* device time of the chunks' row preparation / fold kernels, summed */
	double ms_total;              /* host wall time of the call */
} vbfm_fold_stats;
/* resid: NULL or [rows], e_r after the last pass (= target_r - the extended model's unclipped mean of row
 * r, up to rounding); prior_used: NULL or [1 + k], lambda_w then lambda_v[f]; st may be NULL. */
int vbfm_fold_in(vbfm_model **out, vbfm_model *m, const vbfm_csr *rows, const float *target,
                 const vbfm_fold_opts *o, double *resid, double *prior_used, vbfm_fold_stats *st);
/* any model handle but a chain (that is refused, the message names vbfm_chain_save) to a model file,
 * through the host writer of vbfm_model_save: load -> write reproduces a file byte for byte when iter is
 * the file's */
int vbfm_model_write(vbfm_model *m, const char *path, uint32_t iter);

#ifdef __cplusplus
}
#endif
#endif /* VBFM_H_ */
