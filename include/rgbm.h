/*
 * rgbm.h -- C-ABI of librepairgbm.so: the MI355X-native (HIP, gfx950) repair-model engine.
 *
 * The reference (maropu/spark-data-repair-plugin) has no FFI of its own: its seam for this hot
 * path is the scikit-learn estimator protocol that python/repair/train.py and
 * python/repair/model.py drive against LightGBM 3.3.1.  Each entry point below names the
 * reference interface it replaces (paths relative to /root/reference).  The Python side binds
 * these with ctypes (spark-data-repair-plugin_amd/repair/gbm.py); INTEGRATION.md shows the stub
 * a maintainer of the reference would add.
 *
 * Conventions
 *   - every array is caller-owned, plain pointers + sizes, never retained after return;
 *   - feature matrices are int32 label codes, COLUMN-MAJOR ([column][row]); code -1 (or any code
 *     outside [0, n_codes)) means NULL / unknown category == LightGBM's NaN;
 *   - return 0 on success, negative on error; rgbm_last_error() gives the (thread-local) message;
 *   - device_id >= 0 selects the HIP device; there is NO CPU fallback: without a usable GPU every
 *     compute entry point fails with RGBM_ERR_NO_DEVICE;
 *   - threads: every call is re-entrant.  Training / prediction calls own a HIP stream each, so any number of threads may
 *     train from ONE table at once.  The relational table calls (detect / null / gather / count / read / write / pmf) share
 *     the table's stream and scratch and are serialised per table by the library; the two-step detect -> rgbm_table_cells_fetch
 *     protocol keeps its result in the table, so one thread at a time should drive that pair.
 */
#ifndef RGBM_H_
#define RGBM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RGBM_OK 0
#define RGBM_ERR_ARG (-1)
#define RGBM_ERR_PARAM (-2)
#define RGBM_ERR_LABEL (-3)
#define RGBM_ERR_NO_DEVICE (-10)
#define RGBM_ERR_HIP (-11)
#define RGBM_ERR_NOMEM (-12)
#define RGBM_ERR_FORMAT (-20)

#define RGBM_OBJ_BINARY 0
#define RGBM_OBJ_MULTICLASS 1
#define RGBM_OBJ_REGRESSION 2

typedef struct rgbm_model rgbm_model; /* opaque; host-resident trees, lazily mirrored on a device */
typedef struct rgbm_table rgbm_table; /* opaque; an int32 code table resident in HBM */

/* LightGBM parameters as set by python/repair/train.py:102-115 (fixed) and :148-156 (searched),
 * under their LightGBM core names (sklearn aliases in comments). */
typedef struct {
    int32_t objective;    /* train.py:97-100  binary | multiclass | regression */
    int32_t num_class;    /* train.py:118-119 (multiclass only; binary uses 2) */
    int32_t n_estimators; /* model.lgb.n_estimators, train.py:53-55 */
    int32_t num_leaves;   /* searched, train.py:149 */
    int32_t max_depth;    /* model.lgb.max_depth, train.py:43-44 */
    int32_t max_bin;      /* model.lgb.max_bin, train.py:45-46 (2..255) */
    int32_t min_data_in_leaf; /* min_child_samples, train.py:153 */
    int32_t min_data_in_bin;  /* LightGBM default 3 */
    int32_t bagging_freq;     /* subsample_freq, train.py:151 */
    int32_t seed;             /* random_state=42, train.py:113 */
    int32_t device_id;        /* HIP device ordinal */
    int32_t reserved;         /* flags: RGBM_FLAG_ROW_SHARDED, RGBM_FLAG_NO_MODEL, RGBM_FLAG_WHOLE_TABLE */
    double learning_rate;           /* model.lgb.learning_rate, train.py:41-42 */
    double lambda_l1;               /* reg_alpha, train.py:47-49 */
    double lambda_l2;               /* reg_lambda, train.py:155 */
    double min_gain_to_split;       /* min_split_gain, train.py:50-52 */
    double min_sum_hessian_in_leaf; /* min_child_weight, train.py:154 */
    double bagging_fraction;        /* subsample, train.py:150 */
    double feature_fraction;        /* colsample_bytree, train.py:152 */
} rgbm_params;

/* Per-call measurements filled by the training entry points (bench.py roofline inputs). */
typedef struct {
    double hist_ms;          /* sum of hist_build kernel time (HIP events on the launch stream) */
    double total_ms;         /* whole training call, device side */
    int64_t hist_launches;   /* number of hist_build launches */
    int64_t hist_rows;       /* rows scanned by hist_build over all launches and class trees (a fit on the distinct-row view: rows STREAMED, see rgbm_table_distinct_view_info) */
    int64_t hist_bytes;      /* algorithmic bytes: rows * (F + 8) (+4 per row via an index list) */
    int64_t root_rows;       /* of which full-table (root) scans */
    double root_ms;          /* hist_build time spent in root scans */
    int64_t trees;           /* trees grown */
    double route_ms;         /* always 0 since numerics version 200: DataPartition::Split of a level is part of the level pass (k_level_mt), */
    int64_t route_launches;  /* whose time is in hist_ms; the fields keep the struct layout of version 102 */
    /* version 220: what the LDS-atomic floor of the histogram build is priced with (bench.py roofline.classes.*.atomic_floor_us) */
    int64_t root_atomics_per_row;   /* 64-bit LDS atomics a root pass issues per accumulated row: 2 per joint-bin group (or per feature without joint bins) */
    int64_t level_atomics_per_row;  /* ... a level pass issues per built row: 2 per feature */
} rgbm_train_stats;

/* Number of usable HIP devices (0 if none). */
int rgbm_device_count(void);
/* The library parks freed device blocks in a caching pool (at most RGBM_POOL_MB, default 65536; 0 disables it).
 * rgbm_release_cache gives all of them back to the driver, e.g. before another allocator needs the memory, together with the
 * page-locked host blocks the library keeps for the tree harvest of batched fits and for the outputs of repair chains. */
int rgbm_release_cache(void);
/* Message of the last failing call on this thread. */
const char* rgbm_last_error(void);
/* Library / numerics-spec version (bumped whenever results could change). */
int rgbm_version(void);

/* ---- fit --------------------------------------------------------------------------------
 * Replaces `lgb.LGBMClassifier(**p).fit(X, y)` / `lgb.LGBMRegressor(**p).fit(X, y)`:
 * python/repair/train.py:121-131 (construction), :171-172 (inside cross_val_score), :215-216
 * (final fit).
 *   X_colmajor [f][n]   feature codes;  n_codes[f] dictionary sizes
 *   y_code [n]          class index (0..n_y_codes-1) or, for regression, index into y_value
 *   y_value [n_y_codes] regression only: the distinct target values, ascending
 *   class_weight [n_y_codes] or NULL: per-label weight (sklearn class_weight='balanced' is
 *                       n / (n_labels * count_label), train.py:39-40,105); sample_weight [n] or NULL
 */
int rgbm_train(const int32_t* X_colmajor, int64_t n, int32_t f, const int32_t* n_codes,
               const int32_t* y_code, int32_t n_y_codes, const double* y_value,
               const double* class_weight, const double* sample_weight,
               const rgbm_params* p, rgbm_model** out, rgbm_train_stats* stats /* may be NULL */);

/* ---- predict_proba / predict ------------------------------------------------------------
 * Replaces `model.predict_proba(X)` / `model.predict(X)`: python/repair/model.py:1120,1130.
 * out: binary [n][2] = {1-p, p}; multiclass [n][num_class]; regression [n]. */
int rgbm_predict(const rgbm_model* m, const int32_t* X_colmajor, int64_t n, int32_t f,
                 int32_t device_id, double* out);

/* ---- chained repair ---------------------------------------------------------------------
 * Replaces the body of the grouped-map UDF `repair(pdf)`: python/repair/model.py:1107-1133.
 * For each model in order: score every row from the listed feature columns, arg-max (first
 * maximum, like numpy), then overwrite ONLY the NULL cells of the target column with
 * class_code[label] so that later models see the repair.
 *   table [c][n] codes, modified in place; feat_cols/feat_off[T+1]; class_code/class_off[T+1]
 *   (an empty class list == regression target: column left untouched);
 *   out_label [T][n] class index (-1 for regression), out_prob [T][n] its probability / raw value. */
int rgbm_repair_chain(const rgbm_model* const* models, int32_t T, const int32_t* target_col,
                      const int32_t* feat_cols, const int32_t* feat_off,
                      const int32_t* class_code, const int32_t* class_off,
                      int32_t* table_colmajor, int64_t n, int32_t c, int32_t device_id,
                      int32_t* out_label, double* out_prob);

/* ---- HBM-resident table (the batch path: python/repair/model.py:768-815 without toPandas) ---
 * Upload the label-encoded table once; train one model per target attribute on the rows whose
 * target cell is non-NULL (model.py:776), all other listed columns being the features. */
int rgbm_table_create(const int32_t* codes_colmajor, int64_t n, int32_t c, const int32_t* n_codes,
                      int32_t device_id, rgbm_table** out);
/* CATEGORICAL columns (kind 1; default 0 = ordered codes): a model trained from this table records which codes of the column no
 * training row held, and treats them as MISSING when it predicts -- what the reference's per-model encoders do with a category they
 * have not seen (python/repair/model.py:701-729: the encoders are fitted on the training frame of each model).  Such models are
 * serialised as format version 2 (version 1 + one bitmap per feature); row gathers inherit the kinds. */
int rgbm_table_set_column_kind(rgbm_table* t, int32_t col, int32_t kind);
/* NUMERIC columns: the ascending distinct values behind the codes 0..n_codes[col]-1 (one per code; n = 0 clears).  The trainer then
 * places bin bounds at the midpoints of the VALUES, as LightGBM does on raw numbers (bin.cpp GreedyFindBin), instead of at the
 * midpoints of the rank codes: it only matters for values that no training row of the model holds.  Row gathers inherit it. */
int rgbm_table_set_column_values(rgbm_table* t, int32_t col, const double* values, int32_t n);
/* Pinned host memory for the code matrix (north_star: "pinned int32 column-major feature matrix"): a block from
 * rgbm_host_alloc is page-locked, so rgbm_table_create copies it at PCIe DMA speed without staging.  Any other block is
 * page-locked in place for the duration of the copy (and copied the plain way if that fails). */
int rgbm_host_alloc(size_t bytes, void** out);
void rgbm_host_free(void* p);
void rgbm_table_free(rgbm_table* t);
int rgbm_table_train(const rgbm_table* t, int32_t target_col, const int32_t* feat_cols, int32_t f,
                     const double* y_value /* regression dictionary or NULL */,
                     const double* class_weight /* [n_codes[target]] or NULL */,
                     const rgbm_params* p, rgbm_model** out, rgbm_train_stats* stats);
/* Rows with multiplicities (round 6; a VARIANT of the workload, reported apart from the row-for-row line): row i stands for mult[i] (1..255)
 * identical rows of a larger table.  The reference has no counterpart -- its frames (python/repair/model.py:768-815) hold every row; on the
 * categorical tables it repairs a quarter of the rows are distinct -- but the result is defined by it: every later rgbm_table_train on this
 * table returns byte for byte the model the EXPANDED table gives (identical rows take identical paths and gradients; all sums are exact
 * integers).  NULL clears.  Level grower only (1 <= max_depth <= 7), at most 32 features with a free byte in the last 16-feature record, no
 * bagging, no per-row weights: a training call that cannot honour it fails with RGBM_ERR_PARAM.  A table that carries multiplicities never
 * gets a distinct-row view (rgbm_table_distinct_view_info); setting or clearing them drops the view. */
int rgbm_table_set_row_multiplicity(rgbm_table* t, const uint8_t* mult /* [n] or NULL */);
/* The multiplicities a table carries, one per row (1 everywhere when it carries none). */
int rgbm_table_read_row_multiplicity(const rgbm_table* t, uint8_t* mult_out /* [n] */);
/* The DISTINCT rows of a resident table, found on the device (the host statement is repair.pipeline.distinct_rows; the reference has no
 * counterpart, see rgbm_table_set_row_multiplicity).  All c columns take part and NULL (-1, or any code outside [0, n_codes)) is a value of
 * its own.  The result is a function of the table alone:
 *   - `out` holds one group per distinct row, the groups in order of FIRST OCCURRENCE (ascending position of the first row of each group);
 *   - a group of cnt rows is kept as ceil(cnt / 255) consecutive copies with the multiplicities 255, .., 255, cnt - 255 * (copies - 1),
 *     which are attached to `out` as rgbm_table_set_row_multiplicity attaches them: rgbm_table_train on `out` returns the models of `t`;
 *   - `out` inherits the column kinds and column values, like rgbm_table_gather_rows;
 *   - inverse_out[i] = position in `out` of the first copy of row i's group;  *n_out = rows of `out`.
 * RGBM_ERR_PARAM: more than 2^30 rows; a table that carries multiplicities itself; or a working set -- everything the call allocates with the
 * output at its largest: 8 B per slot of >= 2n slots (a power of two) + (47 + 8 per key word + 4c) B per row -- above half of the device memory.
 * The other table entries do not read multiplicities: on `out` they see its rows.
 * What rgbm_table_train refuses on a table with multiplicities it refuses on `out`: besides the parameters named at
 * rgbm_table_set_row_multiplicity, a table of 17 to 31 features trains only when both 16-feature chunks fit one level pass and the features pack
 * into at most 15 joint-bin groups of at most 256 bins (about: fewer than 16 features with more than 16 bins).  Callers fall back to `t`. */
int rgbm_table_distinct_rows(const rgbm_table* t, rgbm_table** out, int64_t* n_out, int64_t* inverse_out /* [n] or NULL */);
/* The DISTINCT-ROW VIEW.  rgbm_table_train deduplicates a table by itself: the first training call that can use it builds, once per table
 * and version of its contents, the table rgbm_table_distinct_rows makes (concurrent callers wait for that one build), and every fit whose
 * model comes out the same bytes trains on it -- level grower (1 <= max_depth <= 7), classifier objective, no bagging, not row-sharded, at most
 * 32 features with a free byte in the last 16-feature record, a table without multiplicities of its own and of at least RGBM_DISTINCT_MIN_ROWS
 * rows (default 2^20), whose distinct rows are at most RGBM_DISTINCT_MAX_RATIO (default 0.5) of its rows.  What the multiplicity trainer refuses
 * on the view (see rgbm_table_distinct_rows) trains on the whole table inside the same call: no error reaches the caller for it.  Every entry
 * point that writes cells, column kinds, column values or multiplicities drops the view; rgbm_table_free frees it.  RGBM_DISTINCT=0 (read at
 * every training call) and RGBM_FLAG_WHOLE_TABLE (per call) switch it off.  A fit that trained on the view reports in rgbm_train_stats the rows
 * its kernels streamed (root_rows exactly; the level passes' share of hist_rows / hist_bytes pro rata), not rows weighted by multiplicity.
 *   state: 0 no pass yet (or dropped), 1 built (*rows = its rows), 2 not worth it (*rows = the distinct rows; no table kept),
 *          3 cannot (more than 2^30 rows, working set above half of the device memory, or the allocator refused; the reason goes to stderr
 *          under RGBM_TIMING).  *builds = distinct passes run for this table object.  Any of the three outputs may be NULL. */
int rgbm_table_distinct_view_info(const rgbm_table* t, int32_t* state, int64_t* rows, int64_t* builds);
/* Whether a fit of this shape MAY train on the view: a function of its arguments alone (no device), 1 or 0.  rows, f = rows and features of the
 * fit; table_has_mult = the table carries multiplicities of its own; min_rows <= 0 takes the built-in default. */
int rgbm_distinct_view_eligible(int64_t rows, int32_t f, const rgbm_params* p, int32_t table_has_mult, int64_t min_rows);
/* ---- many small fits in one go ------------------------------------------------------------------
 * Replaces the LOOP over fits of python/repair/train.py:158-209 (every hyper-parameter trial is `cross_val_score`: n_splits fits of
 * the same estimator on row subsets of one frame, train.py:171-172) and of python/repair/model.py:768-815 on the reference's default
 * <= 10 000-row training samples (model.py:755-766).  Each spec is one rgbm_table_train call -- its own table (e.g. a fold gathered
 * with rgbm_table_gather_rows), target, features, class weights and parameters -- and every model is the one that call returns, bit
 * for bit; what changes is the schedule: all fits of the batch advance through their boosting iterations TOGETHER, three kernel
 * launches per iteration for the whole batch (csrc/rgbm_small.h: one workgroup grows one class tree of one fit).  Fits the fused
 * kernels do not cover (tables above RGBM_SMALL_ROWS = 65536 rows, more than 256 leaves, row-sharded calls) run one by one inside.
 * A fit with a valid_table always takes the batched path's scoring (its table must then be small enough for the fused kernels).
 * out_status[i] = RGBM_OK or fit i's error code (out_models[i] = NULL then): one failing fit does not fail the batch, which is the
 * reference's contract (train.py:227-229: a failing build yields PoorModel).  All tables must live on one device. */
typedef struct {
    const rgbm_table* table;
    int32_t target_col, n_features;
    const int32_t* feat_cols;
    const double* y_value;        /* regression dictionary or NULL */
    const double* class_weight;   /* [n_codes[target]] or NULL */
    const rgbm_params* params;
    /* optional: score a validation table while the fit trains (cross_val_score, train.py:171-172, without building a predictor): the
     * rows of valid_table get the label / value model.predict would give them -- the same bits, the trees are added to their scores
     * in the predictor's order.  valid_label_out [rows of valid_table]: arg-max class index (-1 for regression);
     * valid_value_out [rows]: its probability / the regression value.  NULL valid_table: nothing is scored. */
    const rgbm_table* valid_table;
    int32_t* valid_label_out;
    double* valid_value_out;
} rgbm_fit_spec;
int rgbm_table_train_batch(const rgbm_fit_spec* fits, int32_t n_fits, rgbm_model** out_models /* [n_fits] */, int32_t* out_status /* [n_fits] */);
/* What the calling thread's last rgbm_table_train_batch call did with each of its n fits (n must be that call's n_fits):
 * out[4 * i ..] = {route, scan_waves, nchunk, lds_bytes} of fit i.  route 0 = the fit failed before a route was chosen, 1 = the fused
 * kernels, 2 = the single-fit trainer because the fit is not eligible (rows above RGBM_SMALL_ROWS, more than 256 leaves, more than 255
 * features, a row-sharded call or row multiplicities), 3 = the single-fit trainer because the batch held one eligible fit, 4 = the
 * single-fit trainer because the fit's working set exceeds the LDS.  Of a route-1 fit: scan_waves = the waves per child of the packed
 * threshold scan (0: one wave per feature), nchunk = its 16-feature chunks, lds_bytes = the dynamic LDS its class trees use (the launch
 * is sized for the largest fit of the batch); 0 otherwise (route 4: lds_bytes = what was too much).  A function of the fits and of the
 * environment switches RGBM_SMALL_ROWS / RGBM_SMALL_PACKED=0 / RGBM_SMALL_ALWAYS=1; tests assert it before they compare models. */
int rgbm_table_train_batch_report(int32_t* out /* [n][4] */, int32_t n);
/* Chained repair of rows [row_begin, row_begin+n_rows) of the resident table, in place in HBM.
 * out_label/out_prob [T][n_rows] are copied back to the host (either may be NULL). */
int rgbm_table_repair_chain(rgbm_table* t, const rgbm_model* const* models, int32_t T,
                            const int32_t* target_col, const int32_t* feat_cols, const int32_t* feat_off,
                            int64_t row_begin, int64_t n_rows, int32_t* out_label, double* out_prob);
/* Copy one column of the resident table back to the host. */
int rgbm_table_read_column(const rgbm_table* t, int32_t col, int32_t* out /* [n] */);

/* ---- the relational steps either side of the models, on the resident table -------
 * Cells are (row position, column index) pairs; the host maps row ids <-> positions.  Result lists are
 * ordered -- by position in the given column list, then ascending row -- so they are a deterministic function
 * of the table.  A detect / rows_of_cells call leaves its result in the table object (device memory) and
 * returns the count; rgbm_table_cells_fetch copies it out.  One such call at a time per table. */
/* NullErrorDetector (src/main/scala/.../python/ErrorDetectorApi.scala:128-157): the NULL cells of `cols`. */
int rgbm_table_detect_nulls(rgbm_table* t, const int32_t* cols, int32_t n_cols, int64_t* n_cells_out);
/* The VALUE detectors (RegExErrorDetector / DomainValues / GaussianOutlierErrorDetector, ErrorDetectorApi.scala:159-187, 249-300)
 * with the NULL detector fused in: on a label-encoded column each of them is a predicate on the dictionary code (the host evaluates
 * a regex once per distinct value, Tukey fences keep a contiguous code range of an ascending numeric dictionary).  The cell
 * (row, cols[j]) with code v is an error iff   v < 0 and null_is_error[j];   or v >= 0, keep_lo[j] <= keep_hi[j] and
 * (v < keep_lo[j] or v > keep_hi[j]);   or v >= 0, flag_bits[j] != NULL and bit v of it is set (ceil(n_codes[cols[j]] / 64) words,
 * bit v = bit v % 64 of word v / 64; a code at or beyond n_codes has no bit).  keep_lo[j] > keep_hi[j]: no range test; flag_bits
 * (or an entry) NULL: no bitset.  The predicates of a column are ORed before the compaction, so every cell appears once.  Result as
 * for rgbm_table_detect_nulls.  `cols` must be distinct and in range (RGBM_ERR_ARG); n_cols == 0 gives 0 cells. */
int rgbm_table_detect_cells(rgbm_table* t, const int32_t* cols, int32_t n_cols, const uint8_t* null_is_error /* [n_cols] */,
                            const int32_t* keep_lo, const int32_t* keep_hi /* [n_cols] */,
                            const uint64_t* const* flag_bits /* [n_cols] or NULL */, int64_t* n_cells_out);
/* ConstraintErrorDetector (ErrorDetectorApi.scala:189-244) for two-tuple denial constraints of the form
 * t1&t2&EQ(t1.X1,t2.X1)&..&EQ(t1.Xm,t2.Xm)&IQ(t1.Y,t2.Y)  (i.e. X1..Xm -> Y): a row violates iff another row
 * agrees with it on every X (NULL-safe, `<=>`) and differs on Y (NULL is a value of its own).  n_eq == 0 is allowed
 * (IQ alone: every row violates as soon as Y takes two values).  Result: the violating rows x cell_cols
 * (n_cell_cols == 0: just the rows). */
int rgbm_table_detect_constraint(rgbm_table* t, const int32_t* eq_cols, int32_t n_eq, int32_t iq_col,
                                 const int32_t* cell_cols, int32_t n_cell_cols,
                                 int64_t* n_rows_out /* may be NULL */, int64_t* n_cells_out);
/* ConstraintErrorDetector for EVERY other two-tuple denial constraint the parser accepts (DenialConstraints.scala:60-95: several IQs,
 * LT / GT, LT / GT across two attributes), 2 <= n_preds <= 16 predicates.  For row i as t1 and row j as t2 a predicate compares
 * L = code(i, left_col) with R = code(j, right_col); a code outside [0, n_codes) is -1, and a code is mapped through left_rank /
 * right_rank (int32 [n_codes[col]], an entry < 0 = "this value has no number") where that pointer is not NULL:
 *   EQ  L == R (NULL equals NULL, `<=>`)      IQ  L != R (NULL is a value of its own)
 *   LT  L >= 0 && R >= 0 && L < R             GT  L >= 0 && R >= 0 && L > R
 * EQ / IQ take left_col == right_col and no rank arrays (RGBM_ERR_ARG otherwise; at most 12 distinct EQ attributes).  Row i violates
 * iff SOME row j of the table -- j == i included, as in the reference's EXISTS sub-query (ErrorDetectorApi.scala:218-223) -- makes
 * every predicate true; with EQ predicates only every row violates.  Result as for rgbm_table_detect_constraint: the ascending
 * violating rows x cell_cols.
 * The rows are grouped by the EQ attributes and the other predicates evaluated over the pairs of each group, so the call knows the
 * sum of |group|^2 before it evaluates a pair: above max_pairs (<= 0: the library default) it returns RGBM_ERR_PARAM
 * and the table's previous result stays as it was.  RGBM_ERR_PARAM also for EQ attributes that span 2^63 value combinations or more
 * and for a table of 2^31 rows or more. */
#define RGBM_DC_EQ 0
#define RGBM_DC_IQ 1
#define RGBM_DC_LT 2
#define RGBM_DC_GT 3
typedef struct rgbm_dc_pred {
    int32_t op;                 /* RGBM_DC_* */
    int32_t left_col;           /* attribute of t1 */
    int32_t right_col;          /* attribute of t2 */
    int32_t reserved;           /* 0 */
    const int32_t* left_rank;   /* [n_codes[left_col]] or NULL */
    const int32_t* right_rank;  /* [n_codes[right_col]] or NULL */
} rgbm_dc_pred;
int rgbm_table_detect_dc(rgbm_table* t, const rgbm_dc_pred* preds, int32_t n_preds, const int32_t* cell_cols, int32_t n_cell_cols,
                         int64_t max_pairs, int64_t* n_rows_out /* may be NULL */, int64_t* n_cells_out);
/* rgbm_table_detect_dc for ORDER constraints, by sort and scan instead of pairs: the same predicate struct, the same semantics (row i
 * as t1, any row j, i included, as t2) and the same result as rgbm_table_detect_dc gives with an unlimited max_pairs -- the ascending
 * violating rows x cell_cols -- in O(n log n) whatever the groups are; no pair is evaluated, so there is no max_pairs.
 * Accepted: 1 <= n_preds <= 16 predicates of which zero to 12 distinct EQ attributes (the 2^63 key-span rule as above), no IQ, and exactly
 * one or two LT / GT predicates, within one attribute or across two, with or without rank arrays; n < 2^31 rows.  The argument errors
 * are RGBM_ERR_ARG as rgbm_table_detect_dc gives them -- among them more than 12 distinct EQ attributes, more than 16 predicates, EQ / IQ
 * across two attributes or with rank arrays, a column out of range -- but a single LT / GT predicate is a constraint here.  Well-formed
 * arguments outside the accepted set (an IQ, no or three and more LT / GT, a key span of 2^63 or more, 2^31 rows or more) are
 * RGBM_ERR_PARAM.  After either refusal the table's previous result is as it was.
 * One order predicate: L < the group's maximum of R.  Two: the group's rows sorted by R1, the suffix maximum of R2 in that order, and
 * per row a binary search for the first R1 above its L1. */
int rgbm_table_detect_dc_scan(rgbm_table* t, const rgbm_dc_pred* preds, int32_t n_preds, const int32_t* cell_cols, int32_t n_cell_cols,
                              int64_t* n_rows_out /* may be NULL */, int64_t* n_cells_out);
/* ConstraintErrorDetector for single-tuple constraints (constant predicates, e.g. t1&EQ(t1.Sex,"Female")&EQ(t1.Relationship,"Husband")):
 * bits[k] holds n_codes[cols[k]] + 1 bits (bit v = bit v % 64 of word v / 64), bit v = "the predicates on cols[k] hold for code v",
 * the last bit for NULL (a code outside [0, n_codes) is NULL).  A row violates iff its bit is set in every listed column; one
 * streaming pass.  `cols`: at least one, distinct, in range, each with a bitset (RGBM_ERR_ARG).  Result as above. */
int rgbm_table_detect_row_bits(rgbm_table* t, const int32_t* cols, int32_t n_cols, const uint64_t* const* bits /* [n_cols] */,
                               const int32_t* cell_cols, int32_t n_cell_cols, int64_t* n_rows_out /* may be NULL */, int64_t* n_cells_out);
/* Ascending positions of the rows that hold at least one of the given cells: the dirty rows of
 * python/repair/model.py:549-553 (left-semi join on the row id). */
int rgbm_table_rows_of_cells(rgbm_table* t, const int64_t* rows, int64_t n_cells, int64_t* n_rows_out);
int rgbm_table_cells_fetch(const rgbm_table* t, int64_t* rows_out /* [n] or NULL */, int32_t* cols_out /* [n] or NULL */);
/* The CELL SET of a table: the union of detector results, kept on the device between the detect calls.  A bit matrix
 * of n_cols x ceil(n / 64) 64-bit words (rounded up to whole 4096-row compaction blocks), device memory of the table's own from the pool.
 * None of these entries writes a code.
 * open:  a zeroed set over `cols`: 1 <= n_cols <= columns, distinct and in range (RGBM_ERR_ARG otherwise).  A second open replaces the set.
 * add:   ORs the table's cell list, as the last rgbm_table_detect_* call left it, into the set.  A cell whose column is not in the set (or that
 *        lies outside the table) is skipped: join semantics, as in rgbm_table_null_cells.  A row list without columns (the n_cell_cols == 0
 *        result of a constraint call) is RGBM_ERR_PARAM; an empty result adds nothing.  The cell list stays as it was.
 * emit:  compacts the set into the table's cell list -- ordered by position in `cols`, then ascending row, every cell once -- and gathers
 *        the codes those cells hold NOW (a code outside [0, n_codes) as it lies, as rgbm_table_read_cells gives it) into a device buffer of
 *        the table.  counts_out[j] = cells of cols[j].  rgbm_table_cells_fetch copies rows / columns out as for every other result,
 *        rgbm_table_cells_fetch_codes the codes.  The set stays open: emit twice gives the same result, add after emit and emit again is allowed.
 * fetch_codes: RGBM_ERR_PARAM when the cell list is no longer that of the last emit (a detect / rows_of_cells call came after it).
 * close: frees the set (rgbm_table_free does too); the last emit's cell list and codes stay fetchable.
 * add / emit without an open set are RGBM_ERR_PARAM.  After every refusal the previous cell list and the set are as they were. */
int rgbm_table_cellset_open(rgbm_table* t, const int32_t* cols, int32_t n_cols);
int rgbm_table_cellset_add(rgbm_table* t);
int rgbm_table_cellset_emit(rgbm_table* t, int64_t* n_cells_out, int64_t* counts_out /* [n_cols] or NULL */);
int rgbm_table_cells_fetch_codes(const rgbm_table* t, int32_t* codes_out /* [n_cells] */);
int rgbm_table_cellset_close(rgbm_table* t);
/* The repair run on the open set: the error cells stay in it from detection through the null-out.  Every entry is
 * RGBM_ERR_PARAM without an open set, and after every refusal the set, the cell list and the codes of the last emit are as they were.
 * add_cells: ORs host-given cells into the set, in any order and with duplicates (setErrorCells; the cells of a second pass).  A cell
 *        outside the table or of a column not in the set is skipped (join semantics, as in add); n_cells == 0 adds nothing.  The
 *        table's cell list stays as it was.  RGBM_ERR_ARG: n_cells < 0, a NULL array with n_cells > 0.
 * drop_weak: for every cell of the set's column target_col, exactly the `weak` flag that rgbm_table_cell_domains gives for that row -- on the
 *        tables of the last rgbm_table_pair_counts call and the codes as they lie now; the other arguments are that entry's -- and the
 *        cell's bit cleared where it is set.  The examined cells (ascending rows, as they were BEFORE pruning) become the table's cell list,
 *        as after a detect call; n_cells_out is their number, n_weak_out the bits cleared.  The refusals of rgbm_table_cell_domains (a
 *        pair index is looked at whatever the number of cells), and RGBM_ERR_PARAM for a target that is not a column of the set.
 * null:  writes NULL into every cell of the set, straight from the matrix; no other code changes.  n_cells_out = the cells.  A table
 *        write like rgbm_table_null_cells (the distinct-row view is dropped).  The set, the cell list and the codes of the last emit stay:
 *        those codes are then what the cells held AT THAT EMIT, no longer what they hold.
 * rows:  the ascending rows that hold at least one cell of the set become the table's cell list, as a row list without columns -- the
 *        result shape of rgbm_table_rows_of_cells, fetched with rgbm_table_cells_fetch(rows, NULL). */
int rgbm_table_cellset_add_cells(rgbm_table* t, const int64_t* rows, const int32_t* cols, int64_t n_cells);
int rgbm_table_cellset_drop_weak(rgbm_table* t, int32_t target_col, const int32_t* pair_idx, int32_t k, const int64_t* min_cnt /* [k] */,
                                 const uint8_t* single_ok /* [n_bins[target]] */, double beta, int64_t row_count, int64_t* n_cells_out,
                                 int64_t* n_weak_out);
int rgbm_table_cellset_null(rgbm_table* t, int64_t* n_cells_out);
int rgbm_table_cellset_rows(rgbm_table* t, int64_t* n_rows_out);
/* convertErrorCellsToNull (src/main/scala/.../python/RepairApi.scala:171-211): NULL the listed cells whose
 * column is one of target_cols; cells outside the table are ignored (join semantics). */
int rgbm_table_null_cells(rgbm_table* t, const int64_t* rows, const int32_t* cols, int64_t n_cells,
                          const int32_t* target_cols, int32_t n_targets);
/* The codes the given cells hold now (cells outside the table read as NULL): the `current_value` of the error cells. */
int rgbm_table_read_cells(const rgbm_table* t, const int64_t* rows, const int32_t* cols, int64_t n_cells, int32_t* codes_out);
/* Store codes into the given cells (cells outside the table are ignored).  The chained repair uses it for CONTINUOUS target
 * attributes: the regressor's prediction (python/repair/model.py:1130-1133, rounded first for integral attributes) is written
 * back as the code of the nearest dictionary value so that later models of the chain see the repaired cell. */
int rgbm_table_write_cells(rgbm_table* t, const int64_t* rows, const int32_t* cols, const int32_t* codes, int64_t n_cells);
/* New resident table made of the given rows (the dirty-row frame the chained repair runs on). */
int rgbm_table_gather_rows(const rgbm_table* t, const int64_t* rows, int64_t n_rows, rgbm_table** out);
/* New resident table: the rows of the parts one after the other; kinds and values inherited, like rgbm_table_gather_rows.
 * RGBM_ERR_PARAM: parts that differ in their columns, dictionaries (code counts, kinds, values) or device. */
int rgbm_table_concat(const rgbm_table* const* parts, int32_t n_parts, rgbm_table** out);
/* SMOTEN in code space (the over-sampling of the reference's training-data rebalancing, train.py:242-293; the statement is
 * repair/rebalance_codes.py `smoten_codes`): every column is nominal, the Value Difference Metric is fitted on the n_fit rows `fit_rows`
 *   P_f[v][c] = rows with code v in feature f and class c / rows with code v
 *   dist(a, b) = sum over the features, in `feat_cols` order, of (sum over the classes, ascending, of |P_f[a_f][c] - P_f[b_f][c]|) squared
 * in double, without contraction: the distances are the statement's, bit for bit.  For every listed class (ascending codes of the target)
 * the k nearest neighbours of each of its m fit rows among the other m - 1, ordered by (distance, position): positions count the class's
 * rows in `fit_rows` order, rows at distance 0 are neighbours, the row itself is not.  nn_out [sum m][k], class by class, may be NULL.
 * picks [pick_off[n_classes]]: for class i the rows pick_off[i] .. pick_off[i + 1] - 1 of `out` are grown from the class's rows picks[..]
 * (the caller's random draws): the target holds the class, every feature the most common code among the k neighbours of the drawn row (ties:
 * the smallest code), every other column NULL (-1).  `out` inherits kinds and values like rgbm_table_gather_rows.
 * RGBM_ERR_PARAM: k outside 1 .. 16; more than 64 features, one listed twice or equal to the target; a class with m <= k; a pick outside
 * its class; a fit row outside the table or with a NULL in the target or a feature; no row to make; P tables above 2^28 entries. */
int rgbm_table_smoten(const rgbm_table* t, int32_t target_col, const int32_t* feat_cols, int32_t f,
                      const int64_t* fit_rows, int64_t n_fit, int32_t k,
                      const int32_t* classes, int32_t n_classes,          /* ascending */
                      const int64_t* pick_off /* [n_classes + 1] */, const int64_t* picks,
                      int64_t* nn_out /* [sum m][k], class by class, or NULL */, rgbm_table** out /* pick_off[n_classes] rows */);
/* Rows per code of one column (+ NULL count): class weights (train.py:39-40,105), domain statistics. */
int rgbm_table_count_codes(const rgbm_table* t, int32_t col, int64_t* counts_out /* [n_codes[col]] */,
                           int64_t* n_null_out /* may be NULL */);
/* Column statistics of a resident table in ONE call (RepairMiscApi.computeAndGetStats in code space; the statement is
 * repair.table_stats.column_stats).  stats_out [n_cols][6] = {nulls, distinct, min_code, max_code, len_sum, len_max};
 * edges_out [n_cols][n_bins + 1] or NULL when n_bins == 0.  len_lut[j]: int32 [n_codes[cols[j]]] or NULL.
 * A column may be listed more than once.  1 <= n_bins <= 254 or 0.
 * A code outside [0, n_codes) is NULL, as for rgbm_table_count_codes.  distinct = codes held by at least one row; min_code / max_code
 * = the lowest / highest of them (-1: none); len_sum = sum(rows of code * len_lut[code]), len_max = the largest len_lut entry (>= 0) of
 * an occurring code (both 0 without a LUT).  With m = the column's non-NULL rows: edges[0] = min_code and edges[i] = the smallest
 * code whose cumulative non-NULL row count is >= (i * m + n_bins - 1) / n_bins (integer division); all -1 when m = 0.  The per-code
 * counts stay on the device.  RGBM_ERR_ARG / RGBM_ERR_PARAM: n_cols < 1 or > 65535, a column outside the table, n_bins outside
 * 0, 1..254, edges_out == NULL with n_bins > 0; a refused call leaves the table as it was. */
int rgbm_table_column_stats(const rgbm_table* t, const int32_t* cols, int32_t n_cols, const int32_t* const* len_lut,
                            int32_t n_bins, int64_t* stats_out, int32_t* edges_out);
/* The measures of the functional dependencies X -> Y of one left-hand side X (lhs_cols, 0 .. 11 distinct columns; none: all rows are one
 * group) against n_rhs >= 1 right-hand sides (rhs_cols, distinct, none of them in X) in one call (RepairMisc.discoverFunctionalDeps; the
 * statement is repair.fd_codes.fd_measures).  A code outside [0, n_codes) is NULL, as for rgbm_table_detect_dc, and NULL is a value of its
 * own on both sides.  groups_out [1] = the distinct X-keys; per right-hand side r: kept_out[r] = the sum over the X-groups of the largest
 * number of the group's rows that share one Y value (rows - kept = the fewest rows to remove for X -> Y to hold, the g3 measure);
 * violating_out[r] = the rows in X-groups of two or more Y values; xy_groups_out[r] = the distinct (X, Y) keys.  All integers: the result
 * does not depend on the order of arrival.  A right-hand side whose dense joint table span(X) * (n_codes[Y] + 1) (span = the product of
 * n_codes + 1 over X) fits a workgroup's LDS counters is counted there (route 0), every other one through two hash tables (route 1).
 * No code is written; the table's cell list and cell set stay as they were.
 * RGBM_ERR_ARG: a NULL argument (lhs_cols may be NULL with n_lhs == 0), n_lhs outside 0 .. 11, n_rhs < 1, a column outside the table, a
 * column twice in either list, a right-hand side that is also in X.  RGBM_ERR_PARAM: span(X) of 2^63 or more, a table of 2^31 rows or
 * more.  After either refusal the output arrays and the report below are as they were. */
int rgbm_table_fd_measures(rgbm_table* t, const int32_t* lhs_cols, int32_t n_lhs /* 0..11 */, const int32_t* rhs_cols, int32_t n_rhs /* >= 1 */,
                           int64_t* groups_out /* [1] */, int64_t* kept_out, int64_t* violating_out, int64_t* xy_groups_out /* each [n_rhs] */);
/* The routes the last successful rgbm_table_fd_measures call on the table took (read-only, no device work; for tests that must know their
 * route).  out [n_rhs + 2]: per right-hand side of that call 0 (LDS counters) or 1 (hash tables), then the two limits: the counters of a
 * dense joint table on route 0, the columns of a left-hand side.  n_rhs must be that call's (0 before any call), else RGBM_ERR_ARG.
 * t == NULL with n_rhs == 0 gives the two limits alone and needs no device. */
int rgbm_table_fd_measures_report(const rgbm_table* t, int32_t* out /* [n_rhs + 2] */, int32_t n_rhs);
/* A resident table in ANOTHER CODE SPACE (a kept fit applied to a later table, whose dictionaries are its own: repair/fitted.py; the statement
 * is repair.recode_codes.recode; the reference left it a TODO, python/repair/model.py:1094).  `out` is a new resident table of the
 * same rows and columns with the dictionary sizes n_codes_out.  A cell whose code lies outside [0, n_codes[j]) is NULL (-1) in `out`; under
 * luts[j] == NULL (identity) every other code stays, and n_codes_out[j] must equal n_codes[j]; otherwise the cell holds luts[j][code] --
 * n_codes[j] entries, each in [-1, n_codes_out[j]).  unmapped_out[j] = cells of column j that were not NULL in `t` and are NULL in `out`: exact
 * integers, whatever the order of arrival.  One streaming pass: a LUT of at most the limit below is staged in LDS per workgroup, a larger one
 * is gathered from global memory.
 * `t` is not written; its cell list, cell set and distinct-row view stay as they were.  `out` inherits NO column kinds, column values or
 * multiplicities: the code space changed, the caller sets them.
 * RGBM_ERR_ARG: a NULL argument (unmapped_out may be NULL), n_codes_out[j] < 1, an identity column whose sizes differ, a LUT entry outside its
 * range (the message names the column and the entry; LUTs are dictionary-sized and validated on the host).  RGBM_ERR_PARAM: a table of 2^31
 * rows or more.  After a refusal *out, unmapped_out and the report below are as they were. */
int rgbm_table_recode(const rgbm_table* t, const int32_t* const* luts /* [c]; luts[j] == NULL: identity */,
                      const int32_t* n_codes_out /* [c] */, rgbm_table** out, int64_t* unmapped_out /* [c] or NULL */);
/* The route of each column of the last successful rgbm_table_recode call on the table (read-only, no device work; for tests that must know
 * their route): out [c + 1] = per column 0 (identity copy), 1 (LDS LUT) or 2 (global LUT) -- -1 before any call --, then the largest LUT that
 * is staged in LDS.  c must be the table's columns, else RGBM_ERR_ARG.  t == NULL with c == 0 gives the limit alone and needs no device. */
int rgbm_table_recode_report(const rgbm_table* t, int32_t* out /* [c + 1] */, int32_t c);
/* Encoding on the device (replaces the pandas encoders of python/repair/model.py:701-729): per column, Arrow-style
 * dictionary indices (idx < 0 = NULL) are mapped through remap[col][idx] (the rank of the dictionary value in
 * sorted order, or -1) into the code table. */
int rgbm_table_create_dict(const int32_t* idx_colmajor, int64_t n, int32_t c, const int32_t* const* remap,
                           const int32_t* dict_size /* [c] */, int32_t device_id, rgbm_table** out);
/* Candidate distributions of the NULL cells of one target attribute (python/repair/model.py:1196-1212): for every row
 * whose target cell is NULL (ascending), the model's classes by descending probability (ties keep class order), those
 * with prob > threshold, at most top_k; class_out is padded with -1, prob_out with 0.  cur_code (optional, per cell: the
 * code the cell held before it was NULLed, -1 = none) -> cur_prob_out = the model's probability of that value.
 * More cells than `cap` is an error that still reports the count in n_cells_out (call again with enough room). */
int rgbm_table_repair_pmf(rgbm_table* t, const rgbm_model* m, int32_t target_col, const int32_t* feat_cols, int32_t f,
                          int32_t top_k, double threshold, const int32_t* cur_code, int64_t cap, int64_t* n_cells_out,
                          int64_t* rows_out /* [cap] */, int32_t* class_out /* [cap][top_k] */,
                          double* prob_out /* [cap][top_k] */, double* cur_prob_out /* [cap] or NULL */);
/* The same with the update costs of the probability modes (python/repair/model.py `_compute_repair_pmf` / `_compute_score`;
 * reference model.py:1145-1165 `_compute_weighted_probs`, 1167-1212, 1223-1277).  Per NULL cell, in the order of the Python loop:
 *   p_c = p_c * (1.0 / (1.0 + weight * cost[cost_row[cell]][c]))  for cost_row[cell] >= 0 and a cost that is not NaN (NaN = None);
 *   renormalise != 0: p_c = p_c / norm when norm = p_0 + p_1 + ... (sequential, in class order) > 0;
 *   cur_prob_out = p[cur_code] (0.0 when cur_code is -1 / not a class), then the stable top-k of rgbm_table_repair_pmf;
 *   top1_cost_out = cost[base][top-1 class], base = cost_row[cell] when >= 0 else the self row n_cost_rows; NaN without a top-1.
 * cost: [n_cost_rows + 1][K] row-major (K = the model's classes; the last row holds the cost of each class against itself), at most
 * 2^28 entries; NULL = no costs (cost_row must then be NULL too).  cost_row: per cell, -1 = leave the cell's probabilities alone.
 * With cost = NULL and renormalise = 0 the outputs are those of rgbm_table_repair_pmf, bit for bit. */
int rgbm_table_repair_pmf_weighted(rgbm_table* t, const rgbm_model* m, int32_t target_col, const int32_t* feat_cols, int32_t f,
                                   int32_t top_k, double threshold, const int32_t* cur_code /* [cells] or NULL */,
                                   const int32_t* cost_row /* [cells] or NULL */, const double* cost /* [n_cost_rows + 1][K] or NULL */,
                                   int64_t n_cost_rows, double weight, int32_t renormalise, int64_t cap, int64_t* n_cells_out,
                                   int64_t* rows_out /* [cap] */, int32_t* class_out /* [cap][top_k] */, double* prob_out /* [cap][top_k] */,
                                   double* cur_prob_out /* [cap] or NULL */, double* top1_cost_out /* [cap] or NULL */);
/* Levenshtein distances (insert / delete / substitute, unit costs) of every pair of two string pools: the `Levenshtein` update
 * cost (python/repair/costs.py; reference costs.py:50-58, used by model.py:1145-1165 and 1223-1240).  Strings are int32 Unicode
 * code points, string i of a pool is cp[off[i] .. off[i + 1]) (off[0] = 0, non-decreasing, n + 1 entries).
 * dist_out: [n_a][n_b] row-major, host memory.  Strings of any length; both pools are copied to device `device_id`. */
int rgbm_edit_distance(int32_t device_id, const int32_t* a_cp, const int64_t* a_off, int64_t n_a, const int32_t* b_cp,
                       const int64_t* b_off, int64_t n_b, int32_t* dist_out);
/* ---- cell-domain analysis and weak labels (python/repair/errors.py:488-578; the value-space statement is repair/domain.py) ----
 * Dense joint counts of column pairs in one pass over the rows (RepairApi.computeFreqStats, src/main/scala/.../python/RepairApi.scala:231-273,
 * GROUPING SETS over (x, y); and the exact stand-in for approx_count_distinct(struct(x, y)) of computeAttrStats, :429-448).
 * pair_cols [n_pairs][2]; n_bins[col] = bins of a column of the discretised view (RepairApi.discretizeTable, :126-149); luts[col] (or luts
 * itself) NULL = the codes are the bins, else int32 [n_codes[col]] code -> bin.  A code / bin outside its range counts as NULL.
 * counts_out: the pairs' tables one after the other, pair (x, y) as int64 [(n_bins[x] + 1)][(n_bins[y] + 1)] row-major with NULL in the last
 * slot of each side.  More than 2^24 dense cells in a pair or 2^25 in a call: RGBM_ERR_PARAM (count sparsely on the host).
 * The tables, bins and LUTs stay with the table (device memory) for rgbm_table_cell_domains until the next call.
 * RGBM_ERR_ARG: a NULL argument other than luts, n_pairs < 1.  RGBM_ERR_PARAM, the previous result untouched: a column outside the table, a pair
 * (x, x), n_bins < 1 for a column of a pair, the two cell limits above. */
int rgbm_table_pair_counts(rgbm_table* t, const int32_t* pair_cols, int32_t n_pairs, const int32_t* const* luts /* [c] or NULL */,
                           const int32_t* n_bins /* [c] */, int64_t* counts_out);
/* The plan the last successful rgbm_table_pair_counts call on the table took (read-only, no device work; for tests that must know their
 * route).  The pairs are packed, in the given order, into groups whose counters share a workgroup's LDS; a group is closed when its counters
 * or its distinct columns would exceed a limit; a pair above the counter limit on its own is counted by a second kernel straight in HBM.
 * pairs_out [n_pairs][3]: {group (-1 = the HBM kernel), slot of x, slot of y among the group's staged columns (-1, -1 with the HBM kernel)}.
 * head_out [6]: {groups, counters of the largest group, workgroups per group (grid x), rows per workgroup -- all 0 when no pair took a
 * group --, the limit of a group's counters, the limit of a group's distinct columns}.  n_pairs must be that call's (0 before any call), else
 * RGBM_ERR_ARG.  t == NULL with n_pairs == 0 gives the two limits alone and needs no device. */
int rgbm_table_pair_counts_report(const rgbm_table* t, int64_t* head_out /* [6] */, int32_t* pairs_out /* [n_pairs][3] */, int32_t n_pairs);
/* Domains of the error cells of ONE discrete target with the naive-Bayes posterior of RepairApi.computeDomainInErrorCells (:479-675)
 * and the weak-label rule of errors.py:517-521, on the tables the last rgbm_table_pair_counts left on the device.  rows: the cells' row
 * positions; pair_idx [k <= 8]: the pairs (of that call) holding the target and its correlated attributes, in order; an element (value c of
 * the target) exists for attribute j iff cnt > min_cnt[j] and carries max(cnt - 1, 0.1); an attribute without elements for the cell (its
 * value is NULL / no group) wipes the attributes before it (the SQL's IF(ISNOTNULL(domain), CONCAT(domain, d), d));
 * score_c = sum over the attributes, in order, of element / row_count (0 where single_ok[c] == 0), prob_c = score_c / (score_0 + score_1 + ...).
 * top_out: the value of the largest prob > beta (ties: smallest code), -1 = none; weak_out: the cell holds exactly that value now.
 * probs_out [n_cells][n_bins[target]] is optional.  A row outside the table has an empty domain (top -1, probability 0, not weak); a
 * current code outside the target's bins counts as NULL.
 * RGBM_ERR_ARG: the target outside the table, n_cells < 0, k < 0, row_count < 1, a NULL array that is needed.  RGBM_ERR_PARAM: k > 8, no
 * rgbm_table_pair_counts result on the table, a target that was counted through a LUT, a pair index outside that call's pairs, a pair
 * that does not hold the target. */
int rgbm_table_cell_domains(rgbm_table* t, int32_t target_col, const int64_t* rows, int64_t n_cells, const int32_t* pair_idx, int32_t k,
                            const int64_t* min_cnt /* [k] */, const uint8_t* single_ok /* [n_bins[target]] */, double beta, int64_t row_count,
                            uint8_t* weak_out, int32_t* top_out, double* top_prob_out, double* probs_out /* or NULL */);
/* ---- rule-based repairs (python/repair/model.py `_build_rule_model`, `_repair`, `_repair_by_nearest_values`) ----
 * The rule model of a functional dependency x -> y (reference model.py:928-953, `FunctionalDepModel` :64-100): over the rows where both
 * cells are non-NULL, map_out[x] is the single y code that x occurs with; -1 when x occurs with two or more y codes, or with none. */
int rgbm_table_fd_map(const rgbm_table* t, int32_t x_col, int32_t y_col, int32_t* map_out /* [n_codes[x_col]] */);
/* One rule step of the chained repair on rows [row_begin, row_begin + n_rows) (reference model.py:1107-1133 with `FunctionalDepModel.predict`
 * :83-84 or `PoorModel.predict` :55-56):  pred = x_col < 0 ? lut[0] : (x >= 0 && x < n_lut ? lut[x] : -1).  out_label gets pred for every
 * row; a NULL y cell receives pred and stays NULL when pred is -1, so the later models of the chain see it as missing (predict gave None).
 * lut entries are -1 or codes of y_col. */
int rgbm_table_rule_fill(rgbm_table* t, int32_t y_col, int32_t x_col /* -1: constant */, const int32_t* lut, int32_t n_lut, int64_t row_begin,
                         int64_t n_rows, int32_t* out_label /* [n_rows] or NULL */);
/* Nearest-value merges (reference model.py:1279-1291 `_repair_by_nearest_values`): for every string of pool a the position in pool b of the
 * closest string when its cost is <= threshold and strictly below every other cost of the row, else -1.  cost == NULL: the costs are the
 * Levenshtein distances of the pools (layout as in rgbm_edit_distance; the [n_a][n_b] matrix never leaves the device).  Otherwise cost is
 * [n_a][n_b] row-major, NaN = the pair has no cost and does not take part, and the pools are not read.  At most 2^30 entries; n_b == 0 gives
 * -1 everywhere. */
int rgbm_nearest_values(int32_t device_id, const int32_t* a_cp, const int64_t* a_off, int64_t n_a, const int32_t* b_cp, const int64_t* b_off,
                        int64_t n_b, const double* cost /* [n_a][n_b] or NULL */, double threshold, int32_t* nearest_out /* [n_a] */);
/* ---- regex-structure repair (RegexStructureRepair.scala, RepairApi.repairByRegularExpression :677-704; the statement is
 * repair/regex_structure.py) ----
 * The structure of a detector's regex as a program of 1 .. 32 segments, matched with the meaning of `findFirstMatchIn` on the derived regex
 * (leftmost start, every segment greedy, first successful backtracking path) against every string of a pool (layout as in
 * rgbm_edit_distance).  A capture takes min .. max (max -1: unbounded; both at most 65535) code points of its class; a constant takes 1 .. its
 * length code points other than U+000A, U+000D, U+0085, U+2028, U+2029 (min = 1 and max = const_len say so).  anchors: bit 0 `^` (the match
 * starts at position 0), bit 1 `$` (it ends at the string's end).  A string that matches is rewritten as its captures and the constants'
 * texts in segment order: state 1, the repaired strings back to back in out_cp with out_off[i + 1] - out_off[i] code points (0 for the
 * other states).  A string of up to 63 code points is matched by one lane (its positions are one 64-bit word), one of up to
 * RGBM_RX_WAVE_MAX_CP by one wave; a longer one gets state 2 and is the caller's (the statement) to evaluate.
 * RGBM_ERR_ARG: a NULL array that is needed, n_segs outside 1 .. 32, anchors outside 0 .. 3, a kind other than 0 / 1, capture bounds outside
 * 0 <= min <= max <= 65535, a constant outside const_cp or with bounds other than 1 .. const_len, constants that overlap (their lengths sum
 * to more than n_const_cp), off[0] != 0, offsets that decrease.  n == 0 is legal. */
#define RGBM_RX_WAVE_MAX_CP 4095 /* positions 0 .. 4095 of the longest string: 64 per lane of one wave */
typedef struct { int32_t kind /* 0 capture, 1 constant */, min, max /* -1 unbounded; constant: 1, length */;
                 uint32_t cls[4] /* capture: bit c = ASCII code point c is in the class */;
                 int32_t const_off, const_len /* constant: its text in const_cp */; } rgbm_rx_seg;
int rgbm_regex_structure(int32_t device_id, const rgbm_rx_seg* segs, int32_t n_segs /* 1..32 */, int32_t anchors,
                         const int32_t* const_cp, int32_t n_const_cp,
                         const int32_t* cp, const int64_t* off, int64_t n,
                         uint8_t* state_out /* [n]: 0 no match, 1 repaired, 2 longer than the device handles */,
                         int64_t* out_off /* [n + 1] */,
                         int32_t* out_cp /* capacity off[n] + n * n_const_cp */,
                         int64_t* info_out /* [4] = {strings on the one-word route, on the wave route, state 2, repaired} */);
/* ---- LOF in code space (LOFOutlierErrorDetector: scikit-learn's LocalOutlierFactor(novelty=False) on one attribute; repair/lof_codes.py) ----
 * The local outlier factor of every entry of a sorted dictionary: values [d] ascending and finite, counts [d] >= 1 rows per entry (two rows
 * in all at least), k_ = max(1, min(k, rows - 1)) neighbours.  The neighbours of an entry are min(count - 1, k_) copies of itself, then the
 * nearest entries outward by |v_c - v_j|, each whole until k_ is reached and the last one partially; two candidates at one distance of which
 * only one fits are a TIE, resolved to the left and counted.  score = the factor (the negated negative_outlier_factor_), float64, sums over
 * the window's entries in ascending order; bit c of flag_bits_out is set when -score < -threshold.  info_out = {entries with a tie, entries
 * with |score - threshold| <= threshold * 2^-40}.  RGBM_ERR_ARG: d < 1, k outside 1 .. 64, a count < 1, fewer than two rows in all, values
 * that are not ascending or not finite. */
int rgbm_lof_1d(int32_t device_id, const double* values /* [d], ascending, finite */, const int64_t* counts /* [d], >= 1 */,
                int32_t d, int32_t k /* 1..64 */, double threshold /* 1.5 */,
                double* score_out /* [d] or NULL */, uint64_t* flag_bits_out /* [ceil(d/64)] */, int64_t* info_out /* [2] = {n_ties, n_near} */);
/* ---- q-gram k-means in code space (RepairMisc.splitInputTable; reference RepairMiscApi.scala:52-153; repair/qgram_kmeans.py) ----
 * One Lloyd assignment step over the resident table.  cols [n_cols <= 1024]: the attributes, code_off[j]: where the dictionary of cols[j]
 * starts among the d_tot dictionary entries of all of them.  p: [d_tot][k] row-major float64 (-2 E C^T), h: [k] (|C_k|^2).  The score of
 * a row for cluster kk is the float64 sum, in this order,  h[kk] + p[code_off[0] + code_0][kk] + p[code_off[1] + code_1][kk] + ...  (a code
 * outside [0, n_codes) is NULL and adds nothing); its label is the lowest kk with the least score.  counts_out[kk][e] = rows of cluster kk
 * holding dictionary entry e, sizes_out[kk] = rows of cluster kk, n_changed_out = rows whose label differs from the previous call's (all
 * rows with first != 0).  The labels (int32 per row) stay with the table on the device; rgbm_table_kmeans_read copies them out.
 * RGBM_ERR_PARAM, the previous labels untouched: k outside 2 .. 64, n_cols outside 1 .. 1024, a column outside the table, d_tot * k outside
 * 1 .. 2^27, code_off[j] < 0 or code_off[j] + n_codes[cols[j]] > d_tot, first == 0 without previous labels (rgbm_table_kmeans_read: no labels). */
int rgbm_table_kmeans_assign(rgbm_table* t, const int32_t* cols, int32_t n_cols, const int64_t* code_off /* [n_cols] */,
                             int32_t k, const double* p /* [d_tot][k] */, int64_t d_tot, const double* h /* [k] */,
                             int32_t first /* 1: there is no previous assignment */,
                             int64_t* counts_out /* [k][d_tot] */, int64_t* sizes_out /* [k] */, int64_t* n_changed_out);
/* One pass of a level of the bisecting k-means (clustering_alg = "bisecting"; repair/qgram_bisect.py) on the same resident labels.
 * A label names a tree node; slot_of[label] is the slot s (0 .. m - 1) of the node this level splits, for the node itself and for its two
 * children, or -1.  p: [d_tot][2m], h: [2m], columns 2s and 2s + 1 = the left and right child of slot s.  A row of slot s is scored against
 * these two only:  s0 = h[2s] + p[code_off[0] + code_0][2s] + ...,  s1 the same at 2s + 1 (float64, in this order, NULL adds nothing); its
 * label becomes child[2s + 1] iff s1 < s0, else child[2s].  A row whose label lies outside [0, n_nodes) or has slot_of == -1 keeps its label
 * and is counted nowhere.  first != 0: there are no labels yet, every row is node 0.  counts_out[2s + side][e] / sizes_out[2s + side]: the
 * rows of that child (holding dictionary entry e); n_changed_out: the scored rows whose label differs from before the pass.
 * RGBM_ERR_PARAM, the previous labels untouched: m outside 1 .. 512, n_nodes outside 1 .. 2048, n_cols outside 1 .. 1024, a column outside
 * the table, d_tot * 2m outside 1 .. 2^27, code_off as above, a slot_of entry outside -1 .. m - 1, a child entry outside 0 .. n_nodes - 1,
 * first == 0 without labels. */
int rgbm_table_kmeans_bisect(rgbm_table* t, const int32_t* cols, int32_t n_cols, const int64_t* code_off /* [n_cols] */, int64_t d_tot,
                             const int32_t* slot_of /* [n_nodes] */, int32_t n_nodes, int32_t m, const int32_t* child /* [2m] */,
                             const double* p /* [d_tot][2m] */, const double* h /* [2m] */, int32_t first,
                             int64_t* counts_out /* [2m][d_tot] */, int64_t* sizes_out /* [2m] */, int64_t* n_changed_out);
int rgbm_table_kmeans_read(const rgbm_table* t, int32_t* assign_out /* [n] */);
int rgbm_table_shape(const rgbm_table* t, int64_t* n_out, int32_t* c_out, int32_t* n_codes_out /* [c] or NULL */);

/* ---- row-sharded multi-GPU training ------------------------------------------------------------
 * The reference parallelises training per target attribute (python/repair/model.py:817-926); a single
 * multiclass target cannot be split that way.  Here every rank (one process per GPU) uploads a ROW SHARD
 * of the table with rgbm_table_create and calls rgbm_table_train for the same targets in the same
 * order; inside, the code counts, the per-level histograms and the child row counts are summed with
 * integer all-reduces (RCCL over xGMI, enqueued on the training stream).  All sums are exact integers,
 * so every rank ends with the same model, bit-identical to single-GPU training on the whole table.
 * The communicator belongs to the calling thread.  Level grower only, no per-row weights; bagging draws per global training-row
 * position (the shards must hold consecutive row ranges in rank order), so the model is the single-device one. */
#define RGBM_COMM_ID_BYTES 128
#define RGBM_FLAG_ROW_SHARDED 1 /* rgbm_params.reserved: this call is one rank of a row-sharded training */
#define RGBM_FLAG_WHOLE_TABLE 4 /* rgbm_params.reserved, rgbm_table_train: train on every row, never on the table's distinct-row view (same model) */
#define RGBM_FLAG_NO_MODEL 2    /* rgbm_params.reserved, rgbm_table_train_batch only: the fit is wanted for its validation scores (a CV fold); no model
                                   is built, out_models[i] stays NULL with status RGBM_OK */
int rgbm_comm_unique_id(void* id_out /* [RGBM_COMM_ID_BYTES], call on one rank, hand to all */);
int rgbm_comm_init(const void* id, int32_t rank, int32_t nranks, int32_t device_id);
int rgbm_comm_finalize(void);
int rgbm_comm_info(int32_t* info /* [3] = {0 none | 1 RCCL | 2 thread group | 3 member of a fusion group, rank, nranks} */);
int rgbm_comm_count(int32_t* n_out /* ranks the communicator really spans (ncclCommCount); 1 without one */);
/* Test transport: the ranks are host threads of one process sharing one device. */
/* ---- C1 / C2 of a multi-GPU job on THIS communicator (device buffers, ncclAllGather over xGMI; a rank holds one RCCL communicator) -------
 * Replace `sparkContext.broadcast(models)` (python/repair/model.py:1069: every worker gets every serialised model) and the union of the
 * grouped-map UDF outputs (model.py:1142: the repaired cells of all row groups).  Blocks are equal-sized: callers exchange their sizes with
 * rgbm_comm_all_gather_sizes first and pad to the largest.  Thread group / no communicator: the same calls, device copies.  Not from inside a
 * fusion group. */
int rgbm_comm_all_gather_sizes(const int64_t* mine, int32_t n, int64_t* all /* [nranks][n] */);
int rgbm_comm_all_gather_bytes(const void* send, int64_t my_bytes, int64_t block_bytes /* >= every rank's my_bytes */, void* recv /* [nranks][block_bytes] */);
/* rgbm_table_repair_chain of this rank's rows with the outputs left on the device, all-gathered there and copied out once:
 * out_label / out_prob [nranks][T][max_rows] (a rank's block: its n_rows rows of every model, zero-padded to max_rows). */
int rgbm_table_repair_chain_gather(rgbm_table* t, const rgbm_model* const* models, int32_t T, const int32_t* target_col,
                                   const int32_t* feat_cols, const int32_t* feat_off, int64_t row_begin, int64_t n_rows, int64_t max_rows,
                                   int32_t* out_label, double* out_prob);
int rgbm_comm_gather_stats(int64_t* out /* [3] = {bytes received, nanoseconds, collectives} of this process's all-gathers */);
int rgbm_local_group_create(int32_t nranks, int32_t device_id, void** group_out);
void rgbm_local_group_free(void* group);
int rgbm_comm_init_local(void* group, int32_t rank);

/* Fusion group: the row-sharded training calls a rank makes AT THE SAME TIME (one host thread + one stream each; the reference trains its
 * targets in parallel, python/repair/model.py:817-926).  The calling thread's communicator moves into the group; every member thread joins
 * with its index (the same indices on every rank), trains its targets with RGBM_FLAG_ROW_SHARDED as usual and leaves.  Inside, the i-th
 * collective of every member still taking part is carried by ONE all-reduce per element type of the rank's communicator over the members'
 * buffers laid side by side (member order): a rank issues 8 collectives per boosting iteration of ALL its row-sharded targets instead of 8
 * per target, and the targets overlap on the device.  Models are unchanged (integer sums).  A member that fails breaks the group: the other
 * members' calls fail at their next collective.  rgbm_fusion_free hands the communicator back to the calling thread. */
int rgbm_fusion_create(int32_t n_members, void** fusion_out);
int rgbm_fusion_join(void* fusion, int32_t member /* 0 .. n_members-1, on the member's own thread */);
int rgbm_fusion_leave(int32_t failed /* 0: done; 1: this member failed -- the group is broken */);
int rgbm_fusion_info(void* fusion, int64_t* info /* [4] = {collectives issued, member parts carried, members still in, broken} */);
int rgbm_fusion_free(void* fusion);

/* ---- model handle: pickling (python/repair/model.py:910,921,1069) -------------------------- */
int rgbm_model_save(const rgbm_model* m, void* buf, size_t* len); /* buf==NULL: length query */
int rgbm_model_load(const void* buf, size_t len, rgbm_model** out);
void rgbm_model_free(rgbm_model* m);
/* info[5] = {objective, num_class, trees_per_iteration, n_iterations, n_features} */
int rgbm_model_info(const rgbm_model* m, int32_t* info);
/* The kernel the predictor runs for this model: out[5] = {form, mask words per tree entry (1: <= 32 leaves, 2: <= 64), padded mask words
 * per tree (fixed form; else 0), trees per LDS stage, LDS bytes of a workgroup}.  form 0 = fixed-stride bit-vector scorer, 1 =
 * dynamic-stride scorer, 2 = walk over index-linked nodes (the other entries are 0).  A function of the model and of the environment
 * switches RGBM_QS_FIXED=0 / RGBM_PREDICTOR=walk alone: it needs no device, and the predictor launches from the same rule. */
int rgbm_model_predict_form(const rgbm_model* m, int32_t* out);
/* The launch plan of the level grower's passes for a table of n_rows rows and f features with nbins[j] bins (1..256) each, k class trees and
 * max_depth (1..7); with_mult: the rows carry multiplicities.  A function of these and of the environment switches (RGBM_LV_BLOCKS, RGBM_MT_BLOCKS,
 * RGBM_MT_TREES, RGBM_LV_LDS, ...) alone: it needs no device, and the trainer launches from the same rule.  out (doubles, whole numbers but for the times):
 *   [0..5]  root pass: row blocks per class tree (gx), nodes of the largest set of workgroup partials (part_items), level-pass launches L, workgroups,
 *           modelled fixed time of a workgroup (us), modelled row-loop time of a workgroup (us);
 *   then per level-pass launch, in launch order, 12 values: level, chunk, first built slot, built slots, routing launch?, class trees per workgroup (T),
 *           class tree groups (G), row blocks (gx), both-chunk form?, rotated?, modelled fixed time (us), modelled row-loop time of a workgroup (us).
 * *n_out = values the plan has (6 + 12 L); RGBM_ERR_ARG when out_len is smaller.  A feature set that the training call would refuse (the
 * histograms of one node exceed the LDS) fails here the same way. */
int rgbm_level_pass_plan(const int32_t* nbins, int32_t f, int64_t n_rows, int32_t k, int32_t max_depth, int32_t with_mult, double* out, int32_t out_len, int32_t* n_out);
/* LightGBM feature_importances_ (train.py:219): type 0 = split counts, 1 = total gain. */
int rgbm_model_importance(const rgbm_model* m, int32_t type, double* out /* [n_features] */);

#ifdef __cplusplus
}
#endif
#endif /* RGBM_H_ */
