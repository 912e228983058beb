/*
 * vbq.h -- C-ABI of the MI355X-native VBQ hot path (libvbq_hip.so).
 *
 * Boundary rules
 *   - plain `extern "C"` functions, plain pointers and sizes; no torch / C++ types.
 *   - every pointer named `d_*` is DEVICE memory (borrowed; e.g. tensor.data_ptr() of a
 *     PyTorch-ROCm tensor), every pointer named `h_*` is HOST memory.
 *   - all work is enqueued on the caller's `stream` (a hipStream_t passed as void*;
 *     NULL = the default stream) and returns without synchronising; nothing is
 *     allocated inside a call -- scratch comes from a caller-provided workspace.
 *   - return value: 0 = ok, negative = VBQ_ERR_*; vbq_last_error() gives the text of
 *     the calling thread's most recent failure.
 *   - no global state besides that thread-local error string (launch policies are per-call arguments, never environment
 *     presets; the one variable read is the test-only VBQ_FAST_DEBUG, see "Launch policy").
 *
 * The reference (mandt-lab/vbq) has no FFI of its own: the boundary it offers is the
 * Python call surface listed in SURVEY.md 8(b).  Each entry point below names the
 * reference code it replaces; INTEGRATION.md shows the ctypes binding a maintainer of
 * the reference would add.
 *
 * Table layout ("level-major"), shared by every entry point that takes `d_table_lm`:
 *   float table[C][T], T = 2^(N+1)-1; the 2^n code points of bit length n occupy slots
 *   [2^n-1, 2^(n+1)-1) in increasing order.  This is exactly
 *   ChannelwisePriorCDFQuantizer.all_code_points (img-compression/quantizer.py:30-36)
 *   and the notebook's `codepoints` (word-embeddings/...ipynb:383-389).
 * Quantization index ("rank index"), produced / consumed as uint16:
 *   slot (n, i) has rank k = (2i+1) * 2^(N-n) in the merged sorted table; the index is
 *   k-1, i.e. the position in `code_points_by_channel` (quantizer.py:37) -- the value
 *   the reference calls `qidx` / `I` (quantizer.py:135,223) whenever the sorted table
 *   is strictly increasing.  Bit length of index q is N - ctz(q+1).
 * Element layout:
 *   VBQ_LAYOUT_BC  channel-last  [n_rows][n_ch]   (quantizer.py:90-91,196-197)
 *   VBQ_LAYOUT_CB  channel-major [n_ch][n_rows]   (the reference's own C x B view, :73)
 *   Outputs with a lambda axis are [n_lambda][...same layout as the input...].
 */
#ifndef VBQ_H_
#define VBQ_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VBQ_ABI_VERSION 5

enum {
    VBQ_OK = 0,
    VBQ_ERR_INVALID_ARGUMENT = -1,
    VBQ_ERR_UNSUPPORTED = -2,
    VBQ_ERR_LAUNCH = -3,
    VBQ_ERR_WORKSPACE = -4
};
/* Refusals.  A call that returns VBQ_ERR_INVALID_ARGUMENT, VBQ_ERR_UNSUPPORTED or VBQ_ERR_WORKSPACE has enqueued nothing:
 * outputs, outputs that are "ADDED to", status words and the workspace hold what they held, whichever of the lambdas, the bit
 * depth or an inner step of a composite call the refusal is about.  VBQ_ERR_LAUNCH is a failure of the runtime in mid-call
 * and is exempt: work enqueued before it stays enqueued. */
/* Buffers.  Every pointer parameter that is not `const` names memory the call writes, of the size and type its comment
 * states, densely laid out.  Such a buffer must not overlap anything else the call reads or writes -- an input, another output,
 * the workspace -- unless the function's comment says so: the kernels read through `__restrict__` pointers and work in tiles,
 * so an overlap gives a silently wrong answer.  What a comment allows is always the buffer's OWN earlier content: state that is
 * updated in place, counts and totals that are ADDED to, status words that are OR-ed into, slots that keep what they held.  The
 * library cannot check any of this cheaply and does not; the Python binding does (vbq_amd/ops.py, _out), and
 * tests/written_buffers.py lists every such parameter with the way a caller reaches it.  The same holds for vbq_ext.h,
 * vbq_budget.h, vbq_kmeans.h and vbq_store.h. */

enum {
    VBQ_LAYOUT_BC = 0,
    VBQ_LAYOUT_CB = 1,
    /* vbq_quantize_f32 only: inputs channel-last [n_rows][n_ch] as the latents arrive, outputs channel-major
     * planes [n_lambda][n_ch][n_rows] -- the solve without the two input transposes (VBQ_MODE_F32; three or more
     * lambdas must lie in the fast kernel's range [1.9e-12, 1.8e19], otherwise VBQ_ERR_UNSUPPORTED; one or two
     * lambdas take the pruned descent, which accepts any value). */
    VBQ_LAYOUT_BC_TO_CB = 2
};

/* Tie-break / arithmetic of the solve. */
enum {
    /* TF-eager path of the image pipeline: every op rounded to f32, candidate order
     * [L_0..L_N, R_1..R_N], first maximum wins (utils.py:319-320,388-401;
     * quantizer.py:183). */
    VBQ_MODE_F32 = 0,
    /* NumPy backend exactly as written: f32 distortion, lambda*len and the score in
     * f64 (utils.py:388 leaves integer lengths uncast for backend=np). */
    VBQ_MODE_F64_SCORE = 1
};

int vbq_abi_version(void);
const char *vbq_last_error(void);

/* Launch policy: `reserved_workgroups` (vbq_quantize_rows_f32, vbq_level_counts_f32, vbq_build_entropy_models_f32).
 * For builds that overlap a collective with the kernels (the rank histogram's all-reduce of step i runs while step
 * i + 1 computes).  The solve kernels run as RESIDENT grids sized to every workgroup slot of the chip; a collective's kernel (RCCL:
 * a few dozen workgroups) takes some of those slots, and a resident workgroup that finds its slot taken starts only after another
 * one has finished all its iterations -- up to twice the kernel time.  With n > 0 the grids of THAT CALL are sized to (slots - n), or
 * launched as short-lived workgroups when the (workgroups x channels) grid shape would give up more than a tenth of the chip.
 * n = 0: every slot; a negative n is taken as 0.  A per-call argument: the library keeps no mutable launch state, two builds
 * with different policies may run side by side, and no environment variable changes which kernel or grid a call takes.  The one
 * variable the library reads is VBQ_FAST_DEBUG (tests only, read once): 1 sends every solve of the fast kernels through the
 * literal scan, 2 switches their near-tie flags off; the kernels and grids stay the same. */

/* The launch shape a solve call would take on the current device -- nothing is launched: h_grid (HOST, int64 [3]) = { workgroups
 * per channel, channels, 1 when every workgroup is resident from start to end (0: short-lived workgroups) } for
 * VBQ_GRID_K1 (the fused per-lambda kernel of vbq_quantize_rows_f32) / VBQ_GRID_K1T (the threshold kernel of vbq_level_counts_f32)
 * on n_rows rows per channel.  A pure function of its arguments and the device's CU count: what makes the launch policy testable. */
enum { VBQ_GRID_K1 = 0, VBQ_GRID_K1T = 1 };
int vbq_solve_grid(int32_t kernel, int64_t n_rows, int32_t n_ch, int32_t workgroups_per_cu, int32_t reserved_workgroups,
                   int64_t *h_grid);

/* Number of GPUs visible / name of device `dev` (for harness output only). */
int vbq_device_count(void);
int vbq_device_name(int dev, char *buf, size_t buflen);

/* ----------------------------------------------------------------------------------
 * K1  R-D solve.  Replaces, in one pass over (mu, sigma):
 *       ChannelwisePriorCDFQuantizer.get_all_N_bit_intervals   quantizer.py:65-80
 *       ChannelwisePriorCDFQuantizer.compress_batch_channel_latents  quantizer.py:156-188
 *       utils.curry_normal_logpdf(ignore_const=True)           utils.py:307-321
 *       utils.batch_quantize_indep_dims                        utils.py:363-423
 *       the qidx lookup                                        quantizer.py:135,223
 *     for all `n_lambda` trade-offs at once (the reference also shares the distortions
 *     across lambdas, utils.py:387,392).
 *
 *   d_mu, d_sigma   f32, n_rows*n_ch elements in `layout`; sigma > 0, all finite.
 *   d_table_lm      f32 [n_ch][T] level-major, non-decreasing in xi for every channel.
 *   d_level_len     f32 [n_lambda][n_ch][N+1] code length of bit-level n (the
 *                   "n + overhead" of quantizer.py:171-175), or NULL for the raw
 *                   lengths n (quantizer.py:167-169).  Lengths are non-negative; when some
 *                   lambda*len falls outside {0} U [2^-39, 2^70] the solve detects it on the
 *                   device and takes its literal (slower) scan, with the same answers.
 *   h_lambdas       HOST doubles [n_lambda]; VBQ_MODE_F32 rounds each to f32 first
 *                   (TF casts the Python scalar to the tensor dtype).
 *   d_out_idx       u16 [n_lambda][n_rows*n_ch] rank index of the winner.
 *   d_out_zhat      optional f32, same shape: the winning code point (Z_hat).
 *   d_out_bits      optional f32, same shape: its code length (num_bits).
 *   d_workspace     vbq_quantize_workspace_bytes() bytes of device scratch.
 *   Which kernel serves a call is an implementation detail (same answers): one or two lambdas with indices as the only
 *   output take a descent that stops as soon as no deeper bit level can win (literal comparisons only: any lambda, any
 *   lengths); sweeps of 16-32 lambdas with raw lengths are solved from ten thresholds per element; everything else by
 *   the fused per-lambda kernel.
 *   N               max_bits_per_coord; kernels are built for 4 <= N <= 12 (the reference uses 10,
 *                   post_process.py:117); N = 11, 12 for channel-major planes / one code book only
 *                   (16 channel tables no longer fit the LDS); the notebook solve and the coder stop at
 *                   10.  Other values return VBQ_ERR_UNSUPPORTED.
 * ---------------------------------------------------------------------------------- */
size_t vbq_quantize_workspace_bytes(int32_t n_ch, int32_t n_lambda, int32_t N);

/* The solve's precondition, checkable: d_bad[0] += #{mu not finite}, d_bad[1] += #{sigma not finite or <= 0} (u32[2],
 * device, zero it first).  The reference lets such values flow through tf.argmax (NaN scores, whatever index results);
 * here they are outside the contract of vbq_quantize_f32, and this is how a caller finds out beforehand. */
int vbq_check_inputs_f32(const float *d_mu, const float *d_sigma, int64_t n, uint32_t *d_bad, void *stream);

int vbq_quantize_f32(const float *d_mu, const float *d_sigma, int64_t n_rows, int32_t n_ch,
                     int32_t layout, const float *d_table_lm, const float *d_level_len,
                     const double *h_lambdas, int32_t n_lambda, int32_t N, int32_t mode,
                     uint16_t *d_out_idx, float *d_out_zhat, float *d_out_bits,
                     void *d_workspace, size_t workspace_bytes, void *stream);

/* ChannelwisePriorCDFQuantizer.get_all_N_bit_intervals (quantizer.py:65-80) as a result of its own (API compatibility; the
 * solve never materialises it): d_left / d_right f32 [n_ch][N+1][n_rows] = the left / right n-bit neighbours of every
 * z on every level, edge padding of the per-level grids included (:54-57,75-76).  d_z_cb: planes [n_ch][n_rows]. */
int vbq_n_bit_intervals_f32(const float *d_z_cb, int64_t n_rows, int32_t n_ch, const float *d_table_lm, int32_t N,
                            float *d_left, float *d_right, void *stream);

/* The same solve on rows [row_begin, row_end) of the full arrays (pointers, n_rows and output addressing are those
 * of the whole tensor): lets the caller cut one pass into chunks and run K2 on chunk j (another stream) while K1
 * works on chunk j + 1.  workgroups_per_cu = 0: default grid (the 4 workgroups per CU that fit, resident from start to
 * end, issue priority rotating over them); 1..5: a resident grid of that many workgroups per CU (at most the 4 that
 * fit; 3 leaves wave slots and LDS for a concurrently running K2).  reserved_workgroups: see "Launch policy" above
 * (vbq_quantize_f32 takes the default).  For planes (VBQ_LAYOUT_CB) the vector path wants row_begin % 8 == 0. */
int vbq_quantize_rows_f32(const float *d_mu, const float *d_sigma, int64_t n_rows, int32_t n_ch,
                          int32_t layout, const float *d_table_lm, const float *d_level_len,
                          const double *h_lambdas, int32_t n_lambda, int32_t N, int32_t mode,
                          uint16_t *d_out_idx, float *d_out_zhat, float *d_out_bits,
                          void *d_workspace, size_t workspace_bytes, int64_t row_begin, int64_t row_end,
                          int32_t workgroups_per_cu, int32_t reserved_workgroups, void *stream);

/* ----------------------------------------------------------------------------------
 * K1t / K1h  Solve + bit-length histogram in one kernel, nothing written per element (K1t: raw lengths at N = 10 without a
 *      per-lambda loop -- ten thresholds per element; K1h: the dense form for everything else).  Replaces the FIRST pass of
 *      ChannelwisePriorCDFQuantizer.build_entropy_models (quantizer.py:96-105): compress_batch_channel_latents
 *      followed by np.bincount(raw_num_bits[:, c], minlength=N+1) per lambda and channel -- which needs the bit
 *      level of every winner and nothing else.  Same arithmetic and tie rules as vbq_quantize_f32 (VBQ_MODE_F32).
 *   d_level_counts  int64 [n_lambda][n_ch][N+1], ADDED to (zero it first).
 *   layout          VBQ_LAYOUT_CB, VBQ_LAYOUT_BC_TO_CB, or any layout with n_ch == 1.
 *   reserved_workgroups  see "Launch policy" above (0: every slot).
 *   Returns VBQ_ERR_UNSUPPORTED for lambdas outside [1.9e-12, 1.8e19] (use vbq_quantize_f32 + vbq_histogram_u16).
 * ---------------------------------------------------------------------------------- */
int vbq_level_counts_f32(const float *d_mu, const float *d_sigma, int64_t n_rows, int32_t n_ch,
                         int32_t layout, const float *d_table_lm, const float *d_level_len,
                         const double *h_lambdas, int32_t n_lambda, int32_t N, int64_t *d_level_counts,
                         void *d_workspace, size_t workspace_bytes, int32_t reserved_workgroups, void *stream);

/* Code lengths from counts through a table: out[i] = (level_period ? i % level_period : 0) + lut[counts[i]].
 * Replaces the float32 arithmetic of quantizer.py:105-110 / 141-146 (counts + n -> / sum -> -log2) when the caller
 * can tabulate it: with B elements per (lambda, channel) row and add-n smoothing, every row's sum is the same
 * exact integer B + K n (< 2^24), so -log2(f32(k + n) / f32(B + K n)) is a function of the count k alone; the
 * caller builds lut[0..B] on the HOST with the reference's own NumPy operations (bit-identical by construction)
 * and the table lookup keeps the whole alternation on the device.  level_period = N + 1 adds the bit level n to
 * every entry (the "n + overhead" of quantizer.py:171-175, one f32 add).  Counts outside [0, lut_n) clamp.
 *   d_counts      int64 (counts_are_i32 = 0) or int32 (!= 0), n entries
 *   d_out_len     optional f32 [n]: level + lut[count];  d_out_model optional f32 [n]: lut[count] */
int vbq_code_lengths_from_counts(const void *d_counts, int32_t counts_are_i32, int64_t n,
                                 const float *d_lut, int64_t lut_n, int32_t level_period,
                                 float *d_out_len, float *d_out_model, void *stream);

/* The same arithmetic on the HOST, for the count tables that cannot be tabulated (2^24 samples per histogram row or more, fractional
 * smoothing): model[r][k] = -log2(f32(count[r][k] + n) / sum_k f32(count[r][k] + n)) exactly as quantizer.py:105-110 / 141-146
 * evaluates it in NumPy float32 (the row sum in NumPy's pairwise order); h_out_len[r][k] = k + model[r][k] when add_level != 0
 * (the "n + overhead" of :171-175).  h_* are HOST pointers (pinned or not); K <= 8192; either output may be NULL.
 *   log2_loop / log2_data   the float32 log2 as a NumPy ufunc inner loop (numpy/ufuncobject.h PyUFuncGenericFunction: args[0] in,
 *                           args[1] out, dimensions[0] elements, byte steps): NumPy's float32 log2 is not libm's, and the
 *                           reference's numbers are NumPy's -- the Python host hands over np.log2's own loop (vbq_amd/pipeline.py).
 *                           NULL: libm's log2f.
 * vbq_host_stage_run(stage) runs it on a filled-in descriptor: the function a caller gives hipLaunchHostFunc to put the step
 * BETWEEN two device stages of a stream without a synchronisation -- plain C on the runtime's callback thread, no interpreter
 * lock involved; `status` receives the return code, `runs` counts the executions. */
typedef void (*vbq_f32_loop)(char **args, const intptr_t *dimensions, const intptr_t *steps, void *data);
typedef struct vbq_host_stage {
    const void *h_counts;
    int32_t counts_are_i32;
    int32_t add_level;
    int64_t n_rows;
    int64_t K;
    float add_n_smoothing;
    int32_t status;
    vbq_f32_loop log2_loop;
    void *log2_data;
    float *h_out_model;
    float *h_out_len;
    int64_t runs;
} vbq_host_stage;
int vbq_host_neg_log2_freq_f32(const void *h_counts, int32_t counts_are_i32, int64_t n_rows, int64_t K, float add_n_smoothing,
                               int32_t add_level, vbq_f32_loop log2_loop, void *log2_data, float *h_out_model,
                               float *h_out_len);
void vbq_host_stage_run(void *stage);

/* ----------------------------------------------------------------------------------
 * K1c  Generic candidate solve.  Replaces utils.batch_quantize_indep_dims
 *      (img-compression/utils.py:363-423) for caller-built candidates, i.e. its
 *      "3D tensor of M x B x K" form (:367-370), and -- with n_lambda = 1 and the sorted
 *      table broadcast by the caller -- utils.quantize_indep_dims (:330-360).
 *   d_P     f32 [M][n_elems] candidate code points (n_elems = B*K flattened).
 *   d_len   f32 [M][n_elems], or [n_lambda][M][n_elems] when len_per_lambda != 0
 *           (the 4-D stack of utils.py:393-394).
 *   d_out_j   optional i32 [n_lambda][n_elems] winning candidate (first maximum);
 *   NaN scores (+-inf candidates against an infinite mu or sigma, lambda = 0 times an infinite length):
 *     VBQ_MODE_F64_SCORE follows np.argmax, the reference's NumPy backend: the first NaN wins.
 *     VBQ_MODE_F32 keeps its strict '>' scan: a NaN score never replaces the running best, so a NaN after
 *     candidate 0 is never taken and a NaN at candidate 0 keeps j = 0.
 *   d_out_zhat / d_out_bits   optional f32 [n_lambda][n_elems]   (utils.py:414-415).
 * ---------------------------------------------------------------------------------- */
int vbq_argmax_candidates_f32(const float *d_P, const float *d_len, int32_t len_per_lambda,
                              const float *d_mu, const float *d_sigma, int64_t n_elems,
                              const double *h_lambdas, int32_t n_lambda, int32_t M, int32_t mode,
                              int32_t *d_out_j, float *d_out_zhat, float *d_out_bits, void *stream);

/* ----------------------------------------------------------------------------------
 * The reference's first, xi-space encoder (img-compression/utils.py:215-304), float64 as there.
 *   vbq_xi_intervals_f64  utils.get_all_N_bit_intervals (:215-260): d_left / d_right [N+1][K] = the two n-bit grid
 *                         points around xi[k] for every bit budget n (n = 0: both 0.5; outside the grid: both the rim).
 *   vbq_xi_select_f64     utils.encode_vectorized after its three callables (:291-303).  d_F, d_endpoints,
 *                         d_unsquashed are [2][N+1][K] (left first, np.stack order): picks the better endpoint per budget
 *                         (first maximum), subtracts lamb * n, picks the best budget (first maximum) and gathers
 *                         z_hat, xi_hat, num_bits (int64, as NumPy's argmax) and the per-coordinate objective f_z_hat
 *                         (the caller sums it: result['score'] = np.sum(f_z_hat)).
 * squash / unsquash / fun are the caller's functions and stay where the caller evaluates them.
 * ---------------------------------------------------------------------------------- */
int vbq_xi_intervals_f64(const double *d_xi, int64_t K, int32_t N, double *d_left, double *d_right, void *stream);
int vbq_xi_select_f64(const double *d_F, const double *d_endpoints, const double *d_unsquashed, int64_t K, int32_t N,
                      double lamb, double *d_z_hat, int64_t *d_num_bits, double *d_xi_hat, double *d_f_z_hat, void *stream);

/* ----------------------------------------------------------------------------------
 * K1n  Notebook solve.  Replaces compress_coordinates(means, stds, beta, bitlengths)
 *      (word-embeddings/compress-trained-word-embeddings.ipynb:429-443): f64 squared
 *      error against an f64 code book, penalty (2*beta)*sigma^2 rounded to f32 and
 *      multiplied by the integer length, first minimum in level-major order; one
 *      shared code book.  Output values are the code points rounded to f32 (the
 *      notebook stores into empty_like(means)).
 *   d_codebook_lm   f64 [T] level-major (ipynb:383-389), non-decreasing in xi.
 *   h_betas         HOST doubles [n_beta].
 *   d_out_idx       u16 [n_beta][n] rank index;  d_out_val optional f32 [n_beta][n].
 *   Non-finite and out-of-range inputs follow NumPy, nothing is special-cased away from it
 *   (tests/test_gpu_notebook_variants.py, against the reference pinned in
 *   tests/test_notebook_f64.py): np.argmin returns the first NaN, and slot 0 (the root)
 *   costs err_0 + w * 0 with w = fl32(fl32(2 beta) * fl32(sigma^2)), so the root is the
 *   answer for a NaN mean, for an infinite mean (every cost inf or NaN) and for every w
 *   that is NaN or +-inf (sigma NaN or inf, sigma^2 overflowing f32, 0 * inf).  sigma = 0
 *   or a sigma^2 that underflows gives w = 0: the nearest code point, the first in
 *   level-major order among equals.  The sign of sigma does not matter.  A negative beta is
 *   scored on all 2^(N+1)-1 points (the neighbours of the mean are not enough there: a
 *   cost near -|w| N can round every point of a level onto the same value, and the first
 *   of them wins); such calls cost about a hundred times a non-negative one.  For
 *   beta >= 0 the kernels score the two neighbours of the mean per level, which equals the
 *   full scan as long as |mean| stays below about 2^50 code-book spacings (1e12 scales at
 *   N = 10; beyond that c - mean rounds neighbouring points onto each other and the first
 *   of them would win; from about 2^53 scales on every point ties and the root wins,
 *   which the kernels reproduce again: +-3e38 is tested).
 * ---------------------------------------------------------------------------------- */
int vbq_quantize_notebook_f64(const float *d_means, const float *d_stds, int64_t n,
                              const double *d_codebook_lm, const double *h_betas, int32_t n_beta,
                              int32_t N, uint16_t *d_out_idx, float *d_out_val, void *stream);

/* ----------------------------------------------------------------------------------
 * K2  Histogram pass.  Replaces the per-channel np.bincount of quantizer.py:104-105
 *     and :138-140 and the Counter of ipynb:453.  counts[l][c][q] += #{elements of
 *     channel c with index q under lambda l}.  Counts are ADDED to d_counts (zero it
 *     first for a fresh histogram); int64 so that 1e9-element shards cannot overflow.
 *     The bit-length histogram of :104 is the same array summed over the ranks of each
 *     level (level = N - ctz(q+1)).
 * ---------------------------------------------------------------------------------- */
int vbq_histogram_u16(const uint16_t *d_idx, int64_t n_rows, int32_t n_ch, int32_t layout,
                      int32_t n_lambda, int32_t N, int64_t *d_counts, void *stream);

/* Same pass with 32-bit counters: half the bytes for the cross-GPU all-reduce.  The caller
 * guarantees that no bin can reach 2^31 -- i.e. the GLOBAL number of rows per channel (over
 * all ranks whose histograms will be summed into this buffer) is below 2^31. */
int vbq_histogram_u16_i32(const uint16_t *d_idx, int64_t n_rows, int32_t n_ch, int32_t layout,
                          int32_t n_lambda, int32_t N, int32_t *d_counts, void *stream);

/* K2 on rows [row_begin, row_end) of the full index array (same addressing rules as vbq_quantize_rows_f32);
 * d_counts is int32 when counts_are_i32 != 0, else int64. */
int vbq_histogram_rows_u16(const uint16_t *d_idx, int64_t n_rows, int32_t n_ch, int32_t layout,
                           int32_t n_lambda, int32_t N, void *d_counts, int32_t counts_are_i32,
                           int64_t row_begin, int64_t row_end, void *stream);

/* K2 as the LAST stage of the build: counts := histogram of the planes d_idx [n_lambda][n_ch][n_rows] (ASSIGNED, not added:
 * no zeroing beforehand) and, when d_models is given, models[l][c][q] = lut[counts[l][c][q]] -- the code-length table of
 * quantizer.py:141-146 in its tabulated form (see vbq_code_lengths_from_counts).  With at least 2048 (lambda, channel) rows
 * one workgroup owns each row, stores its bins and looks the lengths up in the same flush (no memset of the count array, no
 * atomics, no separate pass over it); smaller problems are composed from the plain entry points.  Single-GPU form: sharded
 * builds all-reduce the counts first and then call vbq_code_lengths_from_counts. */
int vbq_histogram_models_u16(const uint16_t *d_idx, int64_t n_rows, int32_t n_ch, int32_t n_lambda, int32_t N,
                             void *d_counts, int32_t counts_are_i32, const float *d_lut, int64_t lut_n,
                             float *d_models, void *stream);

/* Largest index of a u16 index array (d_max: u32, device, MAX-ed into; zero it first).  K2 and the gather are
 * memory-safe for any u16 input (indices >= T are counted in a wrapped bin / read the last table entry); a
 * caller holding indices that did not come from K1 (a file, a decoder) checks max < T with this first. */
int vbq_index_max_u16(const uint16_t *d_idx, int64_t n, uint32_t *d_max, void *stream);

/* ----------------------------------------------------------------------------------
 * K3  Moment pass.  Replaces empirical_std = sqrt(mean(mu^2)) (ipynb:373-374) and the
 *     per-channel mean/std a FactoredGaussianPrior needs (vae_models.py:32-35).
 *     d_out[c] = { sum x, sum x^2 } accumulated in f64 (ADDED to d_out).
 * ---------------------------------------------------------------------------------- */
int vbq_moments_f32(const float *d_x, int64_t n_rows, int32_t n_ch, int32_t layout,
                    double *d_out /* [n_ch][2] */, void *stream);

/* The notebook's moment in NumPy's own float32 order: d_out[0] = np.sum(x.ravel()**2) bit for bit (blocks of 8192
 * elements, pairwise inside a block, block results chained; see vbq_reduce.hip).  Replaces the reduction inside
 * empirical_std = np.sqrt(np.mean(vecs_u.ravel()**2)) (ipynb:374); the caller divides by n and takes the root in
 * float32.  d_x 16-byte aligned; workspace: vbq_numpy_sum_sq_workspace_bytes(n) bytes of device memory. */
size_t vbq_numpy_sum_sq_workspace_bytes(int64_t n);
int vbq_numpy_sum_sq_f32(const float *d_x, int64_t n, float *d_out, void *d_workspace, size_t workspace_bytes,
                         void *stream);

/* np.sum of every row of a float32 batch [n_rows][n] in NumPy's own float32 order, bit for bit: d_out[r] = np.sum(x[r]) for a
 * contiguous x[r] of any shape with n elements.  Replaces the reductions of the evaluation loop, utils.py:547-552
 * (`nbits = np.sum(num_bits)`, `np.sum(num_bits_cl)` per image and lambda): with the per-lambda code lengths of
 * vbq_compress_latents_f32 still on the device, L floats cross PCIe instead of L x [B, C] arrays.  n_rows <= 65535;
 * workspace: vbq_numpy_row_sums_workspace_bytes(n_rows, n) bytes of device memory. */
size_t vbq_numpy_row_sums_workspace_bytes(int64_t n_rows, int64_t n);
int vbq_numpy_row_sums_f32(const float *d_x, int64_t n_rows, int64_t n, float *d_out, void *d_workspace,
                           size_t workspace_bytes, void *stream);

/* ----------------------------------------------------------------------------------
 * Table lookup by rank index: out[l][e] = tab[(l)][c(e)][idx[l][e]].  Replaces
 *   tf.gather(entropy_model, I, batch_dims=1)            quantizer.py:226-228
 *   tf.gather(code_points_by_channel, qidx, batch_dims=1) quantizer.py:136
 *   d_tab   f32 [n_lambda][n_ch][T] when tab_per_lambda != 0, else [n_ch][T];
 *           indexed by rank (i.e. a SORTED table such as code_points_by_channel).
 *   layout / out_layout: element layout of d_idx and of d_out (they may differ: the
 *           Z_hat / num_bits handed back to the caller are channel-last, :228,237).
 * ---------------------------------------------------------------------------------- */
int vbq_gather_f32(const uint16_t *d_idx, int64_t n_rows, int32_t n_ch, int32_t layout,
                   int32_t n_lambda, int32_t N, const float *d_tab, int32_t tab_per_lambda,
                   float *d_out, int32_t out_layout, void *stream);

/* ----------------------------------------------------------------------------------
 * Rate-distortion report of a solve: for every lambda l,
 *     d_out[2l]     += sum_e (z_e - mu_e)^2 / (2 sigma_e^2),   z_e = d_tab_sorted[c(e)][idx[l][e]]   (utils.py:319-320
 *                      without the sign and the constant: the distortion term the solve minimises)
 *     d_out[2l + 1] += sum_e d_rate[(l)][c(e)][idx[l][e]]                                          (the bits of
 *                      quantizer.py:226-228 summed as utils.py:547-549 sums them; skipped when d_rate is NULL)
 * in f64.  d_tab_sorted is the SORTED table (code_points_by_channel); d_rate is [n_lambda][n_ch][T] when
 * rate_per_lambda != 0 (entropy_models), else [n_ch][T].  d_out: f64 [n_lambda][2], zero it first.  A report -- the
 * Lagrangian of BASELINE's R-D gate is d_out[2l] + lambda_l * d_out[2l + 1] -- not an input of any kernel.
 * ---------------------------------------------------------------------------------- */
int vbq_rd_sums_u16(const float *d_mu, const float *d_sigma, const uint16_t *d_idx, int64_t n_rows, int32_t n_ch,
                    int32_t layout, int32_t n_lambda, int32_t N, const float *d_tab_sorted, const float *d_rate,
                    int32_t rate_per_lambda, double *d_out, void *stream);

/* ----------------------------------------------------------------------------------
 * Layout change between channel-last and channel-major planes: out[c][r] = in[r][c]
 * (f32, LDS-tiled).  Replaces the tf.transpose calls around the solve
 * (quantizer.py:73,163-164,223,228): the hot kernels want [C][B] planes so that a
 * workgroup works on ONE channel (one 8 KB table in LDS, wave-uniform penalties).
 * ---------------------------------------------------------------------------------- */
int vbq_transpose_f32(const float *d_in, int64_t n_rows, int64_t n_cols, float *d_out, void *stream);

/* The same for a stack of planes of 2- or 4-byte elements: out[b][c][r] = in[b][r][c] for b < n_batch.  With
 * elem_bytes = 2 it hands the u16 rank indices of the plane kernels ([n_lambda][n_ch][n_rows]) back in the caller's
 * channel-last layout ([n_lambda][n_rows][n_ch], the shape of compress_batch_channel_latents' results,
 * quantizer.py:186-188); with 4, Z_hat / num_bits planes.  n_batch <= 65535. */
int vbq_transpose_planes(const void *d_in, int64_t n_batch, int64_t n_rows, int64_t n_cols, int32_t elem_bytes,
                         void *d_out, void *stream);

/* ----------------------------------------------------------------------------------
 * The per-image call of the evaluation loop: ChannelwisePriorCDFQuantizer.compress_latents
 * (quantizer.py:190-240, called once per image by utils.py:542-554) as ONE C call =
 * three launches (planes, solve, fused lookups).  The three pieces are entry points of
 * their own as well.
 *
 *   vbq_prep_planes_f32     channel-last latents [n_rows][n_ch] -> channel-major planes [n_ch][n_rows]
 *                           (the tf.transpose of quantizer.py:163-164,223), means and spreads in one launch;
 *                           spread_kind says what d_spread_bc holds: VBQ_SPREAD_SIGMA the standard deviations,
 *                           VBQ_SPREAD_VARIANCE exp(logvar) (sigma = sqrt(.), IEEE), VBQ_SPREAD_LOGVAR the encoder's
 *                           log-variances themselves (sigma = sqrt(exp(.)): quantizer.py:197,202
 *                           `tf.exp(posterior_logvars) ** 0.5` inside the same launch).
 *   vbq_gather_latents_u16  ONE pass over rank indices in planes [n_lambda][n_ch][n_rows] writing, channel-last
 *                           [n_lambda][n_rows][n_ch] (any subset; NULL skips an output):
 *                             d_out_zhat      f32  d_table_sorted[c][q]                      quantizer.py:224-225
 *                             d_out_raw_bits  the bit length n(q) = N - ctz(q + 1) of the winner as int32 when
 *                                             d_level_len is NULL (quantizer.py:167-169), else f32
 *                                             d_level_len[l][c][n(q)] = "n + overhead"        quantizer.py:171-175
 *                             d_out_num_bits  f32  d_models[l][c][q] (entropy_models, by rank) quantizer.py:226-228
 *                             d_out_idx       u16  q itself (the index planes transposed)
 *   vbq_compress_latents_f32   prep -> vbq_quantize_f32 on planes (raw lengths when d_level_len is NULL) ->
 *                           gather.  d_spread_bc as for vbq_prep_planes_f32 (spread_kind).
 *                           Workspace: vbq_compress_latents_workspace_bytes() bytes of device memory, 256-byte
 *                           aligned (the planes, the index planes and the solve's own workspace live there).
 * ---------------------------------------------------------------------------------- */
enum { VBQ_SPREAD_SIGMA = 0, VBQ_SPREAD_VARIANCE = 1, VBQ_SPREAD_LOGVAR = 2 };
int vbq_prep_planes_f32(const float *d_means_bc, const float *d_spread_bc, int32_t spread_kind, int64_t n_rows,
                        int32_t n_ch, float *d_mu_cb, float *d_sigma_cb, void *stream);
int vbq_gather_latents_u16(const uint16_t *d_idx_planes, int64_t n_rows, int32_t n_ch, int32_t n_lambda, int32_t N,
                           const float *d_table_sorted, const float *d_level_len, const float *d_models,
                           float *d_out_zhat, void *d_out_raw_bits, float *d_out_num_bits, uint16_t *d_out_idx,
                           void *stream);
size_t vbq_compress_latents_workspace_bytes(int64_t n_rows, int32_t n_ch, int32_t n_lambda, int32_t N);
int vbq_compress_latents_f32(const float *d_means_bc, const float *d_spread_bc, int32_t spread_kind,
                             int64_t n_rows, int32_t n_ch, const float *d_table_lm, const float *d_table_sorted,
                             const float *d_level_len, const float *d_models, const double *h_lambdas,
                             int32_t n_lambda, int32_t N, float *d_out_zhat, void *d_out_raw_bits,
                             float *d_out_num_bits, void *d_workspace, size_t workspace_bytes, void *stream);

/* ----------------------------------------------------------------------------------
 * The whole two-pass build of ChannelwisePriorCDFQuantizer.build_entropy_models (quantizer.py:82-150) on ONE GPU as one C call
 * = six stream-ordered launches, nothing waits for the host (sharded builds all-reduce between the pieces and call them one by
 * one: INTEGRATION.md):
 *     planes (d_spread_bc / spread_kind as for vbq_prep_planes_f32)                                  quantizer.py:87-92
 *     pass 1   vbq_level_counts_f32 with raw lengths -> d_level_counts [n_lambda][n_ch][N+1] (int64, assigned)   :96-105
 *     lengths  d_raw_models = lut_levels[count], d_level_len = n + lut_levels[count]   (f32 [n_lambda][n_ch][N+1])   :105-112, 171-175
 *     pass 2   vbq_quantize_f32 with d_level_len; vbq_histogram_models_u16 -> d_counts [n_lambda][n_ch][T] (int64, or int32 with
 *              counts_are_i32; assigned) and d_models = lut_ranks[count] (f32 [n_lambda][n_ch][T]; both NULL: no model table)   :119-146
 *   d_lut_levels / d_lut_ranks: the tabulated -log2 of the smoothed frequencies for every possible count 0 .. n_rows, built by the
 *   caller with the reference's own NumPy float32 operations (vbq_code_lengths_from_counts): n_lut >= n_rows + 1 entries each.
 *   Workspace: vbq_build_entropy_models_workspace_bytes() bytes of device memory, 256-byte aligned (planes, index planes, solve).
 *   reserved_workgroups: for both solve passes, see "Launch policy" above (0: every slot -- a single-GPU build has no neighbour).
 * ---------------------------------------------------------------------------------- */
size_t vbq_build_entropy_models_workspace_bytes(int64_t n_rows, int32_t n_ch, int32_t n_lambda, int32_t N);
int vbq_build_entropy_models_f32(const float *d_means_bc, const float *d_spread_bc, int32_t spread_kind, int64_t n_rows,
                                 int32_t n_ch, const float *d_table_lm, const double *h_lambdas, int32_t n_lambda,
                                 int32_t N, const float *d_lut_levels, int64_t n_lut_levels, const float *d_lut_ranks,
                                 int64_t n_lut_ranks, int64_t *d_level_counts, float *d_level_len, float *d_raw_models,
                                 void *d_counts, int32_t counts_are_i32, float *d_models, void *d_workspace,
                                 size_t workspace_bytes, int32_t reserved_workgroups, void *stream);

/* ----------------------------------------------------------------------------------
 * K4  BMSHJ2018 prior (learned_prior.py).  Parameters are the EFFECTIVE ones --
 *     softplus(matrix_i), bias_i, tanh(factor_i) -- packed per channel as
 *       [ M0(3x1) b0(3) f0(3) | M1(3x3) b1(3) f1(3) | M2(3x3) b2(3) f2(3) | M3(1x3) b3(1) ]
 *     = 43 floats (dims = (3,3,3), learned_prior.py:11,30-57), row-major matrices.
 *   vbq_bmshj_cdf_pdf_f32   cdf / analytic pdf / log(pdf+1e-10) at x
 *                           (learned_prior.py:70-148, 235-242, 244-334); any of the
 *                           three outputs may be NULL.  x is [n_rows][n_ch] channel-last.
 *   vbq_bmshj_icdf_step_f32 one masked bisection update of learned_prior.py:199-209 on
 *                           [n_rows][n_ch] brackets; writes mid points and accumulates
 *                           d_flags[0] = #(f(mid) != 0), d_flags[1] = bits of the minimum
 *                           bracket width (as u32 of a non-negative float) so that the
 *                           host can apply the global stopping rule of :210-211.
 * ---------------------------------------------------------------------------------- */
#define VBQ_BMSHJ_PARAMS_PER_CHANNEL 43

int vbq_bmshj_cdf_pdf_f32(const float *d_params, const float *d_x, int64_t n_rows, int32_t n_ch,
                          float *d_cdf, float *d_pdf, float *d_logpdf, void *stream);

int vbq_bmshj_icdf_step_f32(const float *d_params, const float *d_xi, int64_t n_rows, int32_t n_ch,
                            float *d_left, float *d_right, float *d_mid, uint32_t *d_flags,
                            void *stream);

/* n_steps of those updates enqueued at once, the stopping rule of learned_prior.py:210-211 applied ON THE DEVICE between them
 * (no host read per bisection step): step j runs only while the pair step j - 1 accumulated does not meet the rule (no
 * f(mid) != 0 left, or the minimum bracket width <= tol).  d_flags: u32 [n_steps + 1][2], written here; after a synchronisation
 * the caller reads it: the first j >= 1 whose pair meets the rule is the number of steps the reference's loop would have run
 * (d_mid holds that step's mid points); none does: call again with first = 0, which continues the chain from flags[n_steps]
 * of the previous call (copied by the caller to flags[0]). */
int vbq_bmshj_icdf_chain_f32(const float *d_params, const float *d_xi, int64_t n_rows, int32_t n_ch,
                             float *d_left, float *d_right, float *d_mid, uint32_t *d_flags, int32_t n_steps,
                             float tol, int32_t first, void *stream);

/* Fit step of the prior (learned_prior.py:402-430: loss = -mean(log(pdf + 1e-10)), full batch).
 * d_x_cb is f32 [n_ch][n_rows] (channel-major planes).  ADDS to d_out[c][0..42] the gradient of
 * sum_rows -log(pdf+1e-10) with respect to the 43 effective parameters of channel c (same
 * packing as above) and to d_out[c][43] that sum itself; f64.  The caller applies the
 * softplus / tanh chain rule, the 1/(n_rows*n_ch) of reduce_mean and the optimiser. */
int vbq_bmshj_nll_grad_f32(const float *d_params, const float *d_x_cb, int64_t n_rows, int32_t n_ch,
                           double *d_out /* [n_ch][44] */, void *stream);

/* ----------------------------------------------------------------------------------
 * Entropy coder for the rank indices.  The reference only ESTIMATES rates
 * as sum(-log2 freq) (quantizer.py:144,226-228); this turns them into bits.  Static-model rANS
 * (32-bit state, 16-bit renormalisation, 15 probability bits).
 *   d_idx    u16 [n_streams][n]   one stream per (lambda, channel): the [L][C][B] planes K1 writes
 *   d_freq   u16 [n_streams][T]   quantised frequencies, every entry >= 1, each row sums to 2^15
 *   seg      symbols per independently coded segment (one GPU thread each)
 *   d_words  u16 [n_streams][nseg][seg+2], nseg = ceil(n/seg): per segment the renormalisation
 *            words in emission order followed by the final state (low half, high half)
 *   d_sizes  u32 [n_streams][nseg] number of valid words of every segment
 * Symbols are coded last-to-first so that decoding runs first-to-last.
 * ---------------------------------------------------------------------------------- */
int vbq_rans_encode_u16(const uint16_t *d_idx, int64_t n_streams, int64_t n, int32_t N, int32_t seg,
                        const uint16_t *d_freq, uint16_t *d_words, uint32_t *d_sizes, void *stream);
/* vbq_rans_sizes_u16: the d_sizes of vbq_rans_encode_u16 for the same arguments, entry by entry, without the words -- the
 * same state machine, renormalisation and final-state flush, storing only u32 [n_streams][nseg] (no d_words buffer of
 * n_streams * nseg * (seg + 2) u16): the exact coded length of every segment.  d_freq may hold entries of 0 for symbols
 * that do not occur (a table fitted to the data it codes, as vbq_rans_decode_values_f32 reads); an index outside the
 * table is read safely, as in the encoder.  Added without an ABI version bump: nothing that existed before changed. */
int vbq_rans_sizes_u16(const uint16_t *d_idx, int64_t n_streams, int64_t n, int32_t N, int32_t seg, const uint16_t *d_freq,
                       uint32_t *d_sizes, void *stream);
/* Decoding treats words / sizes as UNTRUSTED: no read leaves a segment's seg + 2 words, every decoded index is
 * below T, and d_status (u32, device, may be NULL; OR-ed into, zero it first) reports what was wrong --
 * bit 0 a segment size outside [2, seg + 2], bit 1 a segment that ran out of words, bit 2 words left over or a
 * wrong final state (a damaged stream), bit 3 a frequency row that does not sum to 2^15.  Segments with bits 0 / 3
 * decode to zeros. */
int vbq_rans_decode_u16(const uint16_t *d_words, const uint32_t *d_sizes, int64_t n_streams, int64_t n,
                        int32_t N, int32_t seg, const uint16_t *d_freq, uint16_t *d_idx, uint32_t *d_status,
                        void *stream);
/* Packed payload of the byte-string container (vbq_amd/bitstream.py): the valid words of every segment, stream-major
 * then segment-major, without the padding -- segment g = s * nseg + j occupies payload words [off[g], off[g] + size[g]),
 * off = exclusive prefix sum of the sizes.  M = n_streams * nseg segments, nseg = ceil(n / seg), as above.
 * vbq_rans_pack_u16: d_words / d_sizes as vbq_rans_encode_u16 wrote them -> d_payload u16, room for up to
 * M * (seg + 2) words (the largest possible total); d_offsets int64 [M] receives off (it is also the scratch of the
 * scan); *d_total (u64, device) the number of payload words.  Sizes above seg + 2 are clamped (memory safety only). */
int vbq_rans_pack_u16(const uint16_t *d_words, const uint32_t *d_sizes, int64_t n_streams, int64_t n, int32_t seg,
                      uint16_t *d_payload, int64_t *d_offsets, uint64_t *d_total, void *stream);
/* vbq_rans_unpack_u16: the inverse, into the padded layout vbq_rans_decode_u16 reads.  The payload u16 [n_words] and the
 * sizes u16 [M] (as a file stores them) are UNTRUSTED: no read leaves [0, n_words) and no write leaves d_words
 * u16 [M][seg + 2] / d_sizes u32 [M].  d_offsets int64 [M] as above.  d_status (u32, device, may be NULL; OR-ed into, zero
 * it first): bit 0 a size outside [2, seg + 2] (counted as 0), bit 4 sizes whose sum is not n_words.  A segment with a
 * bad size or one that would end past n_words gets size 0 in d_sizes, so that the decoder rejects it as well; its words
 * are not written.  The decoder only reads the first size[g] words of a segment: d_words need not be zeroed. */
int vbq_rans_unpack_u16(const uint16_t *d_payload, int64_t n_words, const uint16_t *d_sizes_in, int64_t n_streams,
                        int64_t n, int32_t seg, uint16_t *d_words, uint32_t *d_sizes, int64_t *d_offsets,
                        uint32_t *d_status, void *stream);
/* Row-wise decode of ONE packed stream (the embedding container of vbq_amd/bitstream.py, magic "VBQe").  These two
 * entry points were added without an ABI version bump: nothing that existed before changed.
 * vbq_rans_segment_offsets_u16: d_offsets int64 [M] = the exclusive prefix sum of the UNTRUSTED sizes u16 [M], at every
 * segment.  d_status as vbq_rans_unpack_u16: bit 0 a size outside [2, seg + 2] (counted as 0), bit 4 a sum other than
 * n_words. */
int vbq_rans_segment_offsets_u16(const uint16_t *d_sizes, int64_t M, int32_t seg, int64_t n_words, int64_t *d_offsets,
                                 uint32_t *d_status, void *stream);
/* vbq_rans_decode_values_f32: decodes the stream of n symbols (nseg = ceil(n / seg) segments) straight from the payload
 * u16 [n_words] (segment g at words [d_offsets[g], d_offsets[g] + d_sizes[g])) and writes d_values[symbol] as f32 --
 * d_freq u16 [T] and d_values f32 [T], T = 2^(N+1) - 1.  Entries of d_freq may be 0 (a table fitted to the data it codes);
 * every entry must be <= 2^15 - 1 and the row must sum to 2^15.
 *   d_segments == NULL: every segment, into d_out f32 [n] in stream order (n_sel is not read beyond n_sel >= 0).
 *   otherwise:          the n_sel listed segment ids (any order, repeats allowed), segment d_segments[i] into
 *                       d_out[i * seg ...]; d_out holds n_sel * seg values, the last segment writes only its valid length.
 * Everything but the table sizes is UNTRUSTED: no read leaves [off, off + size) or [0, n_words), no write leaves d_out,
 * every decoded symbol is below T.  d_status (u32, device, may be NULL; OR-ed into, zero it first): bits 0 - 3 as
 * vbq_rans_decode_u16 (a segment whose words do not lie in [0, n_words) counts as bit 0; an entry above 2^15 - 1 as bit 3),
 * bit 5 (32) a listed segment id outside [0, nseg).  Segments with bits 0 / 3 / 5 decode to zeros; with bits 1 / 2 the
 * output of that segment is meaningless. */
int vbq_rans_decode_values_f32(const uint16_t *d_payload, int64_t n_words, const uint16_t *d_sizes, const int64_t *d_offsets,
                               int64_t n, int32_t seg, int32_t N, const uint16_t *d_freq, const float *d_values,
                               const int64_t *d_segments, int64_t n_sel, float *d_out, uint32_t *d_status, void *stream);

/* ----------------------------------------------------------------------------------
 * Wave-interleaved rANS: the coder of the compact latent file (vbq_amd/bitstream.py, magic "VBQc").  These three entry
 * points were added without an ABI version bump: nothing that existed before changed.
 *
 * Coder constants as above (32-bit state, start state 2^16, 16-bit words, 15 probability bits; c = exclusive cumulative
 * frequency).  The n_streams * n symbols of d_idx u16 [n_streams][n], in that order, are cut every `part` symbols
 * (1 <= part <= 2^24; the last part may be shorter): P = ceil(n_streams * n / part) parts, each coded by 64 lanes.  A part
 * may start and end inside a stream.  Inside a part a RUN is a maximal stretch within one stream; it uses that stream's
 * frequency row and takes ceil(len / 64) steps; in step t lane l owns the run's symbol 64 t + l when that is < len and
 * idles otherwise.  The 64 lane states carry on from run to run.  The words of a part, in the order the decoder reads them:
 *   1. 128 words: the states of lanes 0 .. 63, low half then high half of each;
 *   2. for every run in order and every step in order: each active lane decodes (slot = x & 32767, x = f (x >> 15) + slot
 *      - c), then each active lane whose state is below 2^16 takes one word, in ascending lane order (x = x << 16 | w).
 *   At the end every word has been taken and every lane's state is 2^16.
 * The encoder is the exact inverse: runs last to first, steps last to first; a lane with x >= f << 17 emits x & 0xffff and
 * shifts x >>= 16 before x = (x / f << 15) + x % f + c.  A part of m symbols takes 128 .. m + 128 words.
 *
 * vbq_rans_il_sizes_u16:  d_sizes u32 [P], the words of every part (the encoder's state machine, counting only).
 * vbq_rans_il_encode_u16: writes part p to d_payload words [d_offsets[p], d_offsets[p] + d_sizes[p]), backwards from the
 *   end, so that no padded buffer and no pack pass is needed.  d_sizes as vbq_rans_il_sizes_u16 gave them for the same
 *   arguments, d_offsets int64 [P] their exclusive prefix sum, n_words the length of d_payload (no write leaves it; a part
 *   that does not fit is skipped).
 * vbq_rans_il_decode_u16: d_payload u16 [n_words], d_sizes and d_offsets (the exclusive prefix sum of d_sizes) are
 *   UNTRUSTED: no read leaves a part's [off, off + size), which is itself checked against [0, n_words); every index written
 *   to d_idx u16 [n_streams][n] is below T.  d_status (u32, device, may be NULL; OR-ed into, zero it first): bit 0 a part
 *   size outside [128, m + 128], bit 1 a part ran out of words, bit 2 words left over or a final state other than 2^16,
 *   bit 3 a frequency row that does not sum to 2^15 or holds an entry above 2^15 - 1, bit 4 the sizes do not add up to
 *   n_words (a part outside the payload, or the last part not ending at n_words).  A part with any bit decodes to zeros.
 * ---------------------------------------------------------------------------------- */
int vbq_rans_il_sizes_u16(const uint16_t *d_idx, int64_t n_streams, int64_t n, int32_t N, int32_t part,
                          const uint16_t *d_freq, uint32_t *d_sizes, void *stream);
int vbq_rans_il_encode_u16(const uint16_t *d_idx, int64_t n_streams, int64_t n, int32_t N, int32_t part,
                           const uint16_t *d_freq, const uint32_t *d_sizes, const int64_t *d_offsets, uint16_t *d_payload,
                           int64_t n_words, void *stream);
int vbq_rans_il_decode_u16(const uint16_t *d_payload, int64_t n_words, const uint32_t *d_sizes, const int64_t *d_offsets,
                           int64_t n_streams, int64_t n, int32_t N, int32_t part, const uint16_t *d_freq, uint16_t *d_idx,
                           uint32_t *d_status, void *stream);

/* ----------------------------------------------------------------------------------
 * Class-mapped rANS: the segment coder above with a frequency table that may change from symbol to symbol -- the coder of
 * the lambda-map latent file (vbq_amd/bitstream.py, magic "VBQm").  These three entry points were added without an ABI
 * version bump: nothing that existed before changed.
 *
 * Format, constants and state updates are those of vbq_rans_encode_u16: every stream of n symbols is cut into segments of
 * `seg` symbols, each an independent rANS stream (32-bit state, start state 2^16, 16-bit words, 15 probability bits) coded
 * last symbol to first: a symbol of frequency f and exclusive cumulative frequency c first emits x & 0xffff and shifts
 * x >>= 16 when x >= f << 17, then x = (x / f << 15) + x % f + c; after the first symbol the state goes out low half, then
 * high half.  The decoder starts from those two words and reads backwards: slot = x & 32767, the symbol is the one with
 * c <= slot < c + f, x = f (x >> 15) + slot - c, and x = x << 16 | word while x < 2^16.  What is new:
 *   d_cls    u8 [n]                       one class per symbol POSITION, in [0, n_classes), shared by all streams
 *   d_freq   u16 [n_classes][n_streams][T] the table of symbol i of stream s is row d_freq[d_cls[i]][s] (f and c above)
 *   d_idx    u16 [n_planes][n_streams][n]  n_planes == n_classes: symbol i of stream s is d_idx[d_cls[i]][s][i] -- the
 *            encoder reads straight from the [L][C][B] planes of a solve at n_classes lambdas, no select pass;
 *            n_planes == 1: it is d_idx[0][s][i]
 *   1 <= n_classes <= 4
 * d_words u16 [n_streams][nseg][seg + 2] and d_sizes u32 [n_streams][nseg] have exactly the layout of vbq_rans_encode_u16
 * (sizes in [2, seg + 2]), so vbq_rans_pack_u16 / vbq_rans_unpack_u16 serve unchanged; a segment whose symbols all have
 * class p is word for word what vbq_rans_encode_u16 writes with row d_freq[p][s].  An index outside the table or a class
 * outside [0, n_classes) is read safely by the encoder (as symbol 0 / class 0); the caller checks its map.
 * vbq_rans_map_sizes_u16: the d_sizes of vbq_rans_map_encode_u16 for the same arguments, without the words.
 * vbq_rans_map_decode_u16: words, sizes AND classes are UNTRUSTED.  d_status (u32, device, may be NULL; OR-ed into, zero it
 *   first): bits 0 - 3 as vbq_rans_decode_u16 (bit 3: any of the n_classes rows of the stream), bit 6 (64) a class
 *   >= n_classes in the segment -- it is compared before it selects any table.  Segments with bits 0 / 3 / 6 decode to
 *   zeros; every index written to d_idx u16 [n_streams][n] is below T.
 * Sizes, n_classes, n_planes and null pointers are checked before any device work (VBQ_ERR_INVALID_ARGUMENT); n == 0 or
 * n_streams == 0 returns VBQ_OK and does nothing.
 * ---------------------------------------------------------------------------------- */
int vbq_rans_map_encode_u16(const uint16_t *d_idx, int32_t n_planes, const uint8_t *d_cls, int32_t n_classes, int64_t n_streams,
                            int64_t n, int32_t N, int32_t seg, const uint16_t *d_freq, uint16_t *d_words, uint32_t *d_sizes,
                            void *stream);
int vbq_rans_map_sizes_u16(const uint16_t *d_idx, int32_t n_planes, const uint8_t *d_cls, int32_t n_classes, int64_t n_streams,
                           int64_t n, int32_t N, int32_t seg, const uint16_t *d_freq, uint32_t *d_sizes, void *stream);
int vbq_rans_map_decode_u16(const uint16_t *d_words, const uint32_t *d_sizes, const uint8_t *d_cls, int32_t n_classes,
                            int64_t n_streams, int64_t n, int32_t N, int32_t seg, const uint16_t *d_freq, uint16_t *d_idx,
                            uint32_t *d_status, void *stream);
/* The lambda-map latent file (magic "VBQm", version 1, every field little-endian): one latent tensor coded at up to four
 * lambdas, a class per latent position saying which.
 *   0   4      magic "VBQm"        4  1  version = 1     5  1  N (1..10)     6  1  ndim (>= 1)     7  1  P (1..4)
 *   8   4      C (u32)             12 4  segment (u32, 1..65533)             16 8  n_words (u64)
 *   24  8 P    the lambdas (f64, finite, distinct), class 0 first
 *   ..  16 P   digests (blake2b-128 of the code points and frequencies of each lambda, as VBQb), same order
 *   ..  8 ndim latent shape (u64 each, channel last: shape[-1] == C); B = prod(shape) / C positions
 *   ..         class block: 2 bits per position, position b in byte b / 4 at bits 2 (b % 4) and 2 (b % 4) + 1; ceil(B / 4)
 *              bytes, zero-padded to a multiple of 8 bytes; padding bits are zero and every class is < P
 *   ..  2 C nseg  segment sizes (u16, each in [2, segment + 2]), stream-major (channel), as VBQb
 *   ..  2 n_words payload, as VBQb: channel c is stream c, its symbol b coded with the table of (lambda[class[b]], c). */

/* ----------------------------------------------------------------------------------
 * Packed counters for the histogram all-reduce: three 21-bit fields per int64 word.
 * An integer SUM all-reduce of the words adds the fields independently while every GLOBAL count is
 * below 2^21, at 2.67 instead of 4 bytes per bin on the wire.  n bins <-> (n + 2) / 3 words.
 * Guard: *d_overflow (u32, device, may be NULL; OR-ed into, zero it first) is set to 1 when a LOCAL count is
 * negative or >= 2^21 / n_ranks -- while it stays 0 on every rank the sum over n_ranks ranks cannot carry from one
 * field into the next.  The caller checks the flag before trusting the unpacked sums.
 * ---------------------------------------------------------------------------------- */
int vbq_pack_counts_3x21(const int32_t *d_counts, int64_t n, int64_t *d_words, int32_t n_ranks,
                         uint32_t *d_overflow, void *stream);
int vbq_unpack_counts_3x21(const int64_t *d_words, int64_t n, int32_t *d_counts, void *stream);

/* ----------------------------------------------------------------------------------
 * The one collective of the path: SUM all-reduce of a histogram over the ranks of a node, RCCL over xGMI.
 * Replaces nothing in the reference (it is single-process); it is what makes quantizer.py:104-105 / 138-140 global
 * when the rows are sharded over GPUs: every rank ends up with the counts of ALL rows, integer sums, so the
 * entropy models do not depend on the number of ranks.  One communicator per (process, GPU):
 *   vbq_comm_unique_id   rank 0 fills VBQ_COMM_ID_BYTES host bytes and hands them to the other ranks by any means
 *   vbq_comm_init        collective: every rank calls it with the same id (the current HIP device is the rank's GPU)
 *   vbq_allreduce_hist   in place on d_counts (int64, or int32 when counts_are_i32 != 0), asynchronous on `stream`;
 *                        works for the level histogram of K1t / K1h, the rank histogram of K2 and the packed words of
 *                        vbq_pack_counts_3x21 (int64) alike
 *   vbq_comm_destroy
 * RCCL is bound at run time (dlopen): VBQ_ERR_UNSUPPORTED when no librccl.so can be loaded.
 * ---------------------------------------------------------------------------------- */
#define VBQ_COMM_ID_BYTES 128
int vbq_comm_unique_id(void *h_id);
int vbq_comm_init(void **comm, int32_t n_ranks, const void *h_id, int32_t rank);
int vbq_allreduce_hist(void *comm, void *d_counts, int64_t n, int32_t counts_are_i32, void *stream);
int vbq_comm_destroy(void *comm);

/* ----------------------------------------------------------------------------------
 * Comparison quantizers (img-compression/quantizer.py:259-333).
 *   vbq_uniform_quantize_f32  I = clip(floor((x - min) / delta), 0, levels-1) in f32 (:280,295),
 *                             value = offset + delta * I (:297); I is returned as f32 like the
 *                             reference does.  UniformQuantizer.quantize and the index pass of .fit.
 *   vbq_nearest_code_f64      scipy.cluster.vq.vq(samples, code_points) for 1-D data (:329): f64
 *                             squared distance, first minimum in code-book order; value = the code.
 * Any output may be NULL; d_counts (int64 [levels] / [n_codes]) is ADDED to when given: the
 * np.bincount of :281 / :314.
 * ---------------------------------------------------------------------------------- */
int vbq_uniform_quantize_f32(const float *d_x, int64_t n, float min, float delta, float offset,
                             int32_t levels, float *d_out_index, float *d_out_value, int64_t *d_counts,
                             void *stream);
int vbq_nearest_code_f64(const float *d_x, int64_t n, const double *d_codes, int32_t n_codes,
                         int32_t *d_out_index, double *d_out_value, int64_t *d_counts, void *stream);

/* ----------------------------------------------------------------------------------
 * Analogy evaluator (compress-trained-word-embeddings.ipynb cell 14, ipynb:199-209):
 * prediction_ranks(emb) for Q questions (a, b, c, d) given as int32 [Q][4] word ids.
 *   normed = emb / (1e-8 + |emb|_2);  pred = normed[b] - normed[a] + normed[c];
 *   rank   = V - #{v : pred . normed[v] < pred . normed[d]} - 1        (int64 [Q])
 * One fused f32 MFMA GEMM [Q x K] x [K x V]; the score matrix never reaches HBM.  Scores are fma
 * chains over ascending k (the oracle restates exactly that); NumPy's BLAS order differs in the last
 * bits, which can move a rank only where another word's score is within rounding of the ground truth.
 * Workspace: vbq_analogy_ranks_workspace_bytes(V, K, Q) bytes of device memory.
 * ---------------------------------------------------------------------------------- */
size_t vbq_analogy_ranks_workspace_bytes(int64_t V, int32_t K, int64_t Q);
int vbq_analogy_ranks_f32(const float *d_emb, int64_t V, int32_t K, const int32_t *d_analogies, int64_t Q,
                          int64_t *d_out_ranks, void *d_workspace, size_t workspace_bytes, void *stream);

/* ----------------------------------------------------------------------------------
 * Image metrics (img-compression/img_comparison_metrics.py:6-220), batches
 * [B][H][W][C], float64 arithmetic as in the reference.
 *   vbq_image_sqerr_u8   per-image integer sum of (a - b)^2 (mse :6-16 = sum / n, psnr :19-33 from it)
 *   vbq_u8_to_f64        widening copy (img.astype(float64), :122-123)
 *   vbq_unit_to_u8_f32   np.clip(np.round(X_hat * 255), 0, 255).astype(np.uint8) of the evaluation loop (utils.py:555) on the
 *                        device: reconstructions in [0, 1] -> the uint8 images the metrics compare (a quarter of the bytes, should
 *                        they go to the host for PIL's colour conversion)
 *   vbq_ssim_scale_f64   one scale of _SSIMForMultiScale (:84-157): 'valid' Gaussian window given as its
 *                        separable factor d_window[size] (size <= 11), constants c1 = (k1 max_val)^2,
 *                        c2 = (k2 max_val)^2; writes mean ssim and mean cs per image.  Direct sums where the
 *                        reference uses fftconvolve: agreement to ~1e-10, not bit-exact.
 *   vbq_downsample2_f64  scipy.ndimage.convolve(im, ones(1,2,2,1)/4, mode='reflect')[:, ::2, ::2, :] (:214-216)
 * ---------------------------------------------------------------------------------- */
int vbq_image_sqerr_u8(const uint8_t *d_img1, const uint8_t *d_img2, int64_t n_images, int64_t n_per_image,
                       int64_t *d_out_sum, void *stream);
int vbq_u8_to_f64(const uint8_t *d_in, int64_t n, double *d_out, void *stream);
int vbq_unit_to_u8_f32(const float *d_in, int64_t n, uint8_t *d_out, void *stream);
size_t vbq_ssim_scale_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t size);
int vbq_ssim_scale_f64(const double *d_im1, const double *d_im2, int32_t B, int32_t H, int32_t W, int32_t C,
                       const double *d_window, int32_t size, double c1, double c2, double *d_out_ssim,
                       double *d_out_cs, void *d_workspace, size_t workspace_bytes, void *stream);
int vbq_downsample2_f64(const double *d_in, int32_t B, int32_t H, int32_t W, int32_t C, double *d_out, void *stream);

/* ----------------------------------------------------------------------------------
 * Fixed bit budgets (img-compression/utils.py:106-208), float64 as there.  Both entry points take the per-level score
 * table d_fhat [N+1][E]: fhat(e, n) = the best score of element e when it gets exactly n bits (the better of the two n-bit
 * neighbours; level 0 = the zero-bit value).  The caller builds it; squash / unsquash / f stay where the caller evaluates them.
 *   vbq_budget_dp_f64        utils.encode_mode_dp (:106-160) for n_rows rows of K coordinates, E = n_rows * K, element
 *                            e = row * K + k: the allocation of EXACTLY `budget` bits over the K coordinates of a row, at most
 *                            N per coordinate, that maximises the sum of the scores.
 *                              T[0][n] = fhat(0, n) for n <= N, -inf for n > N
 *                              T[k][n] = max over m = 0..min(n, N) of fhat(k, m) + T[k-1][n-m]     (one rounded add each)
 *                            the first maximum in ascending m wins (np.argmax, :137); d_out_obj[row] = T[K-1][budget];
 *                            d_out_bits [n_rows][K] follows the back-pointers and coordinate 0 takes the remainder (:156), so a
 *                            row's bits sum to `budget`.  budget == N is the reference's call; budget up to K * N generalises
 *                            it.  A row without any finite allocation has objective -inf and its remainder may exceed N.
 *                            Entries of d_fhat are finite or -inf.  A row that holds a NaN or +inf is outside the contract:
 *                            it is still processed memory-safely, gets bits in [0, N], and sets bit 0 of d_status (u32, may
 *                            be NULL, OR-ed into; zero it first).
 *                            Returns VBQ_ERR_INVALID_ARGUMENT for budget < 0, budget > K * N, N > 52, K < 1 or null pointers
 *                            (checked before any device work); n_rows == 0 returns 0.  One workgroup per row; the
 *                            back-pointers (one byte per (k, n)) stay in LDS when K * (budget+1) bytes fit there beside the
 *                            value rows.  Otherwise they go to d_workspace, one slice of K * (budget+1) bytes per resident
 *                            workgroup: vbq_budget_dp_workspace_bytes gives the size that keeps the chip busy (0 when none is
 *                            needed); any workspace that holds at least one slice is accepted, and the rows are then
 *                            processed in as many rounds as it takes.
 *   vbq_budget_patience_f64  the per-coordinate scan of utils.encode_mode (:186-203): g_0 = fhat_0, g_b = fhat_b - lamb * b
 *                            for b = 1..N; a strictly greater g becomes the best and resets the counter, `patience` (>= 1)
 *                            consecutive non-improvements end the scan.  d_out_bits [E] = the best b, d_out_g [E] = its g
 *                            (the caller folds it: obj = np.add.accumulate(g)[-1]).
 * Added without an ABI version bump: nothing that existed before changed.
 * ---------------------------------------------------------------------------------- */
size_t vbq_budget_dp_workspace_bytes(int64_t n_rows, int32_t K, int32_t N, int32_t budget);
int vbq_budget_dp_f64(const double *d_fhat, int64_t n_rows, int32_t K, int32_t N, int32_t budget, int32_t *d_out_bits,
                      double *d_out_obj, uint32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream);
int vbq_budget_patience_f64(const double *d_fhat, int64_t E, int32_t N, double lamb, int32_t patience, int32_t *d_out_bits,
                            double *d_out_g, void *stream);

/* ----------------------------------------------------------------------------------
 * Fixed-size records: the stored form of rows quantized to one bit budget (vbq_budget_dp_f64 spends exactly total_bits
 * raw bits on every row), vbq_amd/bitstream.py magic "VBQr".  Every row of a file costs the same number of words, so row r
 * is found by one multiplication and decoded without an entropy coder.
 *
 * One record (one row of K coordinates).  A code point of bit length n has rank index q; with k = q + 1: n = N - ctz(k),
 * its code is j = k >> (N - n + 1), an n-bit number, and q = ((2 j + 1) << (N - n)) - 1.  The raw bits do not delimit
 * themselves, so a record stores the lengths at a fixed width W = bit_length(N) (1 for N = 1, 2 for N = 3, 4 for N = 10).
 * Bit i of a record is bit i % 32 of little-endian u32 word i / 32.
 *   length block  coordinate k's length n_k in bits [k W, (k+1) W), least significant bit first
 *   code block    from bit K W: j_k takes n_k bits at K W + sum_{i<k} n_i, least significant bit first; a zero-bit
 *                 coordinate takes nothing
 *   padding       zero bits up to record_words = ceil((K W + total_bits) / 32) words
 * Example: N = 3, K = 3, lengths (2, 0, 1), codes (2, -, 1), total_bits = 3: bytes 92 01 00 00, rank indices 9, 7, 11.
 * A record costs K W + total_bits bits and up to 31 bits of padding: at N = 10 the length fields are 4 bits per coordinate.
 *
 * The file, every field little-endian (version 1):
 *     offset  size      field
 *     0       4         magic b"VBQr"
 *     4       1         version = 1
 *     5       1         N (1..10)
 *     6       1         ndim (>= 1)
 *     7       1         reserved = 0
 *     8       4         C: 1 (one code book) or K (one per column)
 *     12      4         total_bits (0 .. K N)
 *     16      4         record_words (must equal the formula above; at most 8192, so that a record fits in LDS)
 *     20      4         reserved = 0
 *     24      8 * ndim  shape (u64 each, every entry >= 1); rows are the slices along axis 0, K = prod(shape[1:])
 *     ...     4 * C T   the code points, f32 [C][T] in rank order, T = 2^(N+1) - 1, every value finite; then 4 zero bytes
 *                       when C T is odd, so that the records start 8-byte aligned
 *     ...     4 * R * record_words   the records of rows 0 .. R - 1 (u32 words).  Nothing follows them.
 *
 * vbq_records_words       record_words of (K, N, total_bits); 0 for K < 1, N outside 1..10 or total_bits outside [0, K N].
 * vbq_records_pack_u16    d_idx u16 [n_rows][K] rank indices -> d_words u32 [n_rows][record_words].  One wave per row: n and
 *                         j from the index alone, a wave prefix sum of the lengths carried over chunks of 64 coordinates, the
 *                         fields OR-ed into an LDS image, the image written with coalesced stores.  d_status (u32, may be
 *                         NULL, OR-ed into; zero it first): bit 0 an index >= T, bit 1 a row whose lengths do not add up to
 *                         total_bits; such a row gets an all-zero record.
 * vbq_records_unpack_f32  decodes every row (d_row_ids NULL; n_sel ignored) or the n_sel rows d_row_ids lists (int64, any
 *                         order, repeats allowed, each in [0, n_rows): the caller checks the range) to any of d_out_values
 *                         f32 [rows][K] = d_table_sorted[c][q] and d_out_idx u16 [rows][K] = q (either may be NULL; with both
 *                         NULL the call only validates).  d_table_sorted f32 [n_tables][T] in rank order, n_tables = 1 or K
 *                         (column k reads row k).  The records are UNTRUSTED: no read leaves a record, whatever its bits.
 *                         d_status: bit 0 a length field > N, bit 1 lengths that do not add up to total_bits, bit 2 non-zero
 *                         padding, bit 3 a row id outside [0, n_rows).  A row with any bit decodes to zeros.
 * All three check their arguments before any device work (VBQ_ERR_INVALID_ARGUMENT for sizes outside the ranges above or
 * null pointers, VBQ_ERR_UNSUPPORTED for a record above 8192 words); n_rows == 0 or no row to decode returns 0.
 * Added without an ABI version bump: nothing that existed before changed.
 * ---------------------------------------------------------------------------------- */
size_t vbq_records_words(int32_t K, int32_t N, int32_t total_bits);
int vbq_records_pack_u16(const uint16_t *d_idx, int64_t n_rows, int32_t K, int32_t N, int32_t total_bits, uint32_t *d_words,
                         uint32_t *d_status, void *stream);
int vbq_records_unpack_f32(const uint32_t *d_words, int64_t n_rows, int32_t K, int32_t N, int32_t total_bits,
                           const float *d_table_sorted, int32_t n_tables, const int64_t *d_row_ids, int64_t n_sel,
                           float *d_out_values, uint16_t *d_out_idx, uint32_t *d_status, void *stream);

/* ----------------------------------------------------------------------------------
 * Nearest rows (fused top-k): the k rows of a matrix that score highest against each of Q queries, without a decoded copy of
 * the matrix.  This is the one definition every layer shares.
 *   rows      v, V of them (1 <= V < 2^31), K f32 each: the decoded records of a "VBQr" file (vbq_records_topk_f32) or a dense
 *             [V][K] f32 matrix (vbq_topk_f32; the same kernel with a dense row loader).
 *   queries   d_queries f32 [Q][K], taken as given.
 *   raw score s(q, v): the f32 chain acc = fmaf(q_k, v_k, acc) over ascending k from acc = 0 -- what v_mfma_f32_32x32x2_f32
 *             computes, bit for bit.
 *   metric    0 (dot): the score is s.  1 (cosine): the score is __fdiv_rn(s, den_v), den_v = __fadd_rn(1e-8f, sqrtf(sum)), sum
 *             the __fadd_rn / __fmul_rn chain of v_k^2 over ascending k from 0 (the notebook's 1e-8 + norm, as in
 *             vbq_analogy_ranks_f32).  The caller divides the QUERIES by their norms if it wants the cosine proper (the Python
 *             layer does, by 1e-8 + |q| in f32).
 *   order     score descending, then row id ascending; scores compare as IEEE values, so -0.0 == 0.0 and the ids break the
 *             tie.  The result is the first k rows of that total order among the rows not excluded: unique, whatever the grid
 *             or the order of the tiles.
 *   exclusion d_exclude int64 [Q][E], 0 <= E <= 8 (may be NULL when E == 0): a listed row is never returned for that query; a
 *             negative entry (or one >= V) means "none".
 *   outputs   d_out_ids int64 [Q][k], d_out_scores f32 [Q][k], 1 <= k <= 64; with fewer than k eligible rows the tail is id -1
 *             and score -inf.
 *   records   d_words / K / N / total_bits / d_table_sorted / n_tables as in vbq_records_unpack_f32.  The words are UNTRUSTED:
 *             no read leaves the staged records; a record that fails the unpack's checks takes part as a row of zeros (score
 *             +-0) and sets the same bits of d_status (u32, may be NULL, OR-ed into; zero it first): bit 0 a length field > N,
 *             bit 1 lengths that do not add up to total_bits, bit 2 non-zero padding.
 *   non-finite queries or rows: memory-safe, nothing more is promised (a NaN score is never returned).
 *   max_workgroups  launch policy, a per-call argument as above: 0 sizes the row split to the device, n > 0 caps it at n
 *             workgroups per block of 32 queries.  The result does not depend on it.
 *   workspace vbq_topk_workspace_bytes(V, K, Q, k, max_workgroups) bytes of device memory for either call (0 for sizes outside
 *             the ranges above or Q < 1): 12 bytes per (workgroup of the row split, query, result).  No V x K buffer exists at
 *             any point of vbq_records_topk_f32.
 * One workgroup holds 32 queries in LDS and walks tiles of rows; the records are re-decoded once per block of 32 queries, so
 * these calls are for a few queries -- many-query workloads decode once and use vbq_analogy_ranks_f32 or a GEMM.  The tiles
 * must fit 160 KiB of LDS: every K <= 512 does (n_tables 1 or K, any N and total_bits).  That is a guarantee, not the limit
 * -- a shorter record leaves room for a longer row, the dense source fits up to K = 624; a call whose smallest tile does not
 * fit returns VBQ_ERR_UNSUPPORTED and names the limit.  Sizes and pointers are checked before any device work
 * (VBQ_ERR_INVALID_ARGUMENT); Q == 0 returns 0; VBQ_ERR_WORKSPACE for a workspace that is too small.
 * Added without an ABI version bump: nothing that existed before changed.
 * ---------------------------------------------------------------------------------- */
size_t vbq_topk_workspace_bytes(int64_t V, int32_t K, int64_t Q, int32_t k, int32_t max_workgroups);
int vbq_records_topk_f32(const uint32_t *d_words, int64_t n_rows, int32_t K, int32_t N, int32_t total_bits,
                         const float *d_table_sorted, int32_t n_tables, const float *d_queries, int64_t Q, int32_t k,
                         int32_t metric, const int64_t *d_exclude, int32_t E, int64_t *d_out_ids, float *d_out_scores,
                         uint32_t *d_status, int32_t max_workgroups, void *d_workspace, size_t workspace_bytes, void *stream);
int vbq_topk_f32(const float *d_emb, int64_t V, int32_t K, const float *d_queries, int64_t Q, int32_t k, int32_t metric,
                 const int64_t *d_exclude, int32_t E, int64_t *d_out_ids, float *d_out_scores, int32_t max_workgroups,
                 void *d_workspace, size_t workspace_bytes, void *stream);

/* ----------------------------------------------------------------------------------
 * Pooled rows (embedding bags): per output row the sum, mean or max of a short list of rows, without the [n_ids][K] matrix
 * of the listed rows in between.  This is the one definition every layer shares.
 *   rows      v, V of them (V >= 1), K f32 each: the decoded records of a "VBQr" file (vbq_records_bag_f32) or a dense [V][K]
 *             f32 matrix (vbq_bag_f32; the same kernel with a dense row loader, so the two agree bit for bit).
 *   d_ids     int64 [n_ids] (may be NULL when n_ids == 0).
 *   d_offsets int64 [n_bags + 1]: bag b is the entries i in [offsets[b], offsets[b+1]), IN THAT ORDER.
 *   d_weights f32 [n_ids], or NULL.
 *   entries   a negative id is padding: skipped silently, not counted.  An id >= V is skipped, not counted, and sets status
 *             bit 3 (the unpack's "row id outside [0, n_rows)").
 *   mode      0 sum   per coordinate k: acc = +0.0f, then for each counted entry in order acc = __fadd_rn(acc, v_k), or with
 *                     weights acc = __fadd_rn(acc, __fmul_rn(w_i, v_k)): two separately rounded f32 operations, never
 *                     contracted, so NumPy float32 arithmetic reproduces the result bit for bit.
 *             1 mean  the unweighted sum, then __fdiv_rn(acc, (float)count), count the number of counted entries; count == 0
 *                     gives +0.0f.  Weights with mean are an argument error.
 *             2 max   acc is the first counted entry's v_k; a later entry replaces it only where v_k > acc as IEEE values: the
 *                     value met first stays on a tie, -0.0 does not displace +0.0 (nor +0.0 a -0.0 met first).  A bag with no
 *                     counted entry gives +0.0f.  Weights with max are an argument error.
 *   records   d_words / K / N / total_bits / d_table_sorted / n_tables as in vbq_records_unpack_f32.  The words are UNTRUSTED:
 *             no read leaves the staged record; a record that fails the unpack's checks takes part as a row of zeros (it is
 *             counted) and sets the same bits 0-2 of d_status: a length field > N, lengths that do not add up to total_bits,
 *             non-zero padding.
 *   offsets   UNTRUSTED too: each bag's range is clamped into [0, n_ids] and begin > end is an empty bag; either sets status
 *             bit 4.  No read leaves d_ids or d_weights, whatever the offsets hold.
 *   d_out     f32 [n_bags][K]; every row is written, an empty bag gives zeros.  The result does not depend on the grid.
 *   d_status  u32, may be NULL, OR-ed into; zero it first.
 * One wave pools one bag, entry by entry (a fixed order of additions is the definition, so a bag is never split): the calls
 * are for many short bags; a few very long bags run serially.  Per bag the kernel keeps the staged record and two sets of K
 * accumulators in LDS, 4 (record_words + 2 K) bytes, and the one code book beside them where it fits and is re-used enough.
 * That must fit 160 KiB: every K <= 16804 does for any (N, total_bits, n_tables) (ceil(14 K / 32) + 2 K <= 40960 words at
 * N = 10, total_bits = 10 K) -- a guarantee, not the limit: a shorter record leaves room for a longer row, the dense source
 * fits up to K = 20480; a call whose record and accumulators do not fit returns VBQ_ERR_UNSUPPORTED and names the limit.
 * Sizes, the mode and null pointers are checked before any device work (VBQ_ERR_INVALID_ARGUMENT, also for weights with mode
 * 1 or 2); n_bags == 0 returns 0; n_ids == 0 with n_bags > 0 writes zeros.
 * Added without an ABI version bump: nothing that existed before changed.
 * ---------------------------------------------------------------------------------- */
int vbq_records_bag_f32(const uint32_t *d_words, int64_t n_rows, int32_t K, int32_t N, int32_t total_bits,
                        const float *d_table_sorted, int32_t n_tables, const int64_t *d_ids, int64_t n_ids,
                        const int64_t *d_offsets, int64_t n_bags, const float *d_weights, int32_t mode, float *d_out,
                        uint32_t *d_status, void *stream);
int vbq_bag_f32(const float *d_emb, int64_t V, int32_t K, const int64_t *d_ids, int64_t n_ids, const int64_t *d_offsets,
                int64_t n_bags, const float *d_weights, int32_t mode, float *d_out, uint32_t *d_status, void *stream);

/* ----------------------------------------------------------------------------------
 * Window decode: a box of one latent file in segments (vbq_amd/bitstream.py, magic "VBQb"), or the same-sized boxes of
 * many files, in ONE launch, straight from the packed payloads into channel-last f32 values -- the latent-side counterpart
 * of vbq_rans_decode_values_f32 with a table per (file, channel) and several files per launch.
 *   d_payload  u16 [n_words]: the payloads of all files, concatenated in file order.
 *   d_sizes    u16 [M]: all files' segment sizes, concatenated in the same order; d_offsets int64 [M] their exclusive prefix
 *              sum (vbq_rans_segment_offsets_u16 over the concatenation), so that an offset addresses d_payload directly.
 *   d_files    int64 [n_files][8], per file: seg_base, n, D1, D2, a0, a1, a2, table.  A file's stream is n symbols per
 *              channel, n = D0 D1 D2; row b = (i0 D1 + i1) D2 + i2.  Segment g of channel c is entry seg_base + c nseg_f + g
 *              of d_sizes / d_offsets, nseg_f = ceil(n / seg).  The box of the file is [a0, a0 + w0) x [a1, a1 + w1) x
 *              [a2, a2 + w2); its extents w0, w1, w2 are the same for every file.  `table` picks the block of d_freq (the
 *              file's lambda).
 *   d_segs     int32 [n_files][n_sel]: per file the segment ids within a stream to decode (the same for every channel), any
 *              order; -1 is padding and skipped silently.
 *   d_channels int32 [n_ch_sel]: the channels to decode, any order, repeats allowed; NULL = all n_ch in order (n_ch_sel must
 *              then be n_ch).
 *   d_freq     u16 [n_tables][n_ch][T], T = 2^(N+1) - 1, every row summing to 2^15; d_values f32 [n_ch][T], the sorted code
 *              points.
 *   d_out      f32 [n_files][w0][w1][w2][n_ch_sel].  One lane decodes one listed segment in full, first symbol to last (so
 *              the end-state check holds as in vbq_rans_decode_u16), and for every symbol inside the box stores
 *              d_values[c][symbol] at d_out[f][i0 - a0][i1 - a1][i2 - a2][j], j the channel's place in d_channels.
 *              Positions of the box that no listed segment covers are left untouched.
 *   d_status   u32 [n_files], may be NULL, OR-ed into; zero it first.  Per file: bits 0 - 3 as vbq_rans_decode_u16 (a segment
 *              whose words do not lie in [0, n_words) counts as bit 0); bit 5 (32) a listed id outside [0, nseg_f), or
 *              seg_base + c nseg_f + g outside [0, M); bit 7 (128) an inconsistent descriptor -- n not a multiple of D1 D2,
 *              a box outside the dimensions, `table` outside [0, n_tables) -- or a channel outside [0, n_ch): nothing of that
 *              file is written.  Segments with bits 0 / 3 write zeros at their positions inside the box; with bits 1 / 2
 *              what the segment wrote is meaningless.
 * Payload, sizes and offsets are UNTRUSTED, with the rules of vbq_rans_decode_values_f32: no read leaves [off, off + size)
 * within [0, n_words), no write leaves d_out, every decoded symbol is below T.
 * Checked before any device work (VBQ_ERR_INVALID_ARGUMENT): n_files <= 65535, n_ch_sel <= 65535, seg in 1..65533, N in
 * 1..10, n_ch >= 1, n_tables >= 1, every other size >= 0, an output whose byte count fits in 63 bits, no null pointer
 * (d_channels, d_status and, with n_words == 0, d_payload excepted).  n_files == 0, n_sel == 0, n_ch_sel == 0 or an empty
 * box return VBQ_OK with no launch.
 * Added without an ABI version bump: nothing that existed before changed.
 * ---------------------------------------------------------------------------------- */
int vbq_rans_decode_window_f32(const uint16_t *d_payload, int64_t n_words, const uint16_t *d_sizes, const int64_t *d_offsets,
                               int64_t M, const int64_t *d_files, int32_t n_files, const int32_t *d_segs, int32_t n_sel,
                               const int32_t *d_channels, int32_t n_ch_sel, int32_t n_ch, int32_t seg, int32_t N,
                               const uint16_t *d_freq, int32_t n_tables, const float *d_values, int64_t w0, int64_t w1,
                               int64_t w2, float *d_out, uint32_t *d_status, void *stream);

/* ----------------------------------------------------------------------------------
 * Mapped window decode: the window decode for lambda-map files (vbq_amd/bitstream.py, magic "VBQm") and files in segments
 * at one lambda ("VBQb") together -- the class-mapped twin of vbq_rans_decode_window_f32, with the same geometry and work
 * split (blocks of 64 listed segments x selected channel x file, one lane per listed segment, decoded in full).  Every
 * argument it shares with that call means what it means there; what differs:
 *   d_files    int64 [n_files][16], per file: seg_base, n, D1, D2, a0, a1, a2 as there; P, the classes of the file's palette
 *              (1..4, at most max_classes); table[0..3], the blocks of d_freq of classes 0..3 (those at p >= P are unused,
 *              = 0); cls_base, the byte offset of the file's class block inside d_cls, or -1: every position has class 0;
 *              three reserved fields, = 0.  Symbol i of channel c pops from the row d_freq[table[class of position i]][c].
 *   d_cls      u8 [cls_bytes], aligned to 8 bytes: the class blocks as the files store them -- 2 bits per position, position
 *              b of a file in byte cls_base + b / 4 at bits 2 (b % 4), a block 8 ceil(n / 32) bytes long.  Nothing is
 *              unpacked: a lane reads one aligned 64-bit word per 32 symbols, the first one from the bit its segment starts
 *              at.  May be NULL when cls_bytes == 0 (every file then has cls_base == -1).
 *   max_classes  the largest P of the launch, 1..4: it sizes the tables in LDS, 8192 + 8196 max_classes bytes per
 *              workgroup (per class c[0..T] and the 2048 search starts; the code points once, they do not depend on lambda).
 *              A file with a smaller P stages only its own tables.
 *   d_status   u32 [n_files]: bits 0 - 3 and bit 5 (32) as vbq_rans_decode_window_f32; bit 6 (64) a class >= P met while
 *              decoding -- it is compared with P before it indexes anything, and the segment writes zeros from there on, as a
 *              starved one does; bit 7 (128) as there, and also P outside [1, max_classes], a table[p], p < P, outside
 *              [0, n_tables), or a cls_base that is neither -1 nor a multiple of 8 with cls_base >= 0 and cls_base +
 *              8 ceil(n / 32) <= cls_bytes: nothing of that file is written.  The values of a file whose status is non-zero
 *              are unspecified; every store still lies inside that file's box.
 * A file with P == 1 and cls_base == -1 decodes bit for bit as vbq_rans_decode_window_f32 does with table = table[0].
 * Payload, sizes, offsets, descriptors, id lists and class blocks are UNTRUSTED: the rules of vbq_rans_decode_window_f32, and
 * no read leaves [0, cls_bytes) of d_cls.
 * Checked before any device work (VBQ_ERR_INVALID_ARGUMENT): what vbq_rans_decode_window_f32 checks, max_classes in 1..4,
 * cls_bytes a multiple of 8 and >= 0; then, unless there is nothing to launch, d_cls non-null when cls_bytes > 0 and aligned
 * to 8 bytes.
 * Added without an ABI version bump: nothing that existed before changed.
 * ---------------------------------------------------------------------------------- */
int vbq_rans_map_decode_window_f32(const uint16_t *d_payload, int64_t n_words, const uint16_t *d_sizes, const int64_t *d_offsets,
                                   int64_t M, const int64_t *d_files, int32_t n_files, const int32_t *d_segs, int32_t n_sel,
                                   const int32_t *d_channels, int32_t n_ch_sel, int32_t n_ch, int32_t seg, int32_t N,
                                   const uint16_t *d_freq, int32_t n_tables, const float *d_values, const uint8_t *d_cls,
                                   int64_t cls_bytes, int32_t max_classes, int64_t w0, int64_t w1, int64_t w2, float *d_out,
                                   uint32_t *d_status, void *stream);

/* ----------------------------------------------------------------------------------
 * Batch encode: every segment of MANY latent files in segments (vbq_amd/bitstream.py, magic "VBQb") in ONE launch -- the
 * writer's counterpart of the window decode.  vbq_rans_encode_u16 gives a workgroup 64 consecutive segments of one stream;
 * a small file has a few segments per channel and leaves most lanes idle.  Here the caller lists the work as items
 * (file, segment) in blocks of 64 that share a frequency table, and a workgroup codes one block of one channel: its lanes take
 * segments of different files.
 *   d_idx      u16 [n_idx]: the rank indices of all files.  Symbol i of channel c of file f is
 *              d_idx[idx_base_f + c * idx_stride_f + i], 0 <= i < n_f.
 *   d_files    int64 [n_files][6], per file: idx_base, idx_stride, n, seg_base, table, 0.  The file has n symbols per channel in
 *              nseg_f = ceil(n / seg) segments; `table` picks the block of d_freq (the file's lambda); the last field is
 *              reserved.
 *   d_items    int32 [n_items][2]: (file, segment within a stream), n_items a multiple of 64.  Items 64 b .. 64 b + 63 are block
 *              b; the files of one block must share one `table` (the block's table is that of its first item whose file names a
 *              valid one).  An item with file == -1 is padding and skipped silently.  Every (file, segment) to be coded appears
 *              once; the same item serves every channel.
 *   d_freq     u16 [n_tables][n_ch][T], T = 2^(N+1) - 1, every entry >= 1, every row summing to 2^15.
 *   d_canon    u16 [n_ch][T] or NULL.  Given: symbol d_canon[c][idx] is coded instead of idx (the canonical rank of a run of
 *              equal code points); the map is applied once to the staged table, not per symbol.  An entry outside the table
 *              counts as 0.
 *   d_words    u16 [M][seg + 2], d_sizes u32 [M].  Segment g of channel c of file f goes to slot seg_base_f + c * nseg_f + g:
 *              its words and its size are exactly what vbq_rans_encode_u16 writes for the same symbols with the row
 *              d_freq[table_f][c] -- same state machine, same emission order, final state low half then high half; an index
 *              outside the table is coded as symbol 0.  Slots that no item names, and the words of a slot past its size, are
 *              left untouched.  With seg_base the file-major exclusive sum of n_ch * nseg_f, ONE
 *              vbq_rans_pack_u16(d_words, d_sizes, n_streams = 1, n = M * seg, seg, ...) packs all files, in file order.
 *   d_status   u32 [n_files], may be NULL, OR-ed into; zero it first.  Bit 7 (128) for a file:
 *                of the descriptor -- `table` outside [0, n_tables), n < 1, symbols of some channel outside [0, n_idx), slots
 *                outside [0, M): every item of the file finds the same, so nothing of that file is written;
 *                of one item -- a segment id outside [0, nseg_f), or a file whose table is not the block's: that item writes
 *                nothing.
 *              An item whose file id lies outside [0, n_files) (other than -1) writes nothing and sets bit 7 of word 0: it has
 *              no word of its own.
 * Descriptors and items are range-checked on the device, without overflow, before anything is indexed with them.  Index loads
 * are 16 bytes wide where a segment's address allows it and 2 bytes wide for an unaligned head or tail: the words do not depend
 * on the alignment.
 * Checked before any device work (VBQ_ERR_INVALID_ARGUMENT): n_files <= 65535, n_ch <= 65535, seg in 1..65533, N in 1..10,
 * n_tables >= 1, every size >= 0, n_items a multiple of 64, M * (seg + 2) words addressable, no null pointer (d_canon and
 * d_status excepted).  n_files == 0, n_items == 0 or n_ch == 0 return VBQ_OK with no launch.
 * Added without an ABI version bump: nothing that existed before changed.
 * ---------------------------------------------------------------------------------- */
int vbq_rans_encode_files_u16(const uint16_t *d_idx, int64_t n_idx, const int64_t *d_files, int32_t n_files,
                              const int32_t *d_items, int64_t n_items, int32_t n_ch, int32_t seg, int32_t N,
                              const uint16_t *d_freq, int32_t n_tables, const uint16_t *d_canon, uint16_t *d_words,
                              uint32_t *d_sizes, int64_t M, uint32_t *d_status, void *stream);

/* ----------------------------------------------------------------------------------
 * Batch sizes: the coded length of MANY latent files in segments at SEVERAL lambdas in ONE launch -- the sizes-only counterpart
 * of the batch encode, for rate control over a batch.  vbq_rans_sizes_u16 gives a workgroup 64 consecutive segments of one
 * stream; here the caller lists the work as items (file, segment) in blocks of 64 and a workgroup sizes one block of one
 * channel at one lambda.  Every file is sized at every lambda.
 *   d_idx      u16 [n_idx]: the rank indices of all files at all lambdas, one plane of lambda_stride indices per lambda.
 *              Symbol i of channel c of file f at lambda l is d_idx[l * lambda_stride + idx_base_f + c * idx_stride_f + i],
 *              0 <= i < n_f.
 *   d_files    int64 [n_files][6], the batch encoder's descriptors: idx_base, idx_stride and n are read; seg_base, table and
 *              the reserved field are ignored.  The file has nseg_f = ceil(n / seg) segments per channel.
 *   d_items    int32 [n_items][2]: (file, segment within a stream), n_items a multiple of 64.  Items 64 b .. 64 b + 63 are block
 *              b; the files of a block need share nothing.  An item with file == -1 is padding and skipped silently.  The same
 *              item serves every channel and every lambda.
 *   d_freq     u16 [n_lambda][n_ch][T], T = 2^(N+1) - 1, every entry >= 1, every row summing to 2^15.
 *   d_canon    u16 [n_ch][T] or NULL, as in the batch encode: symbol d_canon[c][idx] is sized instead of idx; the map is
 *              applied once to the staged table.  An entry outside the table counts as 0.
 *   d_totals   u64 [n_lambda][n_files], ADDED to: zero it first.  d_totals[l][f] grows by the size in 16-bit words (the
 *              renormalisation words + the two words of the final state) of every listed segment of every channel of file f,
 *              coded with the row d_freq[l][c]: exactly the d_sizes entry vbq_rans_encode_files_u16 and vbq_rans_sizes_u16
 *              give for the same symbols; an index outside the table is coded as symbol 0.  Integer adds commute: the result
 *              does not depend on scheduling.
 *   d_status   u32 [n_files], may be NULL, OR-ed into; zero it first.  Bit 7 (128) for a file:
 *                of the descriptor -- n < 1, or symbols of some channel outside [0, lambda_stride): nothing of that file is
 *                added;
 *                of one item -- a segment id outside [0, nseg_f): that item adds nothing.
 *              An item whose file id lies outside [0, n_files) (other than -1) adds nothing and sets bit 7 of word 0.
 * Descriptors and items are range-checked on the device, without overflow, before anything is indexed with them.  Index loads
 * are 16 bytes wide where a segment's address allows it and 2 bytes wide for an unaligned head or tail.
 * Checked before any device work (VBQ_ERR_INVALID_ARGUMENT): n_files <= 65535, n_ch <= 65535, seg in 1..65533, N in 1..10,
 * n_lambda in 1..65535, every size >= 0, n_items a multiple of 64, n_lambda * lambda_stride <= n_idx, no null pointer (d_canon
 * and d_status excepted).  n_files == 0, n_items == 0 or n_ch == 0 return VBQ_OK with no launch.
 * Added without an ABI version bump: nothing that existed before changed.
 * ---------------------------------------------------------------------------------- */
int vbq_rans_sizes_files_u16(const uint16_t *d_idx, int64_t n_idx, int64_t lambda_stride, const int64_t *d_files,
                             int32_t n_files, const int32_t *d_items, int64_t n_items, int32_t n_ch, int32_t seg, int32_t N,
                             const uint16_t *d_freq, int32_t n_lambda, const uint16_t *d_canon, uint64_t *d_totals,
                             uint32_t *d_status, void *stream);

/* ----------------------------------------------------------------------------------
 * Mapped batch encode: every segment of MANY lambda-map files (vbq_amd/bitstream.py, magic "VBQm") in ONE launch -- the batch
 * encode with a frequency table per symbol, and the writer's counterpart of the mapped window decode.
 * vbq_rans_map_encode_u16 gives a workgroup 64 consecutive segments of one stream and stages up to four tables for them; a
 * small file leaves most lanes idle.  Here the caller lists the work as items (file, segment) in blocks of 64 that share a
 * PALETTE -- an ordered list of 1..4 blocks of d_freq, one per class --, and a workgroup codes one block of one channel: it
 * stages the palette's tables once and its lanes take segments of different files, each following its own file's classes.
 *   d_idx      u16 [n_idx]: the rank indices of all files, one plane per class of a file's palette.  Symbol i of channel c of
 *              file f is d_idx[idx_base_f + cls * plane_stride_f + c * idx_stride_f + i] with cls = d_cls[cls_base_f + i],
 *              0 <= i < n_f.  plane_stride_f == 0 reads every class from one plane.
 *   d_cls      u8 [n_cls]: the class bytes, one per position of a file, shared by its channels.  A class byte >= P of the
 *              file's palette is coded as class 0, as vbq_rans_map_encode_u16 does: the caller checks its map.
 *   d_files    int64 [n_files][8], per file: idx_base, idx_stride, plane_stride, n, seg_base, palette, cls_base, 0.  The file has
 *              n symbols per channel in nseg_f = ceil(n / seg) segments; `palette` picks the row of d_palettes; the last field
 *              is reserved.
 *   d_palettes int32 [n_palettes][4]: per palette the blocks of d_freq of its classes, class 0 first; the first -1 ends the row
 *              (P = the entries before it, 1..4; what follows it is not read).
 *   max_classes  the largest P of the palettes in use, 1..4: the launch's dynamic LDS is max_classes tables of 8 KB (at most 32 KB
 *              of the CU's 160 KiB).  A palette with more classes is refused as a defective one.
 *   d_items    int32 [n_items][2]: (file, segment within a stream), exactly as in "Batch encode" with the palette in the place of
 *              the table: n_items a multiple of 64, the files of one block share one `palette` (the block's palette is that of
 *              its first item whose file names a valid one), file == -1 is padding and skipped silently.
 *   d_freq     u16 [n_tables][n_ch][T], T = 2^(N+1) - 1, every entry >= 1, every row summing to 2^15.
 *   d_canon    u16 [n_ch][T] or NULL, as in "Batch encode": applied once to every staged table, not per symbol.
 *   d_words    u16 [M][seg + 2], d_sizes u32 [M].  Segment g of channel c of file f goes to slot seg_base_f + c * nseg_f + g:
 *              its words and its size are exactly what vbq_rans_map_encode_u16 writes for the same symbols, classes and
 *              palette -- and, for a file whose classes are all p, what vbq_rans_encode_files_u16 writes with the table
 *              palette[p]; an index outside the table is coded as symbol 0.  Slots that no item names, and the words of a slot
 *              past its size, are left untouched.  With seg_base the file-major exclusive sum of n_ch * nseg_f, ONE
 *              vbq_rans_pack_u16(d_words, d_sizes, n_streams = 1, n = M * seg, seg, ...) packs all files, in file order.
 *   d_status   u32 [n_files], may be NULL, OR-ed into; zero it first.  Bit 7 (128) for a file:
 *                of the descriptor -- `palette` outside [0, n_palettes); a palette row whose first entry is -1, with an entry
 *                before its first -1 outside [0, n_tables), or with more than max_classes classes; n < 1; symbols of some plane
 *                and channel outside [0, n_idx); classes outside [0, n_cls); slots outside [0, M): every item of the file
 *                finds the same, so nothing of that file is written;
 *                of one item -- a segment id outside [0, nseg_f), or a file whose palette is not the block's: that item writes
 *                nothing.
 *              An item whose file id lies outside [0, n_files) (other than -1) writes nothing and sets bit 7 of word 0: it has
 *              no word of its own.
 * vbq_rans_map_sizes_files_u16: the d_sizes of vbq_rans_map_encode_files_u16 for the same arguments, without the words.
 * Descriptors, palettes and items are range-checked on the device, without overflow, before anything is indexed with them.
 * Eight classes are read in one 8-byte load where a segment's class address allows it and, when the eight agree and that class's
 * plane is 16-byte aligned there, their symbols in one 16-byte load; narrow loads otherwise: words and sizes do not depend on
 * the alignment.
 * Checked before any device work (VBQ_ERR_INVALID_ARGUMENT): n_files <= 65535, n_ch <= 65535, seg in 1..65533, N in 1..10,
 * n_tables >= 1, n_palettes >= 1, max_classes in 1..4, every size >= 0 (n_cls too), n_items a multiple of 64, M * (seg + 2) words
 * addressable, no null pointer (d_canon and d_status excepted).  n_files == 0, n_items == 0 or n_ch == 0 return VBQ_OK with no
 * launch.
 * Added without an ABI version bump: nothing that existed before changed.
 * ---------------------------------------------------------------------------------- */
int vbq_rans_map_encode_files_u16(const uint16_t *d_idx, int64_t n_idx, const uint8_t *d_cls, int64_t n_cls,
                                  const int64_t *d_files, int32_t n_files, const int32_t *d_palettes, int32_t n_palettes,
                                  int32_t max_classes, const int32_t *d_items, int64_t n_items, int32_t n_ch, int32_t seg,
                                  int32_t N, const uint16_t *d_freq, int32_t n_tables, const uint16_t *d_canon,
                                  uint16_t *d_words, uint32_t *d_sizes, int64_t M, uint32_t *d_status, void *stream);
int vbq_rans_map_sizes_files_u16(const uint16_t *d_idx, int64_t n_idx, const uint8_t *d_cls, int64_t n_cls,
                                 const int64_t *d_files, int32_t n_files, const int32_t *d_palettes, int32_t n_palettes,
                                 int32_t max_classes, const int32_t *d_items, int64_t n_items, int32_t n_ch, int32_t seg,
                                 int32_t N, const uint16_t *d_freq, int32_t n_tables, const uint16_t *d_canon, uint32_t *d_sizes,
                                 int64_t M, uint32_t *d_status, void *stream);

/* ----------------------------------------------------------------------------------
 * Mapped batch rates: the coded length of MANY lambda-map files under SEVERAL candidate palettes in ONE launch -- rate control
 * over lambda maps.  "Batch sizes" with a frequency table per symbol, and vbq_rans_map_sizes_files_u16 with a candidate axis:
 * the caller solves every distinct lambda of its candidates ONCE into one plane of indices per lambda, and a candidate is a
 * list of 1..4 of those planes, one per class.  The work is listed as items (file, segment) in blocks of 64; a workgroup
 * sizes one block of one channel under one candidate: it stages the candidate's tables once and its lanes take segments of
 * different files, each following its own file's classes.  Every file is sized under every candidate.
 *   d_idx      u16 [n_idx]: the rank indices of all files at all lambdas, one plane of lambda_stride indices per lambda.
 *              Symbol i of channel c of file f under candidate k is d_idx[t * lambda_stride + idx_base_f + c * idx_stride_f + i]
 *              with t = d_palettes[k][cls] and cls = d_cls[cls_base_f + i], 0 <= i < n_f.
 *   d_cls      u8 [n_cls]: the class bytes, one per position of a file, shared by its channels and by all candidates.  A class
 *              byte >= P of the candidate is coded as class 0, as in "Mapped batch encode": the caller checks its maps.
 *   d_files    int64 [n_files][8], the mapped batch encoder's descriptors: idx_base, idx_stride, n and cls_base are read;
 *              plane_stride, seg_base, palette and the reserved field are ignored (a plan with every file in one palette group
 *              serves).  The file has nseg_f = ceil(n / seg) segments per channel.
 *   d_palettes int32 [n_palettes][4]: per candidate the planes of d_idx -- and the blocks of d_freq -- of its classes, class 0
 *              first; the first -1 ends the row (P = the entries before it, 1..4; what follows it is not read).  Candidates may
 *              share planes, and the same planes in another order are another candidate.
 *   max_classes  the largest P of the candidates, 1..4: the launch's dynamic LDS is max_classes tables of 8 KB (at most 32 KB).
 *   d_items    int32 [n_items][2]: (file, segment within a stream), n_items a multiple of 64, exactly as in "Batch sizes": the
 *              files of a block need share nothing, file == -1 is padding and skipped silently, and the same item serves
 *              every channel and every candidate.
 *   d_freq     u16 [n_lambda][n_ch][T], T = 2^(N+1) - 1, every entry >= 1, every row summing to 2^15: block t belongs to plane t.
 *   d_canon    u16 [n_ch][T] or NULL, as in "Batch encode": applied once to every staged table, not per symbol.
 *   d_totals   u64 [n_palettes][n_files], ADDED to: zero it first.  d_totals[k][f] grows, per listed segment and channel, by
 *              exactly the d_sizes entry vbq_rans_map_sizes_files_u16 writes for the same symbols, classes and palette (the
 *              renormalisation words + the two words of the final state); an index outside the table is coded as symbol 0.
 *              One 64-bit atomic add per (candidate, channel, item); integer adds commute: the result does not depend on
 *              scheduling.
 *   d_status   u32 [n_files], may be NULL, OR-ed into; zero it first.  Bit 7 (128) for a file:
 *                of the descriptor -- n < 1; symbols of some plane t < n_lambda and some channel outside [0, n_idx), that is
 *                idx_base < 0, idx_stride < 0 or idx_base + (n_ch - 1) * idx_stride + n > n_idx - (n_lambda - 1) *
 *                lambda_stride; classes outside [0, n_cls): nothing of that file is added, under any candidate;
 *                of one item -- a segment id outside [0, nseg_f): that item adds nothing.
 *              An item whose file id lies outside [0, n_files) (other than -1) adds nothing and sets bit 7 of word 0.
 *              A defective candidate row -- a first entry of -1, an entry before the first -1 outside [0, n_lambda), or more
 *              classes than max_classes -- sets bit 7 of every listed file of its blocks and adds nothing to its row of
 *              d_totals; the other rows are not affected.
 * Descriptors, candidate rows and items are range-checked on the device, without overflow, before anything is indexed with
 * them.  A lane walks its segment exactly as in "Mapped batch encode" (one copy of the device code serves both): eight classes
 * per 8-byte load where the class address allows it and, when the eight agree and that class's plane is 16-byte aligned there,
 * their symbols in one 16-byte load; narrow loads otherwise: the totals do not depend on the alignment.
 * Checked before any device work (VBQ_ERR_INVALID_ARGUMENT): n_files <= 65535, n_ch <= 65535, seg in 1..65533, N in 1..10,
 * n_lambda in 1..65535, n_palettes in 1..65535, max_classes in 1..4, every size >= 0 (n_cls and lambda_stride too), n_items a
 * multiple of 64, n_lambda * lambda_stride <= n_idx (tested without forming the product), no null pointer (d_canon and d_status
 * excepted).  n_files == 0, n_items == 0 or n_ch == 0 return VBQ_OK with no launch.
 * Added without an ABI version bump: nothing that existed before changed.
 * ---------------------------------------------------------------------------------- */
int vbq_rans_map_rates_files_u16(const uint16_t *d_idx, int64_t n_idx, int64_t lambda_stride, const uint8_t *d_cls, int64_t n_cls,
                                 const int64_t *d_files, int32_t n_files, const int32_t *d_palettes, int32_t n_palettes,
                                 int32_t max_classes, const int32_t *d_items, int64_t n_items, int32_t n_ch, int32_t seg,
                                 int32_t N, const uint16_t *d_freq, int32_t n_lambda, const uint16_t *d_canon,
                                 uint64_t *d_totals, uint32_t *d_status, void *stream);

/* ----------------------------------------------------------------------------------
 * Compact batch: the parts of MANY compact latent files (vbq_amd/bitstream.py, magic "VBQc") sized, written or read in ONE
 * launch each.  vbq_rans_il_sizes_u16 / _encode_u16 / _decode_u16 give a wave one part of ONE tensor: a small file has a few
 * parts, so a few waves run and the call takes the time of one wave's steps.  Here the caller lists the work as items
 * (file, part) and a wave (a workgroup of 64) takes one item: the parts of all files run side by side.  The format and the
 * coder are those of vbq_rans_il_encode_u16 (one copy of the device code serves both); the three calls share one descriptor
 * and one item list, so one plan serves writer and reader.
 *   d_idx      u16 [n_idx]: the rank indices of all files.  A file has n_ch streams of n symbols; symbol i of stream c of file
 *              f is d_idx[idx_base_f + c * idx_stride_f + i], 0 <= i < n_f.
 *   d_files    int64 [n_files][8], per file: idx_base, idx_stride, n, part_base, table, part, word_base, n_words_f.  The first
 *              five fields sit where the batch encoder's descriptor has them, part_base in the place of seg_base.  The file's
 *              n_ch * n symbols in stream-major order are cut every `part` symbols (1 .. 2^24, any value per file) into
 *              P_f = ceil(n_ch * n / part) parts; part p of the file is entry part_base + p of d_sizes / d_offsets; `table`
 *              picks the block of d_freq (the file's lambda); the file's words are d_payload[word_base, word_base +
 *              n_words_f).  The last two fields are the decoder's: the encode-side calls do not read them (an encoder's
 *              offsets are the caller's own, and they are not known when the descriptors are made).
 *   d_items    int32 [n_items][2]: (file, part within the file), in any order, any count: one wave handles one item, a lane is
 *              not an item, so there is no multiple-of-64 rule.  An item with file == -1 is padding and skipped silently.
 *   d_freq     u16 [n_tables][n_ch][T], T = 2^(N+1) - 1, every row summing to 2^15 (the encode side: every entry >= 1).
 *   d_canon    u16 [n_ch][T] or NULL (the encode side), as in the batch encode: symbol d_canon[c][idx] is coded instead of
 *              idx; the map is applied once to the staged table of a run, not per symbol.  An entry outside the table counts
 *              as 0.
 *   d_sizes    u32 [P_all], d_offsets int64 [P_all], d_payload u16 [n_words].
 *   d_status   u32 [n_files], may be NULL, OR-ed into; zero it first.  Per file:
 *                bits 0 - 3 as vbq_rans_il_decode_u16 (the decoder);
 *                bit 4 (16)  the decoder: a part outside the file's words, or the file's last part not ending at word_base +
 *                            n_words_f; the encoder: a part whose [offset, offset + size) leaves [0, n_words) or whose size is
 *                            below 128 -- it is not written;
 *                bit 7 (128) of the descriptor -- `table` outside [0, n_tables), n < 1, `part` outside [1, 2^24], symbols of
 *                            some stream outside [0, n_idx), part_base + P_f outside [0, P_all], or (the decoder) a word range
 *                            outside [0, n_words): every item of the file finds the same, so nothing of that file is read or
 *                            written;
 *                            of one item -- a part id outside [0, P_f): that item does nothing.
 *              An item whose file id lies outside [0, n_files) (other than -1) does nothing and sets bit 7 of word 0: it has no
 *              word of its own.
 * Descriptors and items are range-checked on the device, without overflow, before anything is indexed with them.
 *
 * vbq_rans_il_sizes_files_u16   d_sizes[part_base_f + p] = the words of every listed part: exactly the entry
 *                               vbq_rans_il_sizes_u16 gives for that file alone with the row block d_freq[table_f].  Entries no
 *                               item names are left untouched.
 * vbq_rans_il_encode_files_u16  every listed part backwards from d_offsets[.] + d_sizes[.] into d_payload, so that it begins at
 *                               d_offsets[.] with its 128 state words: exactly the bytes of vbq_rans_il_encode_u16 for that
 *                               file alone.  Sizes and offsets are the caller's own (the sizes call and an exclusive scan) and
 *                               are checked for memory safety only.
 * vbq_rans_il_decode_files_u16  payload, sizes and offsets are UNTRUSTED, with the rules of vbq_rans_il_decode_u16: no read
 *                               leaves a part's [off, off + size), which is checked against the FILE's [word_base, word_base +
 *                               n_words_f) within [0, n_words); every index written is below T; no write leaves the file's own
 *                               index positions inside [0, n_idx).  Writes u16 indices to d_idx at the addresses above;
 *                               positions that belong to no listed part are left untouched.  A part with any status bit
 *                               decodes to zeros; the other parts of the file and the other files decode in full.
 * Checked before any device work (VBQ_ERR_INVALID_ARGUMENT): n_files <= 65535, n_ch in 1..65535, N in 1..10, n_tables >= 1,
 * every size >= 0, n_items <= 2^31 - 1, n_ch * n_idx addressable, no null pointer (d_canon, d_status and, with n_words == 0,
 * d_payload excepted).  n_files == 0 or n_items == 0 return VBQ_OK with no launch.
 * Added without an ABI version bump: nothing that existed before changed.
 *
 * vbq_rans_il_rates_files_u16   the parts of MANY compact files sized at SEVERAL lambdas in ONE launch -- rate control over a
 *                               compact batch.  Every file is sized at every lambda.
 *   d_idx      u16 [n_idx]: one plane of lambda_stride indices per lambda.  Symbol i of stream c of file f at lambda l is
 *              d_idx[l * lambda_stride + idx_base_f + c * idx_stride_f + i].
 *   d_files    int64 [n_files][8], the descriptor above, unchanged: idx_base, idx_stride, n, part_base and part are read;
 *              `table` must be 0 -- the row block of lambda l is d_freq[l], not a table the file names, and any other value is
 *              a bad descriptor (bit 7); the two word fields are not read.
 *   d_items    int32 [n_items][2]: (file, part), any order, any count, file == -1 padding.  The same item serves every lambda.
 *   d_freq     u16 [n_lambda][n_ch][T], every entry >= 1, every row summing to 2^15.   d_canon as above.
 *   d_sizes    u32 [n_lambda][P_all]: entry [l][part_base_f + p] = exactly what vbq_rans_il_sizes_files_u16 gives for that file
 *              alone on plane l with the row block d_freq[l].  Entries no item names are left untouched.  No atomics and no
 *              totals: the result does not depend on scheduling; the host sums a file's parts.
 *   d_status   u32 [n_files], may be NULL, OR-ed into; zero it first.  Bit 7 with the meanings above, but a file's symbols are
 *              checked against its lambda's plane [0, lambda_stride), not against [0, n_idx): a file that fits the whole array
 *              but crosses into the next lambda's plane is refused, at every lambda alike.  An unknown file id other than -1
 *              sets bit 7 of word 0.
 * The grid is (n_items, n_lambda), one wave (a workgroup of 64) per (item, lambda); the coder over a part is the one copy the
 * other calls use.  Checked before any device work (VBQ_ERR_INVALID_ARGUMENT): what the three calls above check (with one
 * table), n_lambda in 1..65535, lambda_stride >= 0, n_lambda * lambda_stride <= n_idx (tested without forming the product),
 * n_lambda * P_all addressable, no null pointer (d_canon and d_status excepted).  n_files == 0 or n_items == 0 return VBQ_OK
 * with no launch.  Added without an ABI version bump: nothing that existed before changed.
 * ---------------------------------------------------------------------------------- */
int vbq_rans_il_sizes_files_u16(const uint16_t *d_idx, int64_t n_idx, const int64_t *d_files, int32_t n_files,
                                const int32_t *d_items, int64_t n_items, int32_t n_ch, int32_t N, const uint16_t *d_freq,
                                int32_t n_tables, const uint16_t *d_canon, uint32_t *d_sizes, int64_t P_all,
                                uint32_t *d_status, void *stream);
int vbq_rans_il_encode_files_u16(const uint16_t *d_idx, int64_t n_idx, const int64_t *d_files, int32_t n_files,
                                 const int32_t *d_items, int64_t n_items, int32_t n_ch, int32_t N, const uint16_t *d_freq,
                                 int32_t n_tables, const uint16_t *d_canon, const uint32_t *d_sizes, const int64_t *d_offsets,
                                 int64_t P_all, uint16_t *d_payload, int64_t n_words, uint32_t *d_status, void *stream);
int vbq_rans_il_decode_files_u16(const uint16_t *d_payload, int64_t n_words, const uint32_t *d_sizes, const int64_t *d_offsets,
                                 int64_t P_all, const int64_t *d_files, int32_t n_files, const int32_t *d_items,
                                 int64_t n_items, int32_t n_ch, int32_t N, const uint16_t *d_freq, int32_t n_tables,
                                 uint16_t *d_idx, int64_t n_idx, uint32_t *d_status, void *stream);
int vbq_rans_il_rates_files_u16(const uint16_t *d_idx, int64_t n_idx, int64_t lambda_stride, const int64_t *d_files,
                                int32_t n_files, const int32_t *d_items, int64_t n_items, int32_t n_ch, int32_t N,
                                const uint16_t *d_freq, int32_t n_lambda, const uint16_t *d_canon, uint32_t *d_sizes,
                                int64_t P_all, uint32_t *d_status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VBQ_H_ */
