/*
 * vbq_budget.h -- C-ABI of the third native library of the VBQ package (libvbq_budget.so): the budget DP of vbq.h solved at
 * many budgets in one forward pass.  The boundary rules are those of vbq.h and vbq_ext.h: plain `extern "C"` functions, `d_*`
 * pointers are DEVICE memory, every other pointer is HOST memory that is read before the call returns, all work is enqueued
 * on the caller's `stream` (a hipStream_t passed as void*; NULL = the default stream) and returns without synchronising,
 * nothing is allocated or copied inside a call, the return value is VBQ_OK or a VBQ_ERR_* code of vbq.h, and
 * vbqb_last_error() gives the text of the calling thread's most recent failure in THIS library (each library keeps one
 * thread-local error string; none sees another's).  A call that returns VBQ_ERR_INVALID_ARGUMENT, VBQ_ERR_UNSUPPORTED or
 * VBQ_ERR_WORKSPACE has enqueued nothing.
 * What a call writes must overlap nothing else it reads or writes: vbq.h, "Buffers".
 */
#ifndef VBQ_BUDGET_H_
#define VBQ_BUDGET_H_

#include "vbq.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VBQB_ABI_VERSION 1

int vbqb_abi_version(void);                 /* 1 */
const char *vbqb_last_error(void);

/* ----------------------------------------------------------------------------------
 * Budget sweep: vbq_budget_dp_f64 at S budgets, and the optimal objective at EVERY budget, from one forward pass.
 * The recurrence of vbq_budget_dp_f64 (vbq.h, "Exact bit budgets"),
 *     T[0][n] = fhat(0, n) (n <= N), -inf (n > N)
 *     T[k][n] = max_{m = 0..min(n, N)} fhat(k, m) + T[k-1][n-m]      one rounded f64 add per candidate, the first maximum
 *                                                                    in ascending m,
 * does not depend on the budget it is run for: a pass over n = 0..width-1 holds every value and every back-pointer that
 * any budget below width needs, and its last row T[K-1][n] is the optimal objective at exactly n bits.
 *   d_fhat    f64, fhat(k, n) of row r at d_fhat[n * n_rows * K + r * K + k]: N, K, the layout and the contract of the entries
 *             (finite or -inf) are those of vbq_budget_dp_f64.
 *   budgets   HOST array of S entries, 0 <= S <= 64, strictly ascending, every entry in [0, K N].  The entries travel to the
 *             kernel by value in the launch arguments: the array may be reused as soon as the call returns.
 *   curve_len in [0, K N + 1]; non-zero needs d_curve, and d_curve != NULL needs it non-zero.
 *   width     max(budgets[S-1] + 1, curve_len): the forward pass runs over n = 0..width-1.
 *   d_out_bits[s][r][k] (i32 [S][n_rows][K]) and d_out_obj[s][r] (f64 [S][n_rows]) equal, bit for bit, what
 *             vbq_budget_dp_f64 writes for row r at budget budgets[s]: the back-pointers are walked from n = budgets[s] down
 *             the coordinates, coordinate 0 takes the remainder, and a row outside the contract gets bits clamped to [0, N].
 *   d_curve[r][n] (f64 [n_rows][curve_len]) = T[K-1][n], the objective vbq_budget_dp_f64 reports for row r at budget n, for
 *             every n < curve_len.  It is NOT monotone in n for arbitrary scores ("exactly n bits", not "at most"), and is
 *             -inf where no allocation of exactly n bits has a finite score.
 *   d_status  u32, may be NULL, OR-ed into; zero it first.  Bit 0: a row held a NaN or +inf.  Every other row stays exact.
 *   S == 0 with a curve is a curve-only pass: no back-pointers are kept, no workspace is needed, and the workgroup's LDS is
 *             the value rows alone.  S == 0 && curve_len == 0, or n_rows == 0, returns 0 with no launch (sizes and budgets are
 *             still checked).
 * Plan: one workgroup per row, 64 / 128 / 256 lanes over n (width <= 64 / <= 128 / above), two f64 value rows [width] and the
 * current and next coordinate's N+1 scores in LDS; with S > 0, one byte of back-pointer per (k, n), in LDS when
 * K * width bytes fit into a CU's 160 KiB beside the rest, otherwise in a slice of d_workspace per resident workgroup, which
 * then loops over rows.  After the last coordinate the lanes store the curve, and lane s < S walks the back-pointers of
 * budgets[s] and stores that budget's bits.
 * vbqb_budget_sweep_workspace_bytes: the workspace for S > 0 at this width, 0 when the back-pointers fit the LDS (or the
 * arguments are refused); a smaller workspace that holds at least one row's back-pointers (K * width bytes rounded up to 16)
 * works with more rounds.
 * Refused before any device work (VBQ_ERR_INVALID_ARGUMENT unless noted, the text names the function and the value):
 * n_rows < 0, K < 1, N outside 0..52, S outside 0..64, curve_len outside [0, K N + 1], budgets == NULL with S > 0, a budget
 * outside [0, K N], budgets not strictly ascending, a null d_fhat / d_out_bits / d_out_obj that the call would use, d_curve and
 * curve_len that disagree, two value rows that do not fit the LDS (VBQ_ERR_UNSUPPORTED), a workspace that holds no row's
 * back-pointers (VBQ_ERR_WORKSPACE).
 * ---------------------------------------------------------------------------------- */
size_t vbqb_budget_sweep_workspace_bytes(int64_t n_rows, int32_t K, int32_t N, int32_t width);
int vbqb_budget_sweep_f64(const double *d_fhat, int64_t n_rows, int32_t K, int32_t N, const int32_t *budgets, int32_t S,
                          int32_t *d_out_bits, double *d_out_obj, double *d_curve, int32_t curve_len, uint32_t *d_status,
                          void *d_workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif  /* VBQ_BUDGET_H_ */
