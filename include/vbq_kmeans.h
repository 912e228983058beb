/*
 * vbq_kmeans.h -- C-ABI of the fourth native library of the VBQ package (libvbq_kmeans.so): the k-means baseline of the image
 * pipeline fitted on the device.  One-dimensional k-means needs neither Lloyd's iteration nor a seed: on sorted samples the
 * optimal clusters are contiguous segments and a dynamic programme finds the global optimum.  The boundary rules are those of
 * vbq.h, vbq_ext.h and vbq_budget.h: plain `extern "C"` functions, `d_*` pointers are DEVICE memory, every other pointer is
 * HOST memory that is read before the call returns, all work is enqueued on the caller's `stream` (a hipStream_t passed as
 * void*; NULL = the default stream) and returns without synchronising, nothing is allocated or copied inside a call, the
 * return value is VBQ_OK or a VBQ_ERR_* code of vbq.h, and vbqk_last_error() gives the text of the calling thread's most
 * recent failure in THIS library (each library keeps one thread-local error string; none sees another's).  A call that returns
 * VBQ_ERR_INVALID_ARGUMENT, VBQ_ERR_UNSUPPORTED or VBQ_ERR_WORKSPACE has enqueued nothing.
 * What a call writes must overlap nothing else it reads or writes: vbq.h, "Buffers".
 */
#ifndef VBQ_KMEANS_H_
#define VBQ_KMEANS_H_

#include "vbq.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VBQK_ABI_VERSION 1

int vbqk_abi_version(void);                 /* 1 */
const char *vbqk_last_error(void);

/* ----------------------------------------------------------------------------------
 * Exact 1-D k-means of C channels at every level count up to Kmax, from one forward pass.
 * A channel is n samples sorted ascending, x[1..n].  The caller hands in (vbq_amd/kmeans1d.py, prefix_sums)
 *     shift   = f64(x[n / 2 + 1])                       the upper median
 *     y[j]    = f64(x[j]) - shift
 *     S1[j]   = y[1] + ... + y[j],  S2[j] = y[1]^2 + ... + y[j]^2,  S1[0] = S2[0] = 0      (f64, j = 0..n)
 * The samples themselves are not an argument: every quantity below is a function of the sums.
 *     cost(i, j) = (S2[j] - S2[i-1]) - s * s / (j - i + 1),  s = S1[j] - S1[i-1]      every operation rounded separately in
 *                  f64; it may come out a few ulp below zero and is not clamped
 *     D[0][0] = 0,  D[q][j] = min_{i = q..j} D[q-1][i-1] + cost(i, j)  (q = 1..Kmax, j = q..n),  A[q][j] = the minimising i
 * EVALUATION ORDER.  The optimal i is monotone in j, and layer q is evaluated by exactly this recursion, which is the
 * definition of every D and A the call reports:
 *     solve(jl, jh, il, ih):  return if jl > jh;  j = (jl + jh) / 2;  scan i ascending over [max(il, q), min(ih, j)] and keep
 *                             the FIRST strict minimum of D[q-1][i-1] + cost(i, j);  D[q][j] = it, A[q][j] = bi;
 *                             solve(jl, j - 1, il, bi);  solve(j + 1, jh, bi, ih)
 *     root: solve(q, n, q, n)
 * The recurrence does not depend on the level count it is run for: the pass at Kmax holds D[q][n] and the back-pointers of
 * every q <= Kmax.
 *   d_S1, d_S2   f64 [C][n + 1];  d_shift f64 [C].
 *   levels       HOST array of S entries, 1 <= S <= 64, strictly ascending, levels[0] >= 1, Kmax = levels[S-1] <= 1024 and
 *                Kmax <= n (as sklearn refuses n_samples < n_clusters).  The entries travel to the kernel by value in the
 *                launch arguments: the array may be reused as soon as the call returns.
 *   Outputs of level s (k = levels[s]) are packed one level after the other: with off(s) = C * (levels[0] + ... + levels[s-1]),
 *   channel c's k entries start at off(s) + c * k; total = C * (levels[0] + ... + levels[S-1]) entries per output.
 *   d_out_starts i32 [total]   the first sample (1-based) of each of the k segments, ascending: the walk j = n, i = A[q][j],
 *                              j = i - 1 for q = k..1 gives the start of segment q
 *   d_out_codes  f64 [total]   shift + (S1[j] - S1[i-1]) / (j - i + 1) of the segment [i, j]: the code points, ascending
 *   d_out_counts i64 [total]   j - i + 1 (written, not added to)
 *   d_out_sse    f64 [C][Kmax] sse[c][q-1] = D[q][n]: the optimal within-cluster sum of squares with q levels, for every q
 *   d_status     u32, may be NULL, OR-ed into; zero it first.  Bit 0: a channel held a NaN or +-inf (its S1[n], S2[n] or
 *                shift is not finite).  That channel's outputs are unspecified but within bounds (starts in [1, n]); every
 *                other channel stays exact.
 *   A level count above the number of distinct values is allowed: zero-cost splits give repeated code points.
 * Plan: one workgroup of 512 lanes per channel (C = 1 runs ONE workgroup: accepted, the layers of a channel are a chain),
 * layers q in sequence; within a layer the recursion depths in sequence with a barrier between them (a node's il / ih are
 * A[q][jl-1] / A[q][jh+1], midpoints of its ancestors, so the nodes of one depth are independent); within a depth one node per
 * lane, except that a node whose scan holds at least 64 candidates is queued and taken by a whole wave, lanes over i, with a
 * reduction that keeps the lowest i among equal minima.  Two f64 value rows and a copy of the channel's S1 and S2 live in LDS
 * when 4 (n + 1) doubles fit beside the queue (n <= 4862); otherwise the value rows live in the workgroup's slice of
 * d_workspace and the sums are read where they are.  The back-pointers, i32 [Kmax][n + 1] per channel in flight, always live in
 * the slice.  After the last layer, lane s < S walks the back-pointers of levels[s].
 * vbqk_kmeans1d_workspace_bytes: the full workspace, one slice per channel in flight (min(C, 2 x compute units)); 0 when the
 * arguments are refused.  A smaller workspace that holds at least one slice works with more rounds: the workgroups loop over
 * the channels.  One slice is 4 Kmax (n + 1) bytes rounded up to 16, plus 16 (n + 1) bytes when n > 4862.
 * Refused before any device work (VBQ_ERR_INVALID_ARGUMENT unless noted, the text names the function and the value):
 * n outside 1..2^30, C < 1, S outside 1..64, levels == NULL, levels[0] < 1, levels not strictly ascending, Kmax > 1024, Kmax > n, a null
 * d_S1 / d_S2 / d_shift / d_out_starts / d_out_codes / d_out_counts / d_out_sse, a workspace that holds no slice
 * or is not 16-byte aligned (VBQ_ERR_WORKSPACE).
 * ---------------------------------------------------------------------------------- */
size_t vbqk_kmeans1d_workspace_bytes(int64_t n, int32_t C, int32_t Kmax);
int vbqk_kmeans1d_f64(const double *d_S1, const double *d_S2, const double *d_shift, int64_t n, int32_t C, const int32_t *levels,
                      int32_t S, int32_t *d_out_starts, double *d_out_codes, int64_t *d_out_counts, double *d_out_sse,
                      uint32_t *d_status, void *d_workspace, size_t workspace_bytes, void *stream);

/* ----------------------------------------------------------------------------------
 * Nearest code point of every channel in one launch: vbq_nearest_code_f64 (vbq.h) per channel.
 *   d_x          f32 [B][C], channel-last;  d_codes f64 [C][k], 1 <= k <= 1024
 *   d_out_index  i32 [B][C], d_out_value f64 [B][C]: for channel c exactly what vbq_nearest_code_f64 returns for the column
 *                d_x[:, c] and the code row d_codes[c]: f64 squared distance (one rounded subtraction, one rounded product), the
 *                FIRST minimum in code-book order; the value is the code point itself.  Either may be NULL.
 *   d_counts     i64 [C][k] or NULL; the number of samples of channel c at code j is ADDED to d_counts[c][j].
 * Plan: workgroups of 256 lanes over (rows, a tile of channels); the tile's code rows sit in LDS.
 * Refused before any device work: B < 0, C < 1, k outside 1..1024, a null d_x or d_codes (with B > 0).  B == 0 returns 0 with
 * no launch.
 * ---------------------------------------------------------------------------------- */
int vbqk_nearest_code_channels_f64(const float *d_x, int64_t B, int32_t C, const double *d_codes, int32_t k,
                                   int32_t *d_out_index, double *d_out_value, int64_t *d_counts, void *stream);

#ifdef __cplusplus
}
#endif

#endif  /* VBQ_KMEANS_H_ */
