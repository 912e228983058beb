/*
 * vbq_ext.h -- C-ABI of the second native library of the VBQ package (libvbq_ext.so): entry points that build on the
 * definitions of vbq.h without being part of libvbq_hip.so.  The boundary rules are those of vbq.h: plain `extern "C"`
 * functions, `d_*` pointers are DEVICE memory, all work is enqueued on the caller's `stream` (a hipStream_t passed as void*;
 * NULL = the default stream) and returns without synchronising, nothing is allocated inside a call, the return value is
 * VBQ_OK or a VBQ_ERR_* code of vbq.h, and vbqx_last_error() gives the text of the calling thread's most recent failure
 * in THIS library (the two libraries keep one thread-local error string each; neither sees the other's).  A call that
 * returns VBQ_ERR_INVALID_ARGUMENT or VBQ_ERR_UNSUPPORTED has enqueued nothing.
 * What a call writes must overlap nothing else it reads or writes: vbq.h, "Buffers".
 */
#ifndef VBQ_EXT_H_
#define VBQ_EXT_H_

#include "vbq.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VBQX_ABI_VERSION 1

int vbqx_abi_version(void);                 /* 1 */
const char *vbqx_last_error(void);

/* ----------------------------------------------------------------------------------
 * Listed rows: the score of each query against the rows the caller names for it, without the [Q M][K] matrix of the
 * listed rows in between -- word-pair similarity (M = 1), reranking of candidates that came from elsewhere, scoring of
 * sampled negatives.  The score is the one of vbq.h, "Nearest rows"; nothing new is defined here.
 *   rows      v, V of them (V >= 1), K f32 each: the decoded records of a "VBQr" file (vbqx_records_scores_f32) or a dense
 *             [V][K] f32 matrix (vbqx_scores_f32; the same kernel with a dense row loader, so the two agree bit for bit).
 *   queries   d_queries f32 [Q][K], taken as given.
 *   d_ids     int64 [Q][M]: pair p = q M + m scores query q against row ids[q][m].
 *   raw score the f32 chain acc = fmaf(q_k, v_k, acc) over ascending k from acc = +0.0f, one rounding per step.
 *   metric    0 (dot): the raw score s.  1 (cosine): __fdiv_rn(s, den_v), den_v = __fadd_rn(1e-8f, sqrtf(sum)), sum the
 *             chain __fadd_rn(sum, __fmul_rn(v_k, v_k)) over ascending k from 0.  The caller divides the QUERIES by their
 *             norms if it wants the cosine proper (the Python layer does, by 1e-8 + |q| in f32).  These are the scores
 *             vbq_records_topk_f32 / vbq_topk_f32 report for the same (query, row), bit for bit.
 *   entries   a negative id is padding: the output is -inf and no status bit is set, so the -1 tail of a search result can
 *             be fed straight back in.  An id >= V gives -inf and sets status bit 3 (the unpack's "row id outside
 *             [0, n_rows)").
 *   records   d_words / K / N / total_bits / d_table_sorted / n_tables as in vbq_records_unpack_f32.  The words are
 *             UNTRUSTED: no read leaves a staged record; a record that fails the unpack's checks takes part as a row of
 *             zeros (score +-0) and sets the same bits 0-2 of d_status: a length field > N, lengths that do not add up to
 *             total_bits, non-zero padding.
 *   d_out     f32 [Q][M]; every element is written, nothing outside it is.
 *   d_status  u32, may be NULL, OR-ed into; zero it first.
 *   non-finite queries or rows: memory-safe, nothing more is promised.
 * One wave scores a group of G consecutive pairs: it stages the G records with one coalesced copy, decodes them one after
 * the other with the unpack's scan into an LDS tile of ranks [G][K | 1] (the odd row stride keeps both the decode's stores,
 * lane -> k, and the chains' loads, lane -> pair, free of bank conflicts), and lane j then walks pair j's chain, looking each
 * code point up as it goes.  A pair is never split and never shares an accumulator, so the result does not depend on how
 * pairs fall into groups.  What hides a record's scan is other waves, so groups are small: G is the largest of 64, 32 and
 * 16 at which tile and staged records stay within 8 KiB, and 8 otherwise (measured: vbqx_scores.hip), which must fit the
 * 160 KiB of a CU: every K <= 3500 does for any (N, total_bits, n_tables).  That is a guarantee, not the limit -- a shorter
 * record leaves room for a longer row (N = 10 at the full budget: up to K = 3549; the dense source: up to K = 5103); a call
 * whose eight pairs do not fit returns VBQ_ERR_UNSUPPORTED and names the limit.  The grid is one workgroup per group: Q M above
 * 2147483647 G is refused.
 * Sizes, the metric and null pointers are checked before any device work (VBQ_ERR_INVALID_ARGUMENT: K < 1, N outside 1..10,
 * total_bits outside [0, K N], n_tables neither 1 nor K, V < 1, Q < 0, M < 0, a metric other than 0 / 1, Q M above the grid
 * limit, a null pointer other than d_status); Q == 0 or M == 0 returns 0 with no launch.
 * ---------------------------------------------------------------------------------- */
int vbqx_records_scores_f32(const uint32_t *d_words, int64_t n_rows, int32_t K, int32_t N, int32_t total_bits,
                            const float *d_table_sorted, int32_t n_tables, const float *d_queries, int64_t Q,
                            const int64_t *d_ids, int64_t M, int32_t metric, float *d_out, uint32_t *d_status, void *stream);
int vbqx_scores_f32(const float *d_emb, int64_t V, int32_t K, const float *d_queries, int64_t Q,
                    const int64_t *d_ids, int64_t M, int32_t metric, float *d_out, uint32_t *d_status, void *stream);

#ifdef __cplusplus
}
#endif

#endif  /* VBQ_EXT_H_ */
