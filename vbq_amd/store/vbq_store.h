/*
 * vbq_store.h -- C-ABI of the fifth native library of the VBQ package (libvbq_store.so): what a set of latent files that stays
 * on the device needs besides the decoders of vbq.h.  The boundary rules are those of vbq.h, vbq_ext.h, vbq_budget.h and
 * vbq_kmeans.h: plain `extern "C"` functions, `d_*` pointers are DEVICE memory, all work is enqueued on the caller's `stream`
 * (a hipStream_t passed as void*; NULL = the default stream) and returns without synchronising, nothing is allocated or copied
 * inside a call, the return value is VBQ_OK or a VBQ_ERR_* code of vbq.h, and vbqs_last_error() gives the text of the calling
 * thread's most recent failure in THIS library.  A call that returns VBQ_ERR_INVALID_ARGUMENT has enqueued nothing.
 * What a call writes must overlap nothing else it reads or writes: vbq.h, "Buffers".
 * The header lives beside its sources (vbq_amd/store): the directory `include` holds the headers of the first four libraries.
 */
#ifndef VBQ_STORE_H_
#define VBQ_STORE_H_

#include "vbq.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VBQS_ABI_VERSION 1

int vbqs_abi_version(void);                 /* 1 */
const char *vbqs_last_error(void);

/* ----------------------------------------------------------------------------------
 * Planned boxes: the descriptors and segment lists that vbq_rans_decode_window_f32 / vbq_rans_map_decode_window_f32 (vbq.h,
 * "Window decode" and "Mapped window decode") read, made ON THE DEVICE from file ids and box origins that live there -- the
 * host never sees which file or which box a sample is.
 *   d_table    int64 [n_files][fields], fields 8 or 16: one row per resident file in exactly the descriptor layout of the
 *              decoder it feeds.  Fields 0..6: seg_base, n, D1, D2, 0, 0, 0; then, with 8 fields, `table`; with 16 fields,
 *              P, table[0..3], cls_base, 0, 0, 0.  The file's geometry is D0 = n / (D1 D2) by D1 by D2, row b = (i0 D1 + i1) D2
 *              + i2.
 *   d_ids      int64 [S]: the file of each sample.  d_origins int64 [S][3]: a0, a1, a2 of each sample's box, whose extents
 *              w0, w1, w2 are those of the call.  Both are UNTRUSTED: they may hold values the host has never seen.
 *   d_desc     int64 [S][fields]: row s is row d_ids[s] of the table with fields 4..6 replaced by the origin.
 *   d_segs     int32 [S][n_sel]: the segments of `seg` symbols that hold at least one row of the box
 *              [a0, a0 + w0) x [a1, a1 + w1) x [a2, a2 + w2), ascending, each once, then -1 up to n_sel: entry for entry
 *              bitstream.box_segments(dims, lo, hi, seg).
 *   d_status   u32 [S], OR-ed into; zero it first.  May not be NULL.
 * A sample is VALID iff 0 <= id < n_files; its row has n >= 0, D1 >= 1, D2 >= 1, D1 D2 representable, n % (D1 D2) == 0 and
 * ceil(n / seg) <= 2^31 - 1 (a segment id is an int32); and 0 <= a_k <= D_k - w_k at all three levels -- written that way an
 * origin of 2^62 cannot overflow.  An invalid sample gets bit 7 (128, the decoders' "inconsistent descriptor"), a list of -1
 * throughout, and the descriptor of row 0 with origin 0 0 0, so that whatever a decoder does with it stays in bounds.  Nothing
 * is read outside d_table, d_ids and d_origins.
 * A list longer than n_sel is cut at n_sel and sets bit 5 (32, the decoders' "segment id out of range"); nothing is written past
 * the row.  With n_sel >= max_listed_segments (vbq_amd/store) that cannot happen.
 * How the list is built: the box is w0 w1 runs of w2 consecutive rows, one per (i0, i1), ascending.  Run r starts at row
 * first_r = (i0 D1 + i1) D2 + a2 and covers the segments lo_r = first_r / seg .. hi_r = (first_r + w2 - 1) / seg; both ends are
 * non-decreasing in r, so run r contributes exactly max(lo_r, hi_{r-1} + 1) .. hi_r, and its place in the list is the
 * exclusive prefix sum of those counts.
 * Plan: workgroups of 256 lanes, one 64-lane wave per sample (a grid-stride loop over samples); the lanes go over the runs in
 * chunks of 64, a wave-wide scan gives the positions, the running position and the last hi carry from chunk to chunk; then
 * the lanes write the -1 tail.  No LDS, no scratch, no atomics: a sample's words are written by its own wave alone.
 * Checked before any device work (VBQ_ERR_INVALID_ARGUMENT): fields in {8, 16}, n_files >= 1, S >= 0, w0, w1, w2 >= 0, seg in
 * 1..65533, n_sel >= 0, no null pointer.  S == 0, an empty box or n_sel == 0 return VBQ_OK with no launch.
 * ---------------------------------------------------------------------------------- */
int vbqs_plan_boxes(const int64_t *d_table, int32_t n_files, int32_t fields, const int64_t *d_ids, const int64_t *d_origins,
                    int64_t S, int64_t w0, int64_t w1, int64_t w2, int32_t seg, int32_t n_sel, int64_t *d_desc, int32_t *d_segs,
                    uint32_t *d_status, void *stream);

#ifdef __cplusplus
}
#endif

#endif  /* VBQ_STORE_H_ */
