// What the two window decoders share on the host -- vbq_rans_window.hip (one table per file) and vbq_rans_map_window.hip (up to
// four, a class per position): the work split and the argument check both entry points make before any device work.
// Contract: include/vbq.h, "Window decode" and "Mapped window decode".
#pragma once
#include "vbq_rans_common.h"

namespace vbq {

constexpr int kWinThreads = 64;                                  // one wave: stage_segment_table scans with wave shuffles alone

// The sizes both entry points accept; `total` = the elements of d_out.
inline int check_window(const char *who, int64_t n_words, int64_t M, int32_t n_files, int32_t n_sel, bool channels, int32_t n_ch_sel,
                        int32_t n_ch, int32_t seg, int32_t N, int32_t n_tables, int64_t w0, int64_t w1, int64_t w2, long long &total) {
    VBQ_REQUIRE(n_words >= 0 && M >= 0 && n_files >= 0 && n_files <= 65535 && n_sel >= 0 && n_ch_sel >= 0 && n_ch_sel <= 65535 &&
                    n_ch >= 1 && seg >= 1 && seg <= 65533 && N >= 1 && N <= 10 && n_tables >= 1 && w0 >= 0 && w1 >= 0 && w2 >= 0,
                VBQ_ERR_INVALID_ARGUMENT,
                "%s: bad sizes n_words=%lld M=%lld n_files=%d n_sel=%d n_ch_sel=%d n_ch=%d seg=%d N=%d "
                "n_tables=%d box=%lld x %lld x %lld", who, (long long)n_words, (long long)M, n_files, n_sel, n_ch_sel, n_ch, seg, N,
                n_tables, (long long)w0, (long long)w1, (long long)w2);
    VBQ_REQUIRE(channels || n_ch_sel == 0 || n_ch_sel == n_ch, VBQ_ERR_INVALID_ARGUMENT,
                "%s: without d_channels every channel is decoded, n_ch_sel=%d must be n_ch=%d", who, n_ch_sel, n_ch);
    total = 0;
    VBQ_REQUIRE(!__builtin_smulll_overflow(w0, w1, &total) && !__builtin_smulll_overflow(total, w2, &total) &&
                    !__builtin_smulll_overflow(total, n_ch_sel, &total) && !__builtin_smulll_overflow(total, n_files, &total) &&
                    total <= INT64_MAX / 4,
                VBQ_ERR_INVALID_ARGUMENT, "%s: an output of %d x %lld x %lld x %lld x %d values is too large", who, n_files,
                (long long)w0, (long long)w1, (long long)w2, n_ch_sel);
    return VBQ_OK;
}

// Blocks of 64 listed segments x selected channel x file.
inline dim3 window_grid(int32_t n_sel, int32_t n_ch_sel, int32_t n_files) {
    return dim3((unsigned)(((int64_t)n_sel + kWinThreads - 1) / kWinThreads), (unsigned)n_ch_sel, (unsigned)n_files);
}

}  // namespace vbq
