// Batches of compact latent files (vbq_amd/bitstream.py, magic "VBQc"): the parts of MANY files sized, written or read in ONE
// launch each.  Contract: include/vbq.h, "Compact batch".
//
// The one-file kernels (vbq_rans_il.hip) give a wave one part of the one tensor: a Kodak-shaped latent at the default part is
// three parts, so three waves run and the time is that of one wave's steps.  Here the host lists the work as items (file, part)
// and a wave takes one item: the parts of all files run side by side.  The coder over a part -- lane mapping, word placement,
// word window, table staging -- is vbq_rans_il_common.h's, the same functions the one-file kernels call: the words and the
// size of a part are the same.  What is new here is only where a part's geometry comes from: a descriptor per file.
#include "vbq_rans_il_common.h"

namespace vbq {
namespace {

constexpr int kIlFields = 8;                                     // idx_base, idx_stride, n, part_base, table, part, word_base, n_words_f
constexpr unsigned kBadFile = 128u;                              // status bit 7
constexpr long kMaxPart = 1L << 24;

// One item: its file's descriptor and its part, checked.  Descriptors and items come from the caller's host plan (the
// decoder's may come from anywhere); every index formed from them is range-checked without overflow before it is used.
struct IlItem {
    long f;                                                      // the file, its status word
    const uint16_t *freq;                                        // the file's row block [n_ch][T]
    long idx_base, stride, n;                                    // symbol i of stream s: idx[idx_base + s * stride + i]
    long a, b;                                                   // the part: symbols [a, b) of the file's n_ch * n
    long slot;                                                   // its entry of d_sizes / d_offsets
    long word_base, n_words_f;                                   // (the decoder's: the file's words)
    bool last;                                                   // the file's last part
};

// false: nothing to do for this item; what was wrong is in status (nothing, for padding).  kWords: the word range of the file
// is checked too (the decoder; the encode side does not read those two fields).  Wave-uniform: every lane reads the same.
template <bool kWords>
__device__ __forceinline__ bool il_open_item(IlItem &it, const int64_t *__restrict__ files, int n_files,
                                             const int32_t *__restrict__ items, long n_idx, long n_ch, int T,
                                             const uint16_t *__restrict__ freq, int n_tables, long P_all, long n_words,
                                             uint32_t *__restrict__ status) {
    const long f = items[2 * (long)blockIdx.x], p = items[2 * (long)blockIdx.x + 1];
    if (f == -1) return false;                                   // padding
    const bool known = f >= 0 && f < n_files;
    bool ok = known;
    if (known) {
        const int64_t *d = files + f * kIlFields;
        const long idx_base = d[0], stride = d[1], n = d[2], part_base = d[3], table = d[4], part = d[5];
        it.f = f, it.idx_base = idx_base, it.stride = stride, it.n = n, it.word_base = d[6], it.n_words_f = d[7];
        // symbols [idx_base + s stride, + n) of every stream s inside [0, n_idx), without forming a sum that could overflow
        // (the host checked that n_ch * n_idx does not)
        ok = table >= 0 && table < n_tables && part >= 1 && part <= kMaxPart && n >= 1 && n <= n_idx && idx_base >= 0 &&
             idx_base <= n_idx - n && stride >= 0 && (n_ch == 1 || stride <= (n_idx - n - idx_base) / (n_ch - 1));
        if (ok) {
            const long total = n_ch * n;
            const long P_f = (total - 1) / part + 1;
            // entries [part_base, part_base + P_f) inside [0, P_all)
            ok = part_base >= 0 && part_base <= P_all && P_f <= P_all - part_base;
            if (kWords)                                          // words [word_base, word_base + n_words_f) inside [0, n_words)
                ok = ok && it.word_base >= 0 && it.word_base <= n_words && it.n_words_f >= 0 &&
                     it.n_words_f <= n_words - it.word_base;
            ok = ok && p >= 0 && p < P_f;                        // (the item's own: the other items of the file go on)
            if (ok) {
                it.a = p * part;
                it.b = it.a + part < total ? it.a + part : total;
                it.slot = part_base + p;
                it.last = p == P_f - 1;
                it.freq = freq + table * n_ch * T;
            }
        }
    }
    if (!ok && status && threadIdx.x == 0) atomicOr(status + (known ? f : 0), kBadFile);   // (an unknown file has no word of its own: word 0)
    return ok;
}

// One wave per item, as k_il_encode codes a part.  kWrite = false: the part's words -> sizes[slot].  kWrite = true: the part
// to payload[offs[slot], + sizes[slot]); sizes and offsets are the caller's own (the kWrite = false pass and a scan) and are
// checked for memory safety only -- a part that would leave [0, n_words) is not written and sets bit 4.
template <bool kWrite>
__global__ void __launch_bounds__(kLanes)
k_il_encode_files(const uint16_t *__restrict__ idx, long n_idx, const int64_t *__restrict__ files, int n_files,
                  const int32_t *__restrict__ items, long n_ch, int T, const uint16_t *__restrict__ freq, int n_tables,
                  const uint16_t *__restrict__ canon, const uint32_t *__restrict__ sizes_in, const int64_t *__restrict__ offs,
                  long P_all, long n_words, uint16_t *__restrict__ payload, uint32_t *__restrict__ sizes_out,
                  uint32_t *__restrict__ status) {
    __shared__ uint32_t fc_l[2048];
    IlItem it;
    if (!il_open_item<false>(it, files, n_files, items, n_idx, n_ch, T, freq, n_tables, P_all, 0L, status)) return;
    long k0 = 0, off = 0;
    if (kWrite) {
        k0 = sizes_in[it.slot], off = offs[it.slot];
        if (k0 < kStateWords || off < 0 || off > n_words - k0) {
            if (status && threadIdx.x == 0) atomicOr(status + it.f, 16u);
            return;
        }
    }
    il_encode_part<kWrite>(idx + it.idx_base, it.stride, it.n, it.a, it.b, T, it.freq, canon, payload, off, k0,
                           kWrite ? nullptr : sizes_out + it.slot, fc_l);
}

// One wave per (item, lambda): the parts of every file sized at SEVERAL lambdas in one launch (rate control over a compact
// batch).  The index array holds one plane of lambda_stride indices per lambda and freq one row block per lambda; an item is
// opened against its lambda's plane alone -- il_open_item with n_idx = lambda_stride and the one table 0 -- so a file that
// crosses into the next plane is refused, at every lambda alike.  The coder over the part is il_encode_part<false>, as above:
// sizes[l][slot] is what k_il_encode_files<false> gives on plane l with the row block freq[l].
__global__ void __launch_bounds__(kLanes)
k_il_rates_files(const uint16_t *__restrict__ idx, long lambda_stride, const int64_t *__restrict__ files, int n_files,
                 const int32_t *__restrict__ items, long n_ch, int T, const uint16_t *__restrict__ freq,
                 const uint16_t *__restrict__ canon, long P_all, uint32_t *__restrict__ sizes, uint32_t *__restrict__ status) {
    __shared__ uint32_t fc_l[2048];
    const long l = blockIdx.y;
    IlItem it;
    if (!il_open_item<false>(it, files, n_files, items, lambda_stride, n_ch, T, freq + l * n_ch * T, 1, P_all, 0L, status)) return;
    il_encode_part<false>(idx + l * lambda_stride + it.idx_base, it.stride, it.n, it.a, it.b, T, it.freq, canon, nullptr, 0L, 0L,
                          sizes + l * P_all + it.slot, fc_l);
}

// One wave per item, as k_il_decode reads a part: sizes, offsets and words are UNTRUSTED.  A part's [off, off + size) is
// checked against the FILE's words, which the descriptor check placed inside [0, n_words); no read leaves it.
__global__ void __launch_bounds__(kLanes)
k_il_decode_files(const uint16_t *__restrict__ payload, long n_words, const uint32_t *__restrict__ sizes,
                  const int64_t *__restrict__ offs, long P_all, const int64_t *__restrict__ files, int n_files,
                  const int32_t *__restrict__ items, long n_ch, int T, const uint16_t *__restrict__ freq, int n_tables,
                  uint16_t *__restrict__ idx, long n_idx, uint32_t *__restrict__ status) {
    __shared__ uint32_t fc_l[2048];
    __shared__ uint16_t c_l[2048 + 2];
    __shared__ uint16_t start[(1 << kPB) / 16];
    IlItem it;
    if (!il_open_item<true>(it, files, n_files, items, n_idx, n_ch, T, freq, n_tables, P_all, n_words, status)) return;
    const long k0 = sizes[it.slot], off = offs[it.slot];
    const long end = it.word_base + it.n_words_f;
    unsigned bad = 0;
    if (k0 < kStateWords || k0 > (it.b - it.a) + kStateWords) bad |= 1u;
    if (off < it.word_base || off > end - k0 || (it.last && off + k0 != end)) bad |= 16u;
    uint16_t *dst = idx + it.idx_base;
    if (!bad) bad = il_decode_part(payload + off, k0, dst, it.stride, it.n, it.a, it.b, T, it.freq, fc_l, c_l, start);
    if (bad) {
        il_zero_part(dst, it.stride, it.n, it.a, it.b);
        if (status && threadIdx.x == 0) atomicOr(status + it.f, bad);
    }
}

// What the entry points check before any device work.
int check_il_files(const char *who, int64_t n_idx, int32_t n_files, int64_t n_items, int32_t n_ch, int32_t N, int32_t n_tables,
                   int64_t P_all, int64_t n_words) {
    VBQ_REQUIRE(n_idx >= 0 && n_files >= 0 && n_files <= 65535 && n_items >= 0 && n_ch >= 1 && n_ch <= 65535 && N >= 1 &&
                    N <= 10 && n_tables >= 1 && P_all >= 0 && n_words >= 0,
                VBQ_ERR_INVALID_ARGUMENT,
                "%s: bad sizes n_idx=%lld n_files=%d n_items=%lld n_ch=%d N=%d n_tables=%d P_all=%lld n_words=%lld", who,
                (long long)n_idx, n_files, (long long)n_items, n_ch, N, n_tables, (long long)P_all, (long long)n_words);
    VBQ_REQUIRE(n_items <= INT32_MAX && n_idx <= (INT64_MAX >> 2) / n_ch, VBQ_ERR_INVALID_ARGUMENT,
                "%s: n_items=%lld items or n_idx=%lld indices are too many", who, (long long)n_items, (long long)n_idx);
    return VBQ_OK;
}

}  // namespace
}  // namespace vbq

extern "C" int vbq_rans_il_sizes_files_u16(const uint16_t *d_idx, int64_t n_idx, const int64_t *d_files, int32_t n_files,
                                           const int32_t *d_items, int64_t n_items, int32_t n_ch, int32_t N,
                                           const uint16_t *d_freq, int32_t n_tables, const uint16_t *d_canon, uint32_t *d_sizes,
                                           int64_t P_all, uint32_t *d_status, void *stream) {
    using namespace vbq;
    if (int r = check_il_files("vbq_rans_il_sizes_files_u16", n_idx, n_files, n_items, n_ch, N, n_tables, P_all, 0)) return r;
    if (n_files == 0 || n_items == 0) return VBQ_OK;
    VBQ_REQUIRE(d_idx && d_files && d_items && d_freq && d_sizes, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_il_sizes_files_u16: null pointer argument");
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_il_encode_files<false>), dim3((unsigned)n_items), dim3(kLanes), 0,
                       reinterpret_cast<hipStream_t>(stream), d_idx, (long)n_idx, d_files, (int)n_files, d_items, (long)n_ch,
                       table_size(N), d_freq, (int)n_tables, d_canon, nullptr, nullptr, (long)P_all, 0L, nullptr, d_sizes,
                       d_status);
    VBQ_CHECK_LAUNCH("rans_il_sizes_files");
    return VBQ_OK;
}

extern "C" int vbq_rans_il_rates_files_u16(const uint16_t *d_idx, int64_t n_idx, int64_t lambda_stride, const int64_t *d_files,
                                           int32_t n_files, const int32_t *d_items, int64_t n_items, int32_t n_ch, int32_t N,
                                           const uint16_t *d_freq, int32_t n_lambda, const uint16_t *d_canon, uint32_t *d_sizes,
                                           int64_t P_all, uint32_t *d_status, void *stream) {
    using namespace vbq;
    if (int r = check_il_files("vbq_rans_il_rates_files_u16", n_idx, n_files, n_items, n_ch, N, 1, P_all, 0)) return r;
    VBQ_REQUIRE(n_lambda >= 1 && n_lambda <= 65535 && lambda_stride >= 0, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_il_rates_files_u16: bad sizes n_lambda=%d lambda_stride=%lld", n_lambda, (long long)lambda_stride);
    VBQ_REQUIRE(lambda_stride <= n_idx / n_lambda, VBQ_ERR_INVALID_ARGUMENT,     // n_lambda * lambda_stride <= n_idx, no product
                "vbq_rans_il_rates_files_u16: n_lambda=%d planes of lambda_stride=%lld indices do not fit in n_idx=%lld", n_lambda,
                (long long)lambda_stride, (long long)n_idx);
    VBQ_REQUIRE(P_all <= (INT64_MAX >> 2) / n_lambda, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_il_rates_files_u16: n_lambda=%d rows of P_all=%lld sizes are too many", n_lambda, (long long)P_all);
    if (n_files == 0 || n_items == 0) return VBQ_OK;
    VBQ_REQUIRE(d_idx && d_files && d_items && d_freq && d_sizes, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_il_rates_files_u16: null pointer argument");
    hipLaunchKernelGGL(k_il_rates_files, dim3((unsigned)n_items, (unsigned)n_lambda), dim3(kLanes), 0,
                       reinterpret_cast<hipStream_t>(stream), d_idx, (long)lambda_stride, d_files, (int)n_files, d_items,
                       (long)n_ch, table_size(N), d_freq, d_canon, (long)P_all, d_sizes, d_status);
    VBQ_CHECK_LAUNCH("rans_il_rates_files");
    return VBQ_OK;
}

extern "C" int vbq_rans_il_encode_files_u16(const uint16_t *d_idx, int64_t n_idx, const int64_t *d_files, int32_t n_files,
                                            const int32_t *d_items, int64_t n_items, int32_t n_ch, int32_t N,
                                            const uint16_t *d_freq, int32_t n_tables, const uint16_t *d_canon,
                                            const uint32_t *d_sizes, const int64_t *d_offsets, int64_t P_all,
                                            uint16_t *d_payload, int64_t n_words, uint32_t *d_status, void *stream) {
    using namespace vbq;
    if (int r = check_il_files("vbq_rans_il_encode_files_u16", n_idx, n_files, n_items, n_ch, N, n_tables, P_all, n_words)) return r;
    if (n_files == 0 || n_items == 0) return VBQ_OK;
    VBQ_REQUIRE(d_idx && d_files && d_items && d_freq && d_sizes && d_offsets, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_il_encode_files_u16: null pointer argument");
    VBQ_REQUIRE(n_words == 0 || d_payload, VBQ_ERR_INVALID_ARGUMENT, "vbq_rans_il_encode_files_u16: null pointer argument d_payload");
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_il_encode_files<true>), dim3((unsigned)n_items), dim3(kLanes), 0,
                       reinterpret_cast<hipStream_t>(stream), d_idx, (long)n_idx, d_files, (int)n_files, d_items, (long)n_ch,
                       table_size(N), d_freq, (int)n_tables, d_canon, d_sizes, d_offsets, (long)P_all, (long)n_words, d_payload,
                       nullptr, d_status);
    VBQ_CHECK_LAUNCH("rans_il_encode_files");
    return VBQ_OK;
}

extern "C" int vbq_rans_il_decode_files_u16(const uint16_t *d_payload, int64_t n_words, const uint32_t *d_sizes,
                                            const int64_t *d_offsets, int64_t P_all, const int64_t *d_files, int32_t n_files,
                                            const int32_t *d_items, int64_t n_items, int32_t n_ch, int32_t N,
                                            const uint16_t *d_freq, int32_t n_tables, uint16_t *d_idx, int64_t n_idx,
                                            uint32_t *d_status, void *stream) {
    using namespace vbq;
    if (int r = check_il_files("vbq_rans_il_decode_files_u16", n_idx, n_files, n_items, n_ch, N, n_tables, P_all, n_words)) return r;
    if (n_files == 0 || n_items == 0) return VBQ_OK;
    VBQ_REQUIRE(d_sizes && d_offsets && d_files && d_items && d_freq && d_idx, VBQ_ERR_INVALID_ARGUMENT,
                "vbq_rans_il_decode_files_u16: null pointer argument");
    VBQ_REQUIRE(n_words == 0 || d_payload, VBQ_ERR_INVALID_ARGUMENT, "vbq_rans_il_decode_files_u16: null pointer argument d_payload");
    hipLaunchKernelGGL(k_il_decode_files, dim3((unsigned)n_items), dim3(kLanes), 0, reinterpret_cast<hipStream_t>(stream),
                       d_payload, (long)n_words, d_sizes, d_offsets, (long)P_all, d_files, (int)n_files, d_items, (long)n_ch,
                       table_size(N), d_freq, (int)n_tables, d_idx, (long)n_idx, d_status);
    VBQ_CHECK_LAUNCH("rans_il_decode_files");
    return VBQ_OK;
}
