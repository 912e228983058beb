"""Word-embedding VBQ with the notebook's call surface
(word-embeddings/compress-trained-word-embeddings.ipynb cells 25-30, JSON lines 373-473).

    empirical_std(vecs)                          ipynb:373-374   (K3 moment pass)
    make_code_book(std, max_codepoint_length)    ipynb:383-390   (host: scipy ppf, as the notebook)
    compress_coordinates(means, stds, beta, ...) ipynb:429-443   (K1n)
    empirical_entropy(values)                    ipynb:452-455   (K2 histogram when indices are given)
    prediction_ranks(emb, analogies_id)          ipynb:199-209   (fused f32 MFMA GEMM + count, vbq_ranks.hip)
    test_beta / test_betas / quantize_coordinates / test_quantization   ipynb:464-473, cells 32, 36-37
    compress_to_bytes / decompress / CompressedEmbeddings    (ours) the quantized matrix as a real byte string (rANS,
                                                             vbq_amd.bitstream "VBQe") and row-wise lookups from it
    coded_nbytes / compress_to_budget                        (ours) the exact file length at every beta; the file of a byte budget
    compress_to_records / compress_to_records_budget / RecordEmbeddings    (ours) rows quantized to one exact bit budget as
                                                             fixed-size records (vbq_amd.bitstream "VBQr"): a row lookup is one
                                                             address computation and one short unpack
    most_similar / RecordEmbeddings.most_similar             (ours) the k nearest rows to a few queries (fused unpack + f32 MFMA +
                                                             top-k, vbq_topk.hip): the records are searched as they are stored
    bag / RecordEmbeddings.bag                               (ours) pooled rows -- the sum, mean or max of a list of rows per
                                                             output, torch.nn.EmbeddingBag on the compressed table (vbq_bag.hip)
    scores / similarity / rerank, also of RecordEmbeddings   (ours) the scores of the rows the caller names per query -- word-pair
                                                             similarity, reranking -- in one launch, bit for bit the search's
                                                             scores (vbq_amd/ext/vbqx_scores.hip, the second library)
    compress_to_records_sweep / records_distortion_curve / compress_to_records_quality / test_total_bits
                                                             (ours) record files at many total_bits from one pass of the budget
                                                             DP, the distortion at EVERY total_bits, and the smallest file of a
                                                             distortion target (vbq_amd/budget/vbqb_sweep.hip, the third library)
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, ops


def _dev(a, dtype=torch.float32):
    from .lazy import device_tensor
    t = device_tensor(a)                     # a result of this package that still lives on the device: no round trip
    return ops.upload(a if t is None else t, ops.current_device("vbq_amd.embeddings"), dtype)


_STAGER = None


def _stager():
    global _STAGER
    if _STAGER is None:
        from .lazy import HostStager
        _STAGER = HostStager()
    return _STAGER


def empirical_std(vecs, exact: bool = True) -> np.float32:
    """np.sqrt(np.mean(vecs.ravel()**2)) (ipynb:374), float32.  exact=True reproduces NumPy's float32 summation order
    on the GPU (vbq_numpy_sum_sq_f32), so the code book built from it is the notebook's bit for bit; exact=False is
    the f64-accumulating moment kernel K3 (order-free, agrees to 1e-6 relative, a little faster)."""
    x = _dev(vecs).reshape(-1)
    if exact:
        s = np.float32(ops.numpy_sum_sq(x).cpu().numpy()[0])
        # np.mean: the f32 sum divided by the count (a float64 division under NumPy 1.17's scalar rules, rounded back
        # to f32 -- the same value as an f32 division whenever the count is a float32 number), then the root in f32
        return np.sqrt(np.float32(float(s) / x.numel()))
    m = ops.moments(x)
    return np.float32(np.sqrt(float(m[0, 1].item()) / x.numel()))


def make_code_book(std, max_codepoint_length: int = 10):
    """ipynb:383-390: (codepoints f64 [T] level-major, lengths int64 [T])."""
    import scipy.stats
    pts, lens = [], []
    for length in range(max_codepoint_length + 1):
        xi = np.arange(0.5 ** (length + 1), 1, 0.5 ** length)
        pts.append(scipy.stats.norm.ppf(xi, scale=std))
        lens.append(np.full(xi.shape, length, dtype=np.int64))
    return np.concatenate(pts), np.concatenate(lens)


def compress_coordinates_sweep(means, stds, betas: Sequence[float], codepoints, *, want_values=True):
    """All betas in one launch.  Returns (idx u16 [n_beta, *shape] device tensor, values f32 or None)."""
    N = int(np.log2(len(codepoints) + 1)) - 1
    return ops.quantize_notebook(_dev(means), _dev(stds), _dev(codepoints, torch.float64), [float(b) for b in betas],
                                 N=N, want_values=want_values)


def compress_coordinates(means, stds, beta, bitlengths=None, codepoints=None):
    """ipynb:429-443.  `codepoints` replaces the notebook's global of the same name; `bitlengths`
    must be the level of every slot (the only table the notebook ever passes) and is validated.
    Returns the quantized array (f32, shaped like `means`).  Torch in -> a device tensor; NumPy in -> an ndarray-like lazy view
    (vbq_amd.lazy): the notebook hands the result straight to prediction_ranks / empirical_entropy (ipynb:466-470), which
    take it on the device -- the 40 MB of a 100000 x 100 vocabulary cross PCIe only if somebody reads them on the host."""
    if codepoints is None:
        raise ValueError("pass codepoints=... (the notebook reads a global; make_code_book() builds it)")
    N = int(np.log2(len(codepoints) + 1)) - 1
    if bitlengths is not None:
        want = np.concatenate([np.full(2 ** n, n) for n in range(N + 1)])
        if not np.array_equal(np.asarray(bitlengths), want):
            raise ValueError("bitlengths must equal the bit level of each level-major slot")
    _, val = compress_coordinates_sweep(means, stds, [beta], codepoints)
    if isinstance(means, torch.Tensor):
        return val[0]
    from .lazy import DeviceStack
    return DeviceStack("coordinates", val, _stager()).rows()[0]


def entropy_from_counts(counts) -> float:
    c = np.asarray(counts.cpu().numpy() if isinstance(counts, torch.Tensor) else counts, dtype=np.float64).ravel()
    c = c[c > 0]
    tot = c.sum()
    return float(tot * np.log2(tot) - c.dot(np.log2(c)))


def entropy_from_indices(idx: torch.Tensor, N: int = 10):
    """ipynb:452-455 on rank indices: one K2 histogram per beta.  idx: u16 [n_beta, ...]."""
    cnt = ops.histogram(idx.reshape(idx.shape[0], -1), 1, N=N)
    return [entropy_from_counts(cnt[i]) for i in range(cnt.shape[0])]


def empirical_entropy(values) -> float:
    """ipynb:452-455 on an arbitrary value array (generic multiset count via torch.unique)."""
    v = _dev(values).reshape(-1)
    _, counts = torch.unique(v, return_counts=True)
    return entropy_from_counts(counts)


def prediction_ranks(emb, analogies_id):
    """ipynb cell 14 (ipynb:199-209).  `analogies_id` ([Q, 4] word ids) replaces the notebook's global.
    emb: [V, K] array or device tensor.  Returns int64 ranks (NumPy in -> NumPy out)."""
    import ctypes as C
    from . import _lib
    e = _dev(emb)
    if e.dim() != 2:
        raise ValueError("emb must be [V, K]")
    an_np = analogies_id.cpu().numpy() if isinstance(analogies_id, torch.Tensor) else np.asarray(analogies_id)
    if an_np.ndim != 2 or an_np.shape[1] != 4:
        raise ValueError("analogies_id must be [Q, 4]")
    V, K = e.shape
    if an_np.size and (an_np.min() < 0 or an_np.max() >= V):
        raise IndexError("analogy word id out of range")          # NumPy fancy indexing raises too
    an = ops.host_tensor(np.asarray(an_np, dtype=np.int32)).to(e.device)
    Q = an.shape[0]
    out = torch.empty(Q, dtype=torch.int64, device=e.device)
    if Q == 0:
        return out if isinstance(emb, torch.Tensor) else out.cpu().numpy()
    h = _lib.lib()
    nbytes = h.vbq_analogy_ranks_workspace_bytes(V, K, Q)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=e.device)
    _lib.check(h.vbq_analogy_ranks_f32(ops._ptr(e), V, K, ops._ptr(an), Q, ops._ptr(out), ops._ptr(ws), C.c_size_t(nbytes),
                                       ops._stream(e)), "vbq_analogy_ranks_f32")
    return out if isinstance(emb, torch.Tensor) else out.cpu().numpy()


def analogy_metrics(ranks):
    """(mrr, acc, hits10) as computed in ipynb cells 30 and 37."""
    r = ranks.cpu().numpy() if isinstance(ranks, torch.Tensor) else np.asarray(ranks)
    return np.average(1 / (1 + r)), np.sum(r == 0) / len(r), np.sum(r < 10) / len(r)


def quantize_coordinates(means, quantization_max):
    """ipynb cell 36, the uniform-rounding baseline (torch on the device: two elementwise ops and a max)."""
    m = _dev(means)
    scale = (quantization_max + 0.5) / m.abs().max()
    q = torch.round(torch.clamp(scale * m, -quantization_max, quantization_max))
    return q if isinstance(means, torch.Tensor) else q.cpu().numpy()


def test_quantization(means, quantization_max, analogies_id):
    """ipynb cell 37: (mrr, acc, hits10, entropy, gzip, bz2, lzma bit lengths) of the rounding baseline.
    The three general-purpose compressors run on the host, as in the notebook."""
    import bz2
    import gzip
    import io
    import lzma
    quantized = np.asarray(quantize_coordinates(np.asarray(means), quantization_max))
    mrr, acc, hits10 = analogy_metrics(prediction_ranks(quantized, analogies_id))
    bits = empirical_entropy(quantized)
    raw = bytes(quantized.astype(np.int8 if quantization_max <= 127 else np.int16).data)
    buf = io.BytesIO()
    with gzip.GzipFile(fileobj=buf, mode="wb", compresslevel=9) as f:
        f.write(raw)
    gz_bits = len(buf.getbuffer()) * 8
    bz_bits = len(bz2.compress(raw, 9)) * 8
    lz_bits = len(lzma.compress(raw, format=lzma.FORMAT_ALONE, preset=9)) * 8
    return mrr, acc, hits10, bits, gz_bits, bz_bits, lz_bits


def test_betas(means, stds, betas: Sequence[float], codepoints, analogies_id):
    """The notebook's sweep `[test_beta(vecs_u, stds_u, beta) for beta in betas]` (ipynb cell 32) with the work
    batched the way the device wants it: one K1n launch solves every beta, one K2 launch counts every beta's
    indices, then one fused rank GEMM per beta.  Returns float64 [n_beta, 4] = (mrr, acc, hits10, bits) rows."""
    idx, val = compress_coordinates_sweep(means, stds, betas, codepoints)
    bits = entropy_from_indices(idx, N=int(np.log2(len(codepoints) + 1)) - 1)
    shape = tuple(np.shape(means))
    rows = []
    for i in range(len(betas)):
        ranks = prediction_ranks(val[i].reshape(shape), analogies_id)
        rows.append(analogy_metrics(ranks) + (bits[i],))
    return np.array(rows, dtype=np.float64)


def test_beta(means, stds, beta, codepoints, analogies_id=None):
    """ipynb:464-473 (the notebook passes the (array, None) tuple on; the array is used here).  With
    `analogies_id` returns (mrr, acc, hits10, bits) like the notebook; without it (compressed, bits).
    Everything stays on the device: K1n -> K2 entropy -> fused rank GEMM."""
    idx, val = compress_coordinates_sweep(means, stds, [beta], codepoints)
    compressed = val[0]
    bits = entropy_from_indices(idx, N=int(np.log2(len(codepoints) + 1)) - 1)[0]
    if analogies_id is None:
        return compressed, bits
    if callable(analogies_id):                                       # a user-supplied prediction_ranks(emb)
        ranks = np.asarray(analogies_id(compressed.cpu().numpy()))
    else:
        ranks = prediction_ranks(compressed.reshape(np.shape(means)), analogies_id)
    return analogy_metrics(ranks) + (bits,)


# ------------------------------------------------------------------------ compressed byte string (vbq_amd.bitstream, "VBQe")
_LOOKUP_SYMBOLS = 1024                       # the default segment: a whole number of rows near this many symbols
_Q75 = 0.6744897501960817                    # norm.ppf(0.75): the level-1 code points of make_code_book are -/+ std * this


def default_segment(row_length: int) -> int:
    """A whole number of rows near 1024 symbols (so that a row lookup decodes exactly one segment), or 1024 for rows
    longer than the format's largest segment."""
    from .bitstream import MAX_SEGMENT
    D = int(row_length)
    return max(1, _LOOKUP_SYMBOLS // D) * D if D <= MAX_SEGMENT else _LOOKUP_SYMBOLS


def _file_args(means, codepoints, segment):
    """(code book f64 [T], N, shape, n coordinates, segment) of a compressed file, validated."""
    from . import bitstream as bs, tables
    cp = np.asarray(_host_array(codepoints), dtype=np.float64).reshape(-1)
    N = int(np.log2(cp.size + 1)) - 1
    if not 1 <= N <= bs.MAX_N or cp.size != tables.table_size(N):
        raise ValueError(f"a code book of {cp.size} points: need 2^(N+1) - 1 of them with N in 1..{bs.MAX_N}")
    shape = tuple(int(d) for d in np.shape(means)) or (1,)
    n = int(np.prod(shape))
    if n == 0:
        raise ValueError("an empty matrix has no compressed form")
    seg = default_segment(int(np.prod(shape[1:]))) if segment is None else int(segment)
    bs.check_segment(seg)
    return cp, N, shape, n, seg


def _check_beta(beta) -> float:
    beta = float(beta)
    if not (np.isfinite(beta) and beta >= 0):
        raise ValueError(f"beta {beta} is not finite and >= 0")
    return beta


def compress_to_bytes(means, stds, beta, codepoints, *, segment=None) -> bytes:
    """The matrix `compress_coordinates(means, stds, beta, codepoints=codepoints)` as a self-describing byte string:
    K1n's rank indices, one K2 histogram, ONE device-to-host copy of the counts, a table fitted to them
    (coder.exact_frequencies), then rANS encode + pack on the device.  `decompress` / `CompressedEmbeddings` read it.
    Rows are the slices along axis 0; `segment` (symbols per rANS segment) defaults to `default_segment(row length)`."""
    from . import bitstream as bs, coder, tables
    cp, N, shape, n, seg = _file_args(means, codepoints, segment)
    beta = _check_beta(beta)
    idx, _ = compress_coordinates_sweep(means, stds, [beta], cp, want_values=False)
    idx = idx.reshape(1, n)
    counts = ops.histogram(idx, 1, N=N).cpu().numpy().reshape(-1)
    freq = coder.exact_frequencies(counts)
    sizes, payload = coder.RansCodec(freq, N=N, segment=seg, allow_zero=True).encode_packed(idx)
    ranks = np.flatnonzero(freq)
    table = np.empty(ranks.size, dtype=bs.TABLE_DTYPE)
    table["rank"] = ranks
    table["freq"] = freq[ranks]
    table["value"] = tables.level_major_to_sorted(cp).astype(np.float32)[ranks]   # what K1n writes: (float) code point
    h = bs.EmbeddingHeader(N=N, shape=shape, segment=seg, beta=beta, empirical_std=float(np.float32(cp[2] / _Q75)),
                           n_words=int(payload.size), K=int(ranks.size))
    return bs.write_embeddings(h, table, sizes, payload)


# ------------------------------------------------------------------------ rate control: exact file lengths, byte budgets
NOTEBOOK_BETAS = [float(b) for b in np.exp(np.linspace(np.log(0.01), np.log(1e5), 50))]    # ipynb cell 32
SWEEP_SCRATCH_BYTES = 1 << 30                # coded_nbytes: the u16 indices of one chunk of betas stay below this


def coded_nbytes(means, stds, betas, codepoints, *, segment=None) -> np.ndarray:
    """int64 [len(betas)]: len(compress_to_bytes(means, stds, beta, codepoints, segment=segment)) for every beta, exact,
    without building a file.  Per chunk of betas (the index scratch stays below SWEEP_SCRATCH_BYTES): one K1n sweep, one K2
    histogram and ONE copy of the counts, the tables fitted to them (coder.exact_frequencies), one vbq_rans_sizes_u16
    launch with one stream and one table per beta (segment sizes only, no words), one copy of the totals."""
    from . import bitstream as bs, coder
    cp, N, shape, n, seg = _file_args(means, codepoints, segment)
    betas = [_check_beta(b) for b in betas]
    out = np.empty(len(betas), dtype=np.int64)
    if not betas:
        return out
    m, s = _dev(means), _dev(stds)                                        # uploaded once for every chunk
    per = int(min(max(1, SWEEP_SCRATCH_BYTES // (2 * n)), 65535))        # (65535: the coder's limit on streams per launch)
    for lo in range(0, len(betas), per):
        chunk = betas[lo:lo + per]
        idx, _ = compress_coordinates_sweep(m, s, chunk, cp, want_values=False)
        idx = idx.reshape(len(chunk), n)
        counts = ops.histogram(idx, 1, N=N).cpu().numpy().reshape(len(chunk), -1)
        freq = np.stack([coder.exact_frequencies(c) for c in counts])   # host: tools/budget_bench.py times it
        sizes = coder.RansCodec(freq, N=N, segment=seg, allow_zero=True).sizes(idx)
        words = sizes.view(torch.int32).sum(dim=1, dtype=torch.int64).cpu().numpy()
        K = np.count_nonzero(freq, axis=1)
        out[lo:lo + len(chunk)] = [bs.embeddings_nbytes(shape, seg, int(k), int(w)) for k, w in zip(K, words)]
    return out


def compress_to_budget(means, stds, codepoints, max_bytes, *, betas=None, segment=None) -> bytes:
    """The file of the numerically SMALLEST beta of `betas` (default: the notebook's grid NOTEBOOK_BETAS) whose exact length is
    <= max_bytes (an integer >= 1), byte for byte compress_to_bytes at that beta; the header says which beta it is.  A larger
    beta usually, but not always, gives a smaller file: the rule takes no monotonicity for granted.  ValueError naming the
    smallest achievable length and its beta when nothing fits."""
    from . import bitstream as bs
    bs.check_budget(max_bytes)
    betas = NOTEBOOK_BETAS if betas is None else [_check_beta(b) for b in betas]
    nbytes = coded_nbytes(means, stds, betas, codepoints, segment=segment)
    beta = bs.smallest_rate_within(dict(zip(betas, nbytes.tolist())), max_bytes, "beta")
    return compress_to_bytes(means, stds, beta, codepoints, segment=segment)


def _row_ids(ids, V: int) -> np.ndarray:
    """The ids of a `rows` call as int64 [n] on the host: ValueError unless one-dimensional, IndexError for ids that are not
    integers or lie outside [0, V)."""
    ids = _host_array(ids)
    if ids.ndim != 1:
        raise ValueError(f"ids must be one-dimensional, got shape {ids.shape}")
    if ids.size and ids.dtype.kind not in "iu":
        raise IndexError(f"row ids must be integers, got {ids.dtype}")
    # (the range is checked on the dtype the ids came in, before the cast to int64: a uint64 id of 2**63 or more would turn
    # negative in it)
    ids = _int64_ids(ids, V, padding=False)
    return ids


class CompressedEmbeddings:
    """A compressed embedding matrix ("VBQe" bytes) on the device.  The header and table are validated on the host; the
    payload, sizes and segment offsets are uploaded and checked ONCE here, so a damaged size raises at load time.  Then
    `rows(ids)` decodes only the segments that hold the requested rows (one launch) and `tensor()` the whole matrix."""

    def __init__(self, data, device=None):
        from . import bitstream as bs, coder
        h, table, _, _ = bs.parse_embeddings(data)
        raw = np.frombuffer(memoryview(data).cast("B"), dtype=np.uint8)
        self.header = h
        self.nbytes = int(raw.size)
        self.device = torch.device(device) if device is not None else ops.current_device("vbq_amd.embeddings")
        T = 2 ** (h.N + 1) - 1
        # ONE upload: dense freq u16 [T] (+ 2 bytes: the values stay 4-byte aligned), values f32 [T], sizes u16 [nseg],
        # payload u16 [n_words] (the last two straight from the file)
        fb, vb = 2 * T + 2, 4 * T
        host = np.zeros(fb + vb + raw.size - h.nbytes, np.uint8)
        host[:2 * T].view(np.uint16)[table["rank"]] = table["freq"]
        host[fb:fb + vb].view(np.float32)[table["rank"]] = table["value"]
        host[fb + vb:] = raw[h.nbytes:]
        dev = torch.from_numpy(host).to(self.device)
        self._freq = dev[:2 * T].view(torch.uint16)
        self._values = dev[fb:fb + vb].view(torch.float32)
        self._sizes = dev[fb + vb:fb + vb + 2 * h.nseg].view(torch.uint16)
        self._payload = dev[fb + vb + 2 * h.nseg:].view(torch.uint16)
        self._offsets = torch.empty(h.nseg, dtype=torch.int64, device=self.device)
        status = torch.zeros(1, dtype=torch.uint32, device=self.device)
        _lib.check(_lib.lib().vbq_rans_segment_offsets_u16(ops._ptr(self._sizes), h.nseg, h.segment, h.n_words,
                                                            ops._ptr(self._offsets), ops._ptr(status), ops._stream(dev)),
                   "vbq_rans_segment_offsets_u16")
        coder._raise_status(int(status.cpu().item()))

    @property
    def shape(self):
        return self.header.shape

    @property
    def beta(self) -> float:
        return self.header.beta

    @property
    def bits_per_coordinate(self) -> float:
        """The whole byte string (header and table included) in bits per coordinate."""
        return 8.0 * self.nbytes / self.header.n

    def _decode(self, segments: Optional[torch.Tensor], out: torch.Tensor):
        from . import coder
        h = self.header
        status = torch.zeros(1, dtype=torch.uint32, device=self.device)
        _lib.check(_lib.lib().vbq_rans_decode_values_f32(
            ops._ptr(self._payload), h.n_words, ops._ptr(self._sizes), ops._ptr(self._offsets), h.n, h.segment, h.N,
            ops._ptr(self._freq), ops._ptr(self._values), ops._ptr(segments), 0 if segments is None else segments.numel(),
            ops._ptr(out), ops._ptr(status), ops._stream(out)), "vbq_rans_decode_values_f32")
        coder._raise_status(int(status.cpu().item()))

    def tensor(self) -> torch.Tensor:
        """The whole matrix, f32 on the device, shaped like the compressed array."""
        out = torch.empty(self.header.n, dtype=torch.float32, device=self.device)
        self._decode(None, out)
        return out.view(self.header.shape)

    def rows(self, ids) -> torch.Tensor:
        """Rows `ids` (any order, repeats allowed) -> f32 device tensor [len(ids), *shape[1:]].  IndexError outside [0, V)."""
        h = self.header
        V, D, seg = h.shape[0], h.row_length, h.segment
        ids = _row_ids(ids, V)
        out_shape = (ids.size,) + tuple(h.shape[1:])
        if ids.size == 0:
            return torch.empty(out_shape, dtype=torch.float32, device=self.device)
        first = ids * D // seg
        if seg % D == 0:                                            # whole rows per segment (the default): gather rows
            uniq, slot = np.unique(first, return_inverse=True)
            per = seg // D
            dev = torch.from_numpy(np.concatenate([uniq, slot.reshape(-1) * per + ids * D % seg // D])).to(self.device)
            buf = torch.empty(uniq.size * seg, dtype=torch.float32, device=self.device)
            self._decode(dev[:uniq.size], buf)
            return buf.view(uniq.size * per, D).index_select(0, dev[uniq.size:]).view(out_shape)
        last = (ids * D + D - 1) // seg                             # rows straddle segments: gather coordinates
        cand = first[:, None] + np.arange(int((last - first).max()) + 1)[None, :]
        uniq = np.unique(cand[cand <= last[:, None]])
        dev = torch.from_numpy(np.concatenate([uniq, ids])).to(self.device)
        segs, rid = dev[:uniq.size], dev[uniq.size:]
        buf = torch.empty(uniq.size * seg, dtype=torch.float32, device=self.device)
        self._decode(segs, buf)
        slot_of = torch.zeros(h.nseg, dtype=torch.int64, device=self.device)
        slot_of[segs] = torch.arange(uniq.size, dtype=torch.int64, device=self.device)
        e = rid[:, None] * D + torch.arange(D, dtype=torch.int64, device=self.device)[None, :]
        return buf[(slot_of[e // seg] * seg + e % seg).reshape(-1)].view(out_shape)


def decompress(data, return_np: bool = True):
    """`compress_to_bytes` or `compress_to_records` inverted, by the magic of `data`: the quantized matrix (f32, bit for bit what
    compress_coordinates returns / the code points quantize_rows_to_budget chose), as a NumPy array or (return_np=False) a
    device tensor.  A damaged byte string raises ValueError (header, table, sizes) or VBQError (payload, records)."""
    from .bitstream import RECORDS_MAGIC
    records = bytes(memoryview(data).cast("B")[:4]) == RECORDS_MAGIC
    t = (RecordEmbeddings if records else CompressedEmbeddings)(data).tensor()
    return t.cpu().numpy() if return_np else t


# ------------------------------------------------------------------------ nearest rows (vbq_topk.hip)
def _search_args(queries, K: int, k, metric, exclude, device):
    """(queries f32 [Q, K] on the device -- for the cosine divided by 1e-8 + |q| in f32 --, exclude int64 [Q, E] or None) of a
    most_similar call; ValueError for k outside 1..64, an unknown metric, a query of the wrong width or with a non-finite
    coordinate, and an exclude list that is not [Q, E <= 8]."""
    import operator
    k = operator.index(k)
    if not 1 <= k <= 64:
        raise ValueError(f"k = {k} outside 1..64")
    q = _query_args(queries, K, metric, device)
    if exclude is not None:
        exclude = ops.upload(exclude, device, torch.int64)
        if exclude.dim() == 1 and q.shape[0] == 1:
            exclude = exclude[None, :]
        if exclude.dim() != 2 or exclude.shape[0] != q.shape[0] or exclude.shape[1] > 8:
            raise ValueError(f"exclude must be [{q.shape[0]}, E] with E <= 8, got shape {tuple(exclude.shape)}")
    return q, k, exclude


def _query_args(queries, K: int, metric, device):
    """The queries of a most_similar or scores call as the kernels take them: f32 [Q, K] on the device, for the cosine divided
    by 1e-8 + |q| in f32; ValueError for an unknown metric, a query of the wrong width or with a non-finite coordinate."""
    if metric not in ("dot", "cosine"):
        raise ValueError(f"metric {metric!r} is neither 'dot' nor 'cosine'")
    q = ops.upload(queries, device, torch.float32)
    if q.dim() == 1:
        q = q[None, :]
    if q.dim() != 2 or q.shape[1] != K:
        raise ValueError(f"queries must be [Q, {K}] or [{K}], got shape {tuple(q.shape)}")
    if not bool(torch.isfinite(q).all()):
        raise ValueError("queries hold a NaN or an infinity")
    if metric == "cosine":
        q = q / (1e-8 + torch.sqrt(torch.sum(q * q, dim=1, keepdim=True)))
    return q.contiguous()


def most_similar(emb, queries, k: int = 10, metric: str = "cosine", exclude=None):
    """The k rows of the dense matrix `emb` ([V, K], tensor or ndarray) nearest to each query ([Q, K] or [K]) -> (ids int64
    [Q, k], scores f32 [Q, k]) device tensors, ordered by score descending, then id ascending, padded with -1 / -inf when fewer
    than k rows are eligible.  metric "cosine": q . v / ((1e-8 + |q|)(1e-8 + |v|)); "dot": q . v; `exclude` ([Q, E <= 8] row
    ids, negative = none) names rows never returned for that query.  The semantics are those of include/vbq.h ("Nearest
    rows"); a "VBQe" file is served as most_similar(CompressedEmbeddings(data).tensor(), ...), a "VBQr" file without decoding it
    by RecordEmbeddings.most_similar."""
    e = _dev(emb)
    if e.dim() != 2:
        raise ValueError("emb must be [V, K]")
    q, k, exclude = _search_args(queries, e.shape[1], k, metric, exclude, e.device)
    return ops.topk(e, q, k, metric, exclude)


def _host_array(a) -> np.ndarray:
    """A tensor (any device, also one that requires grad), NumPy array or sequence as a NumPy array on the host."""
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)


# ------------------------------------------------------------------------ pooled rows (vbq_bag.hip)
_BAG_MODES = ("sum", "mean", "max")


def _bag_args(ids, offsets, weights, mode, V: int):
    """The host checks of a `bag` call -> (ids int64 [n], offsets int64 [B + 1], weights f32 [n] or None), NumPy arrays for
    the C call of include/vbq.h ("Pooled rows").  ids: 1-D with `offsets` [B] (bag starts, torch.nn.EmbeddingBag's convention:
    the last bag runs to the end), or 2-D [B, L] without (row b is bag b); negative ids are padding in both forms.  ValueError
    for an unknown mode, weights with a mode other than "sum", weights that are not finite or not shaped like ids, and offsets
    that do not start at 0, decrease or exceed len(ids); IndexError for ids that are not integers or reach V."""
    host = _host_array
    if mode not in _BAG_MODES:
        raise ValueError(f"mode {mode!r} is none of 'sum', 'mean', 'max'")
    if weights is not None and mode != "sum":
        raise ValueError(f"weights go with mode 'sum' only, not {mode!r}")
    ids = host(ids)
    if ids.ndim not in (1, 2):
        raise ValueError(f"ids must be [n] (with offsets) or [B, L], got shape {ids.shape}")
    if ids.size and ids.dtype.kind not in "iu":
        raise IndexError(f"row ids must be integers, got {ids.dtype}")
    if weights is not None:
        weights = host(weights)
        if weights.shape != ids.shape:
            raise ValueError(f"weights {weights.shape} and ids {ids.shape} differ in shape")
        weights = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        if not np.isfinite(weights).all():
            raise ValueError("weights hold a NaN or an infinity")
    if ids.ndim == 2:
        if offsets is not None:
            raise ValueError("two-dimensional ids are one bag per row: offsets must be None")
        offsets = np.arange(ids.shape[0] + 1, dtype=np.int64) * ids.shape[1]
    else:
        if offsets is None:
            raise ValueError("one-dimensional ids need offsets (the bag starts)")
        offsets = host(offsets)
        if offsets.ndim != 1 or (offsets.size and offsets.dtype.kind not in "iu"):
            raise ValueError(f"offsets must be one-dimensional integers, got shape {offsets.shape} of {offsets.dtype}")
        offsets = np.concatenate([offsets.astype(np.int64), np.array([ids.size], np.int64)])
        if offsets[0] != 0 or (np.diff(offsets) < 0).any():
            raise ValueError(f"offsets must start at 0, never decrease and stay within len(ids) = {ids.size}")
    # (range before cast, as in _row_ids: an id that wrapped to a negative one would be pooled as padding)
    ids = _int64_ids(ids, V, padding=True).reshape(-1)
    return ids, offsets, weights


def _bag_call(call, device, args, mode, tail):
    """Uploads of `args` (what _bag_args returned), the one launch `call(ids, offsets, weights=, mode=, status=)` and the look
    at the status word -> f32 [B, *tail]."""
    ids, offsets, weights = (None if a is None else ops.host_tensor(a).to(device) for a in args)
    status = torch.zeros(1, dtype=torch.uint32, device=device)
    out = call(ids, offsets, weights=weights, mode=mode, status=status)
    assert int(status.cpu().item()) == 0, "ids and offsets checked on the host, records validated at load: no status bit is due"
    return out.view((out.shape[0],) + tuple(tail))


def bag(emb, ids, offsets=None, *, mode: str = "sum", weights=None):
    """Pooled rows of the dense matrix `emb` ([V, K], tensor or ndarray): per bag the sum, mean or max of the rows its ids list
    -> f32 device tensor [B, K], in one launch and without a [len(ids), K] matrix of the listed rows (vbq_bag_f32; the semantics
    are those of include/vbq.h, "Pooled rows": additions in the order of the list, each rounded to f32).  `ids` is 1-D with
    `offsets` [B] (bag starts as in torch.nn.EmbeddingBag: the last bag runs to the end) or 2-D [B, L] without; negative ids are
    padding; `weights` (shaped like ids, finite) go with mode "sum" only.  IndexError for an id that is not an integer or
    reaches V; ValueError for offsets that do not start at 0, decrease or exceed len(ids), for weights of another shape or with
    another mode, and for an unknown mode.  A "VBQe" file is served as bag(CompressedEmbeddings(data).tensor(), ...), a "VBQr"
    file without decoding it by RecordEmbeddings.bag, bit for bit the same.  One wave pools one bag: this is for many short
    bags; a few very long bags run serially ("Pooled rows")."""
    shape = tuple(int(d) for d in np.shape(emb))
    if len(shape) != 2:
        raise ValueError("emb must be [V, K]")
    args = _bag_args(ids, offsets, weights, mode, shape[0])                         # the host checks need no device
    e = _dev(emb)
    return _bag_call(lambda *a, **kw: ops.bag(e, *a, **kw), e.device, args, mode, shape[1:])


# ------------------------------------------------------------------------ listed rows (vbq_amd/ext/vbqx_scores.hip)
def _listed_ids(queries, ids, V: int):
    """The ids of a `scores` call -> (int64 [Q, M] tensor, whether their range was checked here), Q the number of `queries`
    ([Q, K] or [K]).  ids: [Q, M], or [M] with one query; negative ids are padding.  Host-side ids (lists, NumPy, CPU tensors)
    that reach V raise IndexError here, before any device work; a device tensor is not read back -- the kernel's status bit
    reports its range.  IndexError for ids that are not integers, ValueError for another shape.  Needs no device."""
    on_device = isinstance(ids, torch.Tensor) and ids.is_cuda
    if on_device:
        if ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool:
            raise IndexError(f"row ids must be integers, got {ids.dtype}")
        t = ids.to(torch.int64)
    else:
        a = _host_array(ids)
        if a.size and a.dtype.kind not in "iu":
            raise IndexError(f"row ids must be integers, got {a.dtype}")
        t = ops.host_tensor(_int64_ids(a, V, padding=True))
    qs = tuple(np.shape(queries))
    Q = 1 if len(qs) == 1 else (int(qs[0]) if qs else 0)
    if t.dim() == 1 and Q == 1:
        t = t[None, :]
    if t.dim() != 2 or t.shape[0] != Q:
        raise ValueError(f"ids must be [{Q}, M] (or [M] with one query), got shape {tuple(t.shape)}")
    return t, not on_device


def _scores_call(call, queries, listed, K: int, V: int, metric, device):
    """The query checks of a `scores` call, the one launch `call(queries, ids, metric, status=)` on what _listed_ids returned
    and -- for ids that were not checked on the host -- the look at the status word, after the launch -> (scores f32 [Q, M],
    ids int64 [Q, M] on the device)."""
    q = _query_args(queries, K, metric, device)
    ids = listed[0].to(device).contiguous()
    status = None if listed[1] else torch.zeros(1, dtype=torch.uint32, device=device)
    out = call(q, ids, metric, status=status)
    # ids checked on the host and records validated at load: no status bit is due, none is asked for, nothing is waited for
    if status is not None and int(status.cpu().item()) & ops.SCORES_BAD_ROW:
        raise IndexError(f"a row id outside [0, {V}) (negative ids are padding)")
    return out, ids


def _pair_ids(a, b, V: int):
    """The ids of a `similarity` call as two int64 host arrays [P] and their common shape; IndexError unless every id is an
    integer in [0, V), ValueError for two shapes.  Needs no device."""
    a, b = (_host_array(x) for x in (a, b))
    if a.shape != b.shape:
        raise ValueError(f"a {a.shape} and b {b.shape} differ in shape")
    return _row_ids(a.reshape(-1), V), _row_ids(b.reshape(-1), V), a.shape


def _rerank_k(k, M: int) -> int:
    import operator
    k = M if k is None else operator.index(k)
    if not (1 <= k <= M or k == M == 0):
        raise ValueError(f"k = {k} outside 1..M = {M}")
    return k


def _rerank(s: torch.Tensor, ids: torch.Tensor, k: int):
    """(ids, scores) [Q, k] of the scores s [Q, M] of the rows ids [Q, M] in most_similar's total order: score descending, then
    id ascending, -0.0 == 0.0; padding (negative ids, score -inf) at the tail as -1 / -inf.  Two stable torch sorts."""
    key = torch.where(ids < 0, torch.iinfo(torch.int64).max, ids)
    by_id = torch.argsort(key, dim=1, stable=True)
    by_score = torch.argsort(s.gather(1, by_id) + 0.0, dim=1, descending=True, stable=True)       # + 0.0: -0.0 sorts as 0.0
    order = by_id.gather(1, by_score)[:, :k]
    out_ids = ids.gather(1, order)
    return torch.where(out_ids < 0, -1, out_ids), s.gather(1, order)


def _dense_shape(emb):
    shape = tuple(int(d) for d in np.shape(emb))
    if len(shape) != 2:
        raise ValueError("emb must be [V, K]")
    return shape


def _dense_scores(emb, shape, queries, listed, metric):
    e = _dev(emb)
    return _scores_call(lambda *a, **kw: ops.scores(e, *a, **kw), queries, listed, shape[1], shape[0], metric, e.device)


def scores(emb, queries, ids, metric: str = "cosine"):
    """The score of each query against the rows it lists, on the dense matrix `emb` ([V, K], tensor or ndarray) -> f32 device
    tensor [Q, M], in one launch and without a [Q * M, K] matrix of the listed rows (vbqx_scores_f32; the semantics are those
    of include/vbq_ext.h, "Listed rows").  queries: [Q, K] or [K]; ids: integers [Q, M], or [M] with one query.  The scores are
    those `most_similar` reports for the same (query, row), bit for bit: metric "cosine" is q . v / ((1e-8 + |q|)(1e-8 + |v|)),
    "dot" is q . v.  A negative id is padding and scores -inf, so the -1 tail of a most_similar result can be fed back in.
    IndexError for ids that are not integers or reach V: host-side ids (lists, NumPy) before any device work, a device tensor
    -- which is not read back first -- after the launch.  ValueError for a query of the wrong width or with a non-finite
    coordinate, an unknown metric, ids of another shape.  A "VBQe" file is served as scores(CompressedEmbeddings(data).tensor(),
    ...), a "VBQr" file without decoding it by RecordEmbeddings.scores, bit for bit the same."""
    shape = _dense_shape(emb)
    listed = _listed_ids(queries, ids, shape[0])                                    # the host checks need no device
    return _dense_scores(emb, shape, queries, listed, metric)[0]


def similarity(emb, a, b, metric: str = "cosine"):
    """The score of row a[i] against row b[i] of the dense matrix `emb` -> f32 device tensor shaped like `a`: word-pair
    similarity.  `a` and `b` are integer arrays of one shape, every id in [0, V) (IndexError otherwise).  Row a is the QUERY
    -- for the cosine divided by 1e-8 + |row a| as most_similar does with a query --, row b the candidate, scored as `scores`
    with one id per query.  The two roles round differently: the result is NOT bitwise symmetric in (a, b)."""
    shape = _dense_shape(emb)
    a, b, out_shape = _pair_ids(a, b, shape[0])
    e = _dev(emb)
    queries = e.index_select(0, ops.host_tensor(a).to(e.device))
    return _dense_scores(e, shape, queries, (ops.host_tensor(b)[:, None], True), metric)[0].view(out_shape)


def rerank(emb, queries, ids, k=None, metric: str = "cosine"):
    """`scores(emb, queries, ids, metric)` put into most_similar's order -> (ids int64 [Q, k or M], scores f32 [Q, k or M])
    device tensors: score descending, then id ascending, -0.0 == 0.0; padding (negative ids) goes to the tail as -1 / -inf;
    an id listed twice stays twice.  ValueError for k outside 1..M.  A torch sort over the scores."""
    shape = _dense_shape(emb)
    listed = _listed_ids(queries, ids, shape[0])
    k = _rerank_k(k, listed[0].shape[1])
    return _rerank(*_dense_scores(emb, shape, queries, listed, metric), k)


# ------------------------------------------------------------------------ fixed-size records (vbq_amd.bitstream, "VBQr")
def _records_args(means, codepoints, N):
    """(code book f32 level-major [T] or [K, T], matrix shape, C) of a record file."""
    from .tables import table_size
    shape = tuple(int(d) for d in np.shape(means)) or (1,)
    if int(np.prod(shape)) == 0:
        raise ValueError("an empty matrix has no compressed form")
    cp = np.asarray(_host_array(codepoints), dtype=np.float32)
    K = int(np.prod(shape[1:]))
    C = K if cp.shape == (K, table_size(N)) else 1
    return cp, shape, C


def compress_to_records(means, stds, total_bits, codepoints, N: int = 10) -> bytes:
    """The matrix quantized row by row to EXACTLY total_bits raw bits (vbq_amd.quantize_rows_to_budget; rows are the slices
    along axis 0) as a self-describing byte string of fixed-size records: the budget DP's rank indices, one pack launch
    (vbq_records_pack_u16), ONE device-to-host copy.  `codepoints`: level-major, one code book [T] or one per column [K, T],
    T = 2^(N+1) - 1.  `decompress` / `RecordEmbeddings` read it; bitstream.records_nbytes gives its length in advance.  A row
    costs K * W + total_bits bits whatever it holds (W = 4 at N = 10): what the format buys is a row lookup by address, not
    size -- `compress_to_bytes` stays the small file."""
    import operator
    from . import bitstream as bs, tables
    from .rows_budget import quantize_rows_to_budget
    cp, shape, C = _records_args(means, codepoints, N)
    h = bs.RecordsHeader(N=int(N), shape=shape, C=C, total_bits=operator.index(total_bits))
    h.check()
    R, K, RW = h.n_rows, h.row_length, h.record_words
    idx, _, _ = quantize_rows_to_budget(_dev(means).reshape(R, K), _dev(stds).reshape(R, K), h.total_bits, table=cp, N=h.N)
    buf = torch.zeros(R * RW + 1, dtype=torch.int32, device=idx.device).view(torch.uint32)       # the records, then the status
    ops.records_pack(idx, h.total_bits, h.N, status=buf[-1:], out=buf[:-1].view(R, RW))
    host = buf.cpu().numpy()
    if host[-1]:
        raise _lib.VBQError("compress_to_records: the rank indices of a row do not spell the bit lengths it was given (a code "
                            "book with equal neighbouring code points has no unique rank index)")
    return bs.write_records(h, tables.level_major_to_sorted(cp.reshape(C, h.T)), host[:-1])


def compress_to_records_budget(means, stds, codepoints, max_bytes, N: int = 10) -> bytes:
    """`compress_to_records` at the largest total_bits whose file is <= max_bytes long (bitstream.records_total_bits_within:
    a closed form, nothing is searched).  ValueError naming the smallest possible file when even total_bits = 0 does not fit."""
    from . import bitstream as bs
    _, shape, C = _records_args(means, codepoints, N)
    return compress_to_records(means, stds, bs.records_total_bits_within(shape, N, C, max_bytes), codepoints, N)


def _records_headers(shape, C, budgets, N):
    import operator
    from . import bitstream as bs
    headers = [bs.RecordsHeader(N=int(N), shape=shape, C=C, total_bits=operator.index(b)) for b in budgets]
    for h in headers:
        h.check()
    return headers


def compress_to_records_sweep(means, stds, budgets, codepoints, N: int = 10):
    """[compress_to_records(means, stds, b, codepoints, N) for b in budgets], byte for byte, with the rows solved at every
    budget in ONE sweep (vbq_amd.quantize_rows_to_budgets: the candidates scored once, one DP pass at the largest budget), then
    one pack launch and one device-to-host copy per budget.  `budgets`: ints in any order, repeats allowed."""
    from . import bitstream as bs, tables
    from .rows_budget import quantize_rows_to_budgets
    cp, shape, C = _records_args(means, codepoints, N)
    headers = _records_headers(shape, C, budgets, N)
    if not headers:
        return []
    R, K = headers[0].n_rows, headers[0].row_length
    idx, _, _ = quantize_rows_to_budgets(_dev(means).reshape(R, K), _dev(stds).reshape(R, K), [h.total_bits for h in headers],
                                         table=cp, N=int(N))
    table = tables.level_major_to_sorted(cp.reshape(C, headers[0].T))
    files = []
    for s, h in enumerate(headers):
        RW = h.record_words
        buf = torch.zeros(R * RW + 1, dtype=torch.int32, device=idx.device).view(torch.uint32)   # the records, then the status
        ops.records_pack(idx[s], h.total_bits, h.N, status=buf[-1:], out=buf[:-1].view(R, RW))
        host = buf.cpu().numpy()
        if host[-1]:
            raise _lib.VBQError("compress_to_records: the rank indices of a row do not spell the bit lengths it was given (a code "
                                "book with equal neighbouring code points has no unique rank index)")
        files.append(bs.write_records(h, table, host[:-1]))
    return files


def records_distortion_curve(means, stds, codepoints, N: int = 10) -> np.ndarray:
    """D(b) for b = 0..K N, float64 NumPy [K N + 1]: the mean of ((z_hat - mu) / sigma)^2 over the matrix that the record file
    compress_to_records(means, stds, b, codepoints, N) has -- with bitstream.records_nbytes, the whole rate-distortion curve of
    the format.  D(b) = -2 * sum_r objective(r, b) / (R K), the objectives from the curve-only pass of the budget DP
    (vbq_amd.rows_budget.budget_curve) over chunks of at most rows_budget.CURVE_SCRATCH_BYTES // (8 (K N + 1)) rows, whose f64
    column sums are added in ascending chunk order: the [R, K N + 1] matrix is never held.  D need not be monotone in b --
    every row spends exactly b bits."""
    from . import rows_budget
    cp, shape, C = _records_args(means, codepoints, N)
    h = _records_headers(shape, C, [0], N)[0]
    R, K = h.n_rows, h.row_length
    mu, sg = _dev(means).reshape(R, K), _dev(stds).reshape(R, K)
    step = max(1, rows_budget.CURVE_SCRATCH_BYTES // (8 * (K * h.N + 1)))
    total = None
    for r0 in range(0, R, step):
        part = rows_budget.budget_curve(mu[r0:r0 + step], sg[r0:r0 + step], table=cp, N=h.N).sum(dim=0)
        total = part if total is None else total + part
    return (-2.0 * total / (R * K)).cpu().numpy()


def _smallest_bits_within(curve, max_distortion) -> int:
    """The smallest b with curve[b] <= max_distortion.  The curve need not be monotone, so every b is looked at (no bisection).
    ValueError naming the curve's minimum and where it is reached when no b qualifies."""
    curve = np.asarray(curve, dtype=np.float64)
    target = float(max_distortion)
    if target != target:
        raise ValueError("max_distortion is NaN")
    ok = np.flatnonzero(curve <= target)
    if ok.size == 0:
        best = int(np.nanargmin(curve))
        raise ValueError(f"no total_bits reaches a distortion of {target!r}: the smallest is {float(curve[best])!r}, "
                         f"at total_bits = {best}")
    return int(ok[0])


def compress_to_records_quality(means, stds, codepoints, max_distortion, N: int = 10) -> bytes:
    """`compress_to_records` at the SMALLEST total_bits whose record file has a distortion D(b) <= max_distortion
    (records_distortion_curve: the mean of ((z_hat - mu) / sigma)^2) -- the dual of compress_to_records_budget.  ValueError
    naming min_b D(b) and the b it is reached at when no total_bits qualifies."""
    b = _smallest_bits_within(records_distortion_curve(means, stds, codepoints, N), max_distortion)
    return compress_to_records(means, stds, b, codepoints, N)


def test_total_bits(means, stds, budgets, codepoints, analogies_id):
    """test_betas for record files: float64 [len(budgets), 4] rows (mrr, acc, hits10, bits) of the matrix quantized row by row
    to each total_bits of `budgets` -- one budget sweep (vbq_amd.quantize_rows_to_budgets), then one fused rank GEMM per budget
    on the chosen code points.  `bits` is the file's cost per coordinate, 8 * bitstream.records_nbytes / n."""
    from . import bitstream as bs
    from .rows_budget import _rows_sweep
    N = int(np.log2(np.shape(codepoints)[-1] + 1)) - 1
    cp, shape, C = _records_args(means, codepoints, N)
    headers = _records_headers(shape, C, budgets, N)
    if not headers:
        return np.zeros((0, 4), dtype=np.float64)
    R, K = headers[0].n_rows, headers[0].row_length
    chosen = _rows_sweep("embeddings.test_total_bits", _dev(means).reshape(R, K), _dev(stds).reshape(R, K),
                         [h.total_bits for h in headers], cp, N)[3]
    rows = []
    for s, h in enumerate(headers):
        ranks = prediction_ranks(chosen[s], analogies_id)
        rows.append(analogy_metrics(ranks) + (8.0 * bs.records_nbytes(shape, N, h.total_bits, C) / h.n,))
    return np.array(rows, dtype=np.float64)


class RecordEmbeddings:
    """A matrix of fixed-size records ("VBQr" bytes) on the device.  The header and the code points are validated on the host;
    code points and records are uploaded ONCE and every record is checked in one validating pass here, so a damaged record
    raises VBQError at load time.  Then `rows(ids)` is one launch that reads only the records asked for -- a row's address
    is its number times the record length -- and `tensor()` decodes the whole matrix."""

    def __init__(self, data, device=None):
        from . import bitstream as bs
        h, _, _ = bs.parse_records(data)
        raw = np.frombuffer(memoryview(data).cast("B"), dtype=np.uint8)
        self.header = h
        self.nbytes = int(raw.size)
        self.device = torch.device(device) if device is not None else ops.current_device("vbq_amd.embeddings")
        dev = torch.from_numpy(raw[h.nbytes:].copy()).to(self.device)       # ONE upload: code points, padding, records
        self._table = dev[:4 * h.C * h.T].view(torch.float32).view(h.C, h.T)
        self._words = dev[h.table_nbytes:].view(torch.uint32).view(h.n_rows, h.record_words)
        status = torch.zeros(1, dtype=torch.uint32, device=self.device)
        ops.records_unpack(self._words, h.row_length, h.N, h.total_bits, None, want_values=False, status=status)
        bits = int(status.cpu().item())
        if bits:
            what = [name for b, name in ops.RECORDS_UNPACK_STATUS if bits & b]
            raise _lib.VBQError("damaged record file: a record holds " + ", ".join(what))

    @property
    def shape(self):
        return self.header.shape

    @property
    def total_bits(self) -> int:
        return self.header.total_bits

    @property
    def bits_per_coordinate(self) -> float:
        """The whole byte string (header and code points included) in bits per coordinate."""
        return 8.0 * self.nbytes / self.header.n

    def _decode(self, row_ids: Optional[torch.Tensor]) -> torch.Tensor:
        h = self.header
        return ops.records_unpack(self._words, h.row_length, h.N, h.total_bits, self._table, row_ids)[0]

    def tensor(self) -> torch.Tensor:
        """The whole matrix, f32 on the device, shaped like the compressed array."""
        return self._decode(None).view(self.header.shape)

    def rows(self, ids) -> torch.Tensor:
        """Rows `ids` (any order, repeats allowed) -> f32 device tensor [len(ids), *shape[1:]].  IndexError outside [0, V)."""
        h = self.header
        ids = _row_ids(ids, h.n_rows)
        out_shape = (ids.size,) + tuple(h.shape[1:])
        if ids.size == 0:
            return torch.empty(out_shape, dtype=torch.float32, device=self.device)
        return self._decode(ops.host_tensor(ids).to(self.device)).view(out_shape)

    def most_similar(self, queries=None, *, ids=None, k: int = 10, metric: str = "cosine", exclude=None):
        """The k rows nearest to each query -> (ids int64 [Q, k], scores f32 [Q, k]) device tensors, as the module's
        `most_similar` on tensor() bit for bit, but straight from the records: no V x K float32 matrix is written or read,
        only a workspace of 12 bytes per (workgroup, query, result).  Exactly one of `queries` ([Q, K] or [K], tensor or
        ndarray) and `ids` (row ids: the queries are rows(ids), and each query's own row is excluded in addition to `exclude`,
        which then holds at most 7 columns) is given.  IndexError for ids outside [0, V).  The records are decoded once per
        block of 32 queries: this is for a few queries; many (the analogy set) decode once -- tensor() -- and use
        prediction_ranks or a matrix product.  Records too long for the kernel's tiles (K above 512 can be) raise VBQError
        naming the limit; tensor() still serves them."""
        h = self.header
        if (queries is None) == (ids is None):
            raise ValueError("give exactly one of queries and ids")
        K = h.row_length
        if ids is not None:
            own = _row_ids(ids, h.n_rows)
            queries = self.rows(own).reshape(own.size, K)
        q, k, exclude = _search_args(queries, K, k, metric, exclude, self.device)
        if ids is not None:
            own = ops.host_tensor(own).to(self.device)[:, None]
            exclude = own if exclude is None else torch.cat([own, exclude], dim=1)
            if exclude.shape[1] > 8:
                raise ValueError("with ids, exclude holds at most 7 columns (the query's own row is the eighth)")
        status = torch.zeros(1, dtype=torch.uint32, device=self.device)
        out = ops.records_topk(self._words, K, h.N, h.total_bits, self._table, q, k, metric, exclude, status=status)
        assert int(status.cpu().item()) == 0, "a record validated at load failed the unpack's checks"
        return out

    def bag(self, ids, offsets=None, *, mode: str = "sum", weights=None):
        """Pooled rows -> f32 device tensor [B, *shape[1:]]: per bag the sum, mean or max of the rows its ids list, as the
        module's `bag` on tensor() bit for bit, but straight from the records in one launch: no [len(ids), K] float32 matrix is
        written or read.  `ids` is 1-D with `offsets` [B] (bag starts as in torch.nn.EmbeddingBag: the last bag runs to the
        end) or 2-D [B, L] without; negative ids are padding; `weights` (shaped like ids, finite) go with mode "sum" only.
        IndexError for an id that is not an integer or reaches V; ValueError for bad offsets, weights or mode (the module's
        `bag` lists them).  One wave pools one bag, entry by entry in the order given: this is for many short bags; a few very
        long bags run serially.  Rows too long for the kernel's LDS (K above 16804 can be) raise VBQError naming the limit."""
        h = self.header
        args = _bag_args(ids, offsets, weights, mode, h.n_rows)
        return _bag_call(lambda *a, **kw: ops.records_bag(self._words, h.row_length, h.N, h.total_bits, self._table, *a, **kw),
                         self.device, args, mode, h.shape[1:])

    def _scores(self, queries, listed, metric):
        h = self.header
        return _scores_call(lambda *a, **kw: ops.records_scores(self._words, h.row_length, h.N, h.total_bits, self._table, *a, **kw),
                            queries, listed, h.row_length, h.n_rows, metric, self.device)

    def scores(self, queries, ids, metric: str = "cosine"):
        """The score of each query against the rows it lists -> f32 device tensor [Q, M], as the module's `scores` on tensor()
        bit for bit, but straight from the records in one launch: no [Q * M, K] float32 matrix is written or read, nothing
        but the result is allocated.  queries: [Q, K] or [K]; ids: integers [Q, M], or [M] with one query.  The scores are those
        `most_similar` reports for the same (query, row), bit for bit; a negative id is padding and scores -inf, so the -1 tail
        of a most_similar result can be fed back in.  IndexError for ids that are not integers or reach V: host-side ids
        (lists, NumPy) before any device work, a device tensor -- which is not read back first -- after the launch.
        ValueError for the queries most_similar refuses and for ids of another shape.  Records too long for the kernel's LDS
        (K above 3500 can be) raise VBQError naming the limit."""
        return self._scores(queries, _listed_ids(queries, ids, self.header.n_rows), metric)[0]

    def similarity(self, a, b, metric: str = "cosine"):
        """The score of row a[i] against row b[i] -> f32 device tensor shaped like `a`: word-pair similarity.  `a` and `b` are
        integer arrays of one shape, every id in [0, V) (IndexError otherwise).  Row a is the QUERY -- rows(a), for the cosine
        divided by 1e-8 + |row a| as most_similar(ids=a) does --, row b the candidate, scored as `scores` with one id per
        query.  The two roles round differently: the result is NOT bitwise symmetric in (a, b)."""
        h = self.header
        a, b, out_shape = _pair_ids(a, b, h.n_rows)
        queries = self.rows(a).reshape(a.size, h.row_length)
        return self._scores(queries, (ops.host_tensor(b)[:, None], True), metric)[0].view(out_shape)

    def rerank(self, queries, ids, k=None, metric: str = "cosine"):
        """`scores(queries, ids, metric)` put into most_similar's order -> (ids int64 [Q, k or M], scores f32 [Q, k or M]) device
        tensors: score descending, then id ascending, -0.0 == 0.0; padding (negative ids) goes to the tail as -1 / -inf; an id
        listed twice stays twice.  ValueError for k outside 1..M.  A torch sort over the scores: rerank of most_similar's own
        output returns it unchanged."""
        listed = _listed_ids(queries, ids, self.header.n_rows)
        k = _rerank_k(k, listed[0].shape[1])
        return _rerank(*self._scores(queries, listed, metric), k)


def _int64_ids(ids: np.ndarray, V: int, padding: bool) -> np.ndarray:
    """Integer ids of any width as a C-contiguous int64 array, their range checked ON THE DTYPE THEY CAME IN: a uint64 id of
    2**63 or more would turn negative in the cast -- padding where negative ids are padding.  IndexError for an id that
    reaches V, and, unless negative ids are `padding`, for one below 0."""
    if ids.size and (int(ids.max()) >= V or (not padding and int(ids.min()) < 0)):
        bad = ids[(ids >= V) | (ids < 0)] if not padding else ids[ids >= V]
        raise IndexError(f"row {int(bad.reshape(-1)[0])} outside [0, {V})" + (" (negative ids are padding)" if padding else ""))
    return np.ascontiguousarray(ids, dtype=np.int64)
