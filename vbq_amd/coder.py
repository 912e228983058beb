"""Entropy coder for the rank indices: static-model rANS on the GPU.

The reference stops at ESTIMATING the rate as sum(-log2 freq) with add-n smoothed frequencies
(quantizer.py:138-146, 226-228; utils.py:547).  This module turns the same per-(lambda, channel)
histograms into integer frequency tables and the indices into a bitstream, and decodes it back.
Format: include/vbq.h (vbq_rans_encode_u16).  Nothing here changes the quantization path.
pack_device / unpack_device / encode_packed / decode_packed turn the padded per-segment layout into the contiguous payload of
a compressed file (vbq_amd.bitstream) and back on the device (vbq_rans_pack_u16 / vbq_rans_unpack_u16).
MappedRansCodec is the same segment coder with a table per symbol: a class map picks one of up to four tables at every
position (vbq_rans_map_*_u16; the lambda map of a VBQm file).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, ops
from ._lib import check
from .bitstream import MAX_CLASSES, MAX_PART, check_part  # the format's limits live with the format

PROB_BITS = 15
DEFAULT_SEGMENT = 1024


def quantize_frequencies(counts, add_n_smoothing=1, prob_bits: int = PROB_BITS) -> np.ndarray:
    """Histogram counts [..., T] -> uint16 frequencies [..., T], every entry >= 1, every row summing
    to 2**prob_bits.  Deterministic largest-remainder rounding of the add-n smoothed frequencies
    the reference's entropy model uses (quantizer.py:141-143)."""
    c = np.asarray(counts.cpu().numpy() if isinstance(counts, torch.Tensor) else counts, dtype=np.float64)
    lead, T = c.shape[:-1], c.shape[-1]
    M = 1 << prob_bits
    if T > M:
        raise ValueError("more symbols than probability slots")
    c = c.reshape(-1, T) + float(add_n_smoothing)
    p = c / c.sum(axis=1, keepdims=True)
    out = np.empty(c.shape, dtype=np.int64)
    for r in range(c.shape[0]):
        ideal = p[r] * M
        f = np.maximum(1, np.floor(ideal).astype(np.int64))
        diff = M - int(f.sum())
        if diff > 0:                                    # hand the missing slots to the largest remainders
            order = np.argsort(-(ideal - np.floor(ideal)), kind="stable")
            f[order[:diff]] += 1 if diff <= T else 0
            if diff > T:
                f[order] += diff // T
                f[order[: diff % T]] += 1
        elif diff < 0:                                  # take the surplus from the most probable symbols
            need = -diff
            while need > 0:
                order = np.argsort(-f, kind="stable")
                for j in order:
                    if need == 0:
                        break
                    take = min(need, int(f[j]) - 1, max(1, int(f[j]) // 64))
                    f[j] -= take
                    need -= take
        assert f.sum() == M and f.min() >= 1
        out[r] = f
    return out.reshape(lead + (T,)).astype(np.uint16)


def exact_frequencies(counts, prob_bits: int = PROB_BITS) -> np.ndarray:
    """Counts [T] of the very data a table will code -> uint16 frequencies [T] summing to 2**prob_bits.  Unlike
    `quantize_frequencies` (a model that must code unseen symbols), a symbol that does not occur gets 0: an embedding
    matrix is coded with the table fitted to it.  Every nonzero count gets >= 1, no entry exceeds 2**prob_bits - 1 (the
    encoder divides by f < 2^15): when a single symbol occurs, its neighbour (the next symbol, or the previous one for the
    last) gets 1.  Deterministic largest-remainder rounding; the leftover slots go to the largest remainders, ties to the
    lower symbol, and a surplus is taken from the largest entries."""
    c = np.asarray(counts.cpu().numpy() if isinstance(counts, torch.Tensor) else counts).reshape(-1)
    if c.size and (c.dtype.kind not in "iu" and not np.all(np.isfinite(c)) or np.any(c < 0)):
        raise ValueError("counts must be finite and >= 0")
    c = c.astype(np.int64)
    T, M = c.size, 1 << prob_bits
    if T < 2 or T > M:
        raise ValueError(f"{T} symbols: need 2..{M}")
    used = np.flatnonzero(c)
    if used.size == 0:
        raise ValueError("no symbol occurs: nothing to fit a table to")
    f = np.zeros(T, dtype=np.int64)
    if used.size == 1:
        s = int(used[0])
        f[s] = M - 1
        f[s + 1 if s + 1 < T else s - 1] = 1
        return f.astype(np.uint16)
    cu = c[used]
    ideal = cu.astype(np.float64) * (M / float(cu.sum()))
    fu = np.maximum(1, np.floor(ideal).astype(np.int64))
    diff = M - int(fu.sum())
    if diff > 0:                                        # at most len(used) - 1 slots: one to each of the largest remainders
        order = np.argsort(-(ideal - np.floor(ideal)), kind="stable")
        fu[order[:diff]] += 1
    while diff < 0:                                     # the floor of 1 overshot: take from the largest entries, never below 1
        order = np.argsort(-fu, kind="stable")
        for j in order:
            if diff == 0:
                break
            take = min(-diff, int(fu[j]) - 1, max(1, int(fu[j]) // 64))
            fu[j] -= take
            diff += take
    f[used] = fu
    assert int(f.sum()) == M and int(f.max()) < M and np.all((f > 0) == (c > 0))
    return f.astype(np.uint16)


def ideal_bits(counts, freq, prob_bits: int = PROB_BITS) -> float:
    """Cross-entropy of the data under the quantised table: sum counts * -log2(freq / 2^PB)."""
    c = np.asarray(counts.cpu().numpy() if isinstance(counts, torch.Tensor) else counts, dtype=np.float64)
    return float(np.sum(c * (prob_bits - np.log2(np.asarray(freq, dtype=np.float64)))))


def _raise_status(st: int):
    """The OR-ed status word of vbq_rans_decode_u16 / vbq_rans_unpack_u16 / vbq_rans_map_decode_u16 /
    vbq_rans_decode_window_f32 / vbq_rans_map_decode_window_f32 / vbq_rans_il_decode_u16 / vbq_rans_il_decode_files_u16 (a part counts as a segment in the
    messages) -> VBQError (nothing when 0)."""
    if st:
        what = [m for b, m in ((1, "segment size out of range"), (2, "segment ran out of words"),
                               (4, "left-over words / wrong final state"), (8, "invalid frequency table"),
                               (16, "segment sizes do not add up to the payload length"),
                               (32, "segment id out of range"), (64, "class outside the palette"),
                               (128, "inconsistent window descriptor")) if st & b]
        raise _lib.VBQError("rANS bitstream rejected: " + ", ".join(what))


class RansCodec:
    """Encoder / decoder for u16 rank indices laid out as streams [S, n] (S = L*C planes of K1)."""

    def __init__(self, freq, N: int = 10, segment: Optional[int] = DEFAULT_SEGMENT, *, allow_zero: bool = False):
        """allow_zero=True accepts zero entries (`exact_frequencies`: a table fitted to the data it codes).  Such a table
        codes only symbols whose entry is nonzero; every entry must then stay below 2**15.  segment=None: a codec for the
        interleaved layout alone (the calls that cut streams into segments then raise ValueError)."""
        T = ops.table_size(N)
        # the codec's own copy: a later edit of `freq` is not its table (the device copy is made once)
        self.freq_host = _freq_host(freq).reshape(-1, T).clone()
        sums = self.freq_host.to(torch.int64).sum(dim=1)
        if allow_zero:
            if not bool(torch.all(sums == (1 << PROB_BITS))) or int(self.freq_host.to(torch.int64).max()) >= (1 << PROB_BITS):
                raise ValueError("every frequency row must sum to 2**15 with every entry below 2**15")
        elif not bool(torch.all(sums == (1 << PROB_BITS))) or int(self.freq_host.to(torch.int64).min()) < 1:
            raise ValueError("every frequency row must be >= 1 and sum to 2**15")
        self.N, self.segment, self.T = N, None if segment is None else int(segment), T
        self._freq_dev: Optional[torch.Tensor] = None

    @property
    def n_streams(self) -> int:
        """Streams of one encode / decode call: one per frequency row."""
        return self.freq_host.shape[0]

    def _freq(self, device):
        if self._freq_dev is None or self._freq_dev.device != device:
            self._freq_dev = self.freq_host.to(device).contiguous()
        return self._freq_dev

    def _streams(self, idx, segments: bool = True):
        """The checked index tensor and its geometry -> (idx, S, n, nseg); nseg is None with segments=False (the interleaved
        layout, which has none)."""
        idx = ops._dev(idx, torch.uint16, "idx")
        n = idx.shape[-1]
        S = idx.numel() // max(n, 1)
        if S != self.freq_host.shape[0]:
            raise ValueError(f"{S} index streams but {self.freq_host.shape[0]} frequency rows")
        return idx, S, n, self._nseg(n) if segments else None

    def _nseg(self, n: int) -> int:
        if self.segment is None:
            raise ValueError("this codec was made without a segment: it serves the interleaved layout only")
        return (n + self.segment - 1) // self.segment

    def _decoded(self, device, n: int, launch) -> torch.Tensor:
        """The tail of every decode: idx u16 [S, n] and a zeroed status word, launch(idx, status) -- one or more launches
        that OR their flags into the word --, then ONE synchronisation to read it; VBQError when a flag is set."""
        idx = torch.empty((self.n_streams, n), dtype=torch.uint16, device=device)
        status = torch.zeros(1, dtype=torch.uint32, device=device)
        launch(idx, status)
        _raise_status(int(status.cpu().item()))
        return idx

    # What MappedRansCodec overrides: how the inputs are prepared (`sel` = what its launches take besides: nothing here) and
    # the three launches.
    def _inputs(self, idx, cls):
        """The encoder's side -> (idx, n, nseg, sel)."""
        idx, _, n, nseg = self._streams(idx)
        return idx, n, nseg, None

    def _decode_sel(self, cls, n, device):
        """The decoder's side -> sel."""
        return None

    def _encode(self, idx, sel, n, words, sizes):
        check(_lib.lib().vbq_rans_encode_u16(ops._ptr(idx), self.n_streams, n, self.N, self.segment,
                                             ops._ptr(self._freq(idx.device)), ops._ptr(words), ops._ptr(sizes),
                                             ops._stream(idx)), "vbq_rans_encode_u16")

    def _sizes(self, idx, sel, n, sizes):
        check(_lib.lib().vbq_rans_sizes_u16(ops._ptr(idx), self.n_streams, n, self.N, self.segment,
                                            ops._ptr(self._freq(idx.device)), ops._ptr(sizes), ops._stream(idx)),
              "vbq_rans_sizes_u16")

    def _decode(self, words, sizes, sel, n, idx, status):
        """status: u32 [1] the decoder ORs its flags into (read it with _raise_status)."""
        check(_lib.lib().vbq_rans_decode_u16(ops._ptr(words), ops._ptr(sizes), idx.shape[0], n, self.N, self.segment,
                                             ops._ptr(self._freq(idx.device)), ops._ptr(idx), ops._ptr(status),
                                             ops._stream(idx)), "vbq_rans_decode_u16")

    def encode(self, idx: torch.Tensor, *, _cls=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """idx: u16 device tensor [..., n] with prod(leading dims) == number of frequency rows.
        Returns (words u16 [S, nseg, segment+2], sizes u32 [S, nseg])."""
        idx, n, nseg, sel = self._inputs(idx, _cls)
        words = torch.zeros((self.n_streams, nseg, self.segment + 2), dtype=torch.uint16, device=idx.device)
        sizes = torch.zeros((self.n_streams, nseg), dtype=torch.uint32, device=idx.device)
        self._encode(idx, sel, n, words, sizes)
        return words, sizes

    def sizes(self, idx: torch.Tensor, *, _cls=None) -> torch.Tensor:
        """The sizes `encode` returns -- u32 [S, nseg], 16-bit words per segment -- without the words (vbq_rans_sizes_u16): the
        exact coded length of every segment at 4 bytes of output per segment instead of a padded word buffer."""
        idx, n, nseg, sel = self._inputs(idx, _cls)
        sizes = torch.zeros((self.n_streams, nseg), dtype=torch.uint32, device=idx.device)
        self._sizes(idx, sel, n, sizes)
        return sizes

    def decode(self, words: torch.Tensor, sizes: torch.Tensor, n: int, *, _cls=None) -> torch.Tensor:
        """words / sizes are untrusted (they may come from a file): shapes are checked here, segment sizes and
        word counts in the kernel; a damaged stream raises VBQError instead of returning garbage."""
        words = ops._dev(words, torch.uint16, "words")
        sizes = ops._dev(sizes, torch.uint32, "sizes")
        S = self.n_streams
        nseg = self._nseg(n)
        if words.numel() != S * nseg * (self.segment + 2) or sizes.numel() != S * nseg:
            raise ValueError(f"expected words [{S}, {nseg}, {self.segment + 2}] and sizes [{S}, {nseg}] for {n} symbols per "
                             f"stream, got {tuple(words.shape)} and {tuple(sizes.shape)}")
        sel = self._decode_sel(_cls, n, words.device)
        return self._decoded(words.device, n, lambda idx, status: self._decode(words, sizes, sel, n, idx, status))

    # ------------------------------------------------------------ packed payload (vbq_amd.bitstream, vbq_rans_pack_u16)
    def pack_device(self, words: torch.Tensor, sizes: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The payload of `pack`, built on the device: -> (payload u16 [S * nseg * (segment+2)] whose first `total` words are
        valid, total u64 [1], offsets int64 [S, nseg]), all device tensors; nothing is read back."""
        words = ops._dev(words, torch.uint16, "words")
        sizes = ops._dev(sizes, torch.uint32, "sizes")
        S, nseg = sizes.shape
        if tuple(words.shape) != (S, nseg, self.segment + 2):
            raise ValueError(f"words {tuple(words.shape)} do not match sizes {tuple(sizes.shape)} and segment {self.segment}")
        payload = torch.empty(S * nseg * (self.segment + 2), dtype=torch.uint16, device=words.device)
        offsets = torch.empty((S, nseg), dtype=torch.int64, device=words.device)
        total = torch.empty(1, dtype=torch.uint64, device=words.device)
        self._pack(words, sizes, payload, offsets, total)
        return payload, total, offsets

    def _pack(self, words, sizes, payload, offsets, total):
        S, nseg = sizes.shape
        check(_lib.lib().vbq_rans_pack_u16(ops._ptr(words), ops._ptr(sizes), S, nseg * self.segment, self.segment,
                                           ops._ptr(payload), ops._ptr(offsets), ops._ptr(total), ops._stream(words)),
              "vbq_rans_pack_u16")

    def unpack_device(self, payload: torch.Tensor, sizes: torch.Tensor, n: int, status: Optional[torch.Tensor] = None):
        """vbq_rans_unpack_u16: untrusted payload u16 [n_words] + sizes u16 [S * nseg] -> (words [S, nseg, segment+2],
        sizes u32 [S, nseg], status u32 [1]) in the layout `decode` reads.  Nothing is checked on the host here."""
        payload = ops._dev(payload, torch.uint16, "payload")
        sizes = ops._dev(sizes, torch.uint16, "sizes")
        S = self.n_streams
        nseg = self._nseg(n)
        if sizes.numel() != S * nseg:
            raise ValueError(f"expected {S * nseg} segment sizes for {S} streams of {n} symbols, got {sizes.numel()}")
        dev = payload.device
        words = torch.empty((S, nseg, self.segment + 2), dtype=torch.uint16, device=dev)
        out_sizes = torch.empty((S, nseg), dtype=torch.uint32, device=dev)
        offsets = torch.empty(S * nseg, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.uint32, device=dev) if status is None else ops._status(
            status, 1, dev, (("payload", payload), ("sizes", sizes)))
        check(_lib.lib().vbq_rans_unpack_u16(ops._ptr(payload), payload.numel(), ops._ptr(sizes), S, n, self.segment,
                                             ops._ptr(words), ops._ptr(out_sizes), ops._ptr(offsets), ops._ptr(status),
                                             ops._stream(payload)), "vbq_rans_unpack_u16")
        return words, out_sizes, status

    def encode_packed(self, idx: torch.Tensor, *, _cls=None) -> Tuple[np.ndarray, np.ndarray]:
        """encode + pack on the device -> (sizes u32 [S, nseg], payload u16 [total]) on the host, in TWO device-to-host
        copies: the total together with the sizes, then the payload."""
        idx, n, nseg, sel = self._inputs(idx, _cls)
        dev, S = idx.device, self.n_streams
        words = torch.empty((S, nseg, self.segment + 2), dtype=torch.uint16, device=dev)    # pack reads valid words only
        aux = torch.empty(8 + 4 * S * nseg, dtype=torch.uint8, device=dev)                  # total u64, then sizes u32
        total, sizes = aux[:8].view(torch.uint64), aux[8:].view(torch.uint32).view(S, nseg)
        payload = torch.empty(S * nseg * (self.segment + 2), dtype=torch.uint16, device=dev)
        offsets = torch.empty((S, nseg), dtype=torch.int64, device=dev)
        self._encode(idx, sel, n, words, sizes)
        self._pack(words, sizes, payload, offsets, total)
        h = aux.cpu().numpy()
        n_words = int(h[:8].view(np.uint64)[0])
        return h[8:].view(np.uint32).reshape(S, nseg), payload[:n_words].cpu().numpy()

    def decode_packed(self, payload: torch.Tensor, sizes: torch.Tensor, n: int, *, _cls=None) -> torch.Tensor:
        """unpack + the existing decoder, one status word for both (one synchronisation): u16 indices [S, n].
        A damaged payload raises VBQError."""
        sel = self._decode_sel(_cls, n, payload.device)

        def launch(idx, status):
            words, out_sizes, _ = self.unpack_device(payload, sizes, n, status)
            self._decode(words, out_sizes, sel, n, idx, status)
        return self._decoded(payload.device, n, launch)

    # ------------------------------------------------------------ wave-interleaved layout (bitstream VBQc, vbq_rans_il_*_u16)
    # The S * n symbols in stream-major order are cut every `part` symbols; 64 lanes code a part together (format:
    # include/vbq.h).  `segment` plays no role here: it may be None.
    def _parts(self, n_symbols: int, part) -> int:
        part = int(part)
        check_part(part)
        return (n_symbols + part - 1) // part

    def sizes_interleaved(self, idx: torch.Tensor, part: int) -> torch.Tensor:
        """Words of every part of the interleaved layout -- u32 [P] on the device, P = ceil(S * n / part) -- without the
        words (vbq_rans_il_sizes_u16): the exact coded length."""
        idx, S, n, _ = self._streams(idx, segments=False)
        sizes = torch.zeros(self._parts(S * n, part), dtype=torch.uint32, device=idx.device)
        check(_lib.lib().vbq_rans_il_sizes_u16(ops._ptr(idx), S, n, self.N, int(part), ops._ptr(self._freq(idx.device)),
                                               ops._ptr(sizes), ops._stream(idx)), "vbq_rans_il_sizes_u16")
        return sizes

    def encode_interleaved(self, idx: torch.Tensor, part: int) -> Tuple[np.ndarray, np.ndarray]:
        """-> (sizes u32 [P], payload u16 [n_words]) on the host.  The sizes kernel first, their exclusive scan on the device,
        then the encoder writes every part straight to its place in the payload (no padded buffer, no pack pass).  Two
        device-to-host copies: the sizes (they say how long the payload is), then the payload."""
        idx, S, n, _ = self._streams(idx, segments=False)
        sizes = self.sizes_interleaved(idx, part)
        s64 = sizes.view(torch.int32).to(torch.int64)                                       # (a size is at most 2^24 + 128)
        offsets = torch.cumsum(s64, 0) - s64
        sizes_h = sizes.cpu().numpy()
        n_words = int(sizes_h.sum(dtype=np.int64))
        payload = torch.empty(n_words, dtype=torch.uint16, device=idx.device)
        check(_lib.lib().vbq_rans_il_encode_u16(ops._ptr(idx), S, n, self.N, int(part), ops._ptr(self._freq(idx.device)),
                                                ops._ptr(sizes), ops._ptr(offsets), ops._ptr(payload), n_words,
                                                ops._stream(idx)), "vbq_rans_il_encode_u16")
        return sizes_h, payload.cpu().numpy()

    def _decode_interleaved(self, payload, sizes, n, part, idx, status):
        """One launch of the untrusted decoder; status: u32 [1] it ORs its flags into (read it with _raise_status)."""
        s64 = sizes.view(torch.int32).to(torch.int64) & 0xffffffff
        offsets = torch.cumsum(s64, 0) - s64
        check(_lib.lib().vbq_rans_il_decode_u16(ops._ptr(payload), payload.numel(), ops._ptr(sizes), ops._ptr(offsets),
                                                idx.shape[0], n, self.N, int(part), ops._ptr(self._freq(idx.device)),
                                                ops._ptr(idx), ops._ptr(status), ops._stream(idx)), "vbq_rans_il_decode_u16")

    def decode_interleaved(self, payload: torch.Tensor, sizes: torch.Tensor, n: int, part: int) -> torch.Tensor:
        """payload u16 [n_words] and sizes u32 [P] (device tensors, untrusted: they may come from a file) -> u16 indices
        [S, n].  Shapes are checked here, everything else in the kernel; a damaged stream raises VBQError."""
        payload = ops._dev(payload, torch.uint16, "payload").reshape(-1)
        sizes = ops._dev(sizes, torch.uint32, "sizes").reshape(-1)
        S = self.freq_host.shape[0]
        P = self._parts(S * int(n), part)
        if sizes.numel() != P:
            raise ValueError(f"expected {P} part sizes for {S} streams of {n} symbols in parts of {part}, got {sizes.numel()}")
        return self._decoded(payload.device, int(n),
                             lambda idx, status: self._decode_interleaved(payload, sizes, int(n), part, idx, status))

    @staticmethod
    def compressed_bits(sizes: torch.Tensor) -> int:
        return int(sizes.to(torch.int64).sum().item()) * 16

    @staticmethod
    def pack(words: torch.Tensor, sizes: torch.Tensor) -> bytes:
        """Contiguous byte string: the valid words of every segment, stream-major (host side)."""
        w = words.cpu().numpy()
        sz = sizes.cpu().numpy().astype(np.int64)
        keep = np.arange(w.shape[-1])[None, None, :] < sz[..., None]
        return w[keep].tobytes()


class MappedRansCodec(RansCodec):
    """The segment coder with a table per symbol (vbq_rans_map_*_u16, include/vbq.h "Class-mapped rANS"): freq u16 [P, S, T],
    1 <= P <= 4, and a class map cls [n] with values in [0, P), shared by the S streams -- symbol i of stream s is coded with
    freq[cls[i], s].  Words and sizes have the layout of RansCodec, so its pack / unpack calls serve unchanged."""

    def __init__(self, freq, N: int = 10, segment: int = DEFAULT_SEGMENT):
        f = _freq_host(freq)
        if f.dim() != 3 or not 1 <= f.shape[0] <= MAX_CLASSES or f.shape[2] != ops.table_size(N):
            raise ValueError(f"freq must be [P, S, {ops.table_size(N)}] with 1 <= P <= {MAX_CLASSES}, got {tuple(f.shape)}")
        super().__init__(f, N=N, segment=int(segment))                   # (rows checked there; freq_host is [P * S, T])
        self.P, self.S = int(f.shape[0]), int(f.shape[1])

    @property
    def n_streams(self) -> int:
        return self.S

    def _parts(self, n_symbols, part):
        raise ValueError("the class-mapped coder has no interleaved layout")

    def _classes(self, cls, n: int, device, check: bool) -> torch.Tensor:
        """cls as u8 [n] on the device.  check: ValueError for a class outside [0, P) (the encoder's side; the decoder's
        classes are untrusted and checked in the kernel)."""
        if not isinstance(cls, torch.Tensor):
            cls = torch.from_numpy(np.array(cls))                        # (a copy: the array may be read-only)
        if cls.dtype.is_floating_point or cls.dtype == torch.bool:
            raise ValueError(f"classes must be integers, got {cls.dtype}")
        cls = cls.reshape(-1)
        if cls.numel() != n:
            raise ValueError(f"{cls.numel()} classes for {n} symbols per stream")
        if check and n:                                                  # where the classes are: a host array costs no sync
            lo, hi = torch.aminmax(cls.to(torch.int64))
            if int(lo) < 0 or int(hi) >= self.P:
                raise ValueError(f"class outside [0, {self.P})")
        cls = cls.to(device)
        if cls.dtype != torch.uint8:                                     # (no wrap-around into the palette: the kernel rejects 255)
            cls = cls.to(torch.int64)
            cls = torch.where((cls < 0) | (cls > 255), 255, cls)
        return cls.to(torch.uint8).contiguous()

    def _inputs(self, idx, cls):
        """The checked index tensor [P, S, n] or [S, n] and its class map -> (idx, n, nseg, (n_planes, cls))."""
        idx = ops._dev(idx, torch.uint16, "idx")
        n = idx.shape[-1]
        if tuple(idx.shape) == (self.P, self.S, n) and idx.dim() == 3:
            planes = self.P
        elif tuple(idx.shape) == (self.S, n):
            planes = 1
        else:
            raise ValueError(f"idx must be [{self.P}, {self.S}, n] or [{self.S}, n], got {tuple(idx.shape)}")
        nseg = self._nseg(n)
        return idx, n, nseg, (planes, self._classes(cls, n, idx.device, check=True))

    def _decode_sel(self, cls, n, device):
        return self._classes(cls, n, device, check=False)

    def _encode(self, idx, sel, n, words, sizes):
        check(_lib.lib().vbq_rans_map_encode_u16(ops._ptr(idx), sel[0], ops._ptr(sel[1]), self.P, self.S, n, self.N, self.segment,
                                                 ops._ptr(self._freq(idx.device)), ops._ptr(words), ops._ptr(sizes),
                                                 ops._stream(idx)), "vbq_rans_map_encode_u16")

    def _sizes(self, idx, sel, n, sizes):
        check(_lib.lib().vbq_rans_map_sizes_u16(ops._ptr(idx), sel[0], ops._ptr(sel[1]), self.P, self.S, n, self.N, self.segment,
                                                ops._ptr(self._freq(idx.device)), ops._ptr(sizes), ops._stream(idx)),
              "vbq_rans_map_sizes_u16")

    def _decode(self, words, sizes, cls, n, idx, status):
        check(_lib.lib().vbq_rans_map_decode_u16(ops._ptr(words), ops._ptr(sizes), ops._ptr(cls), self.P, self.S, n, self.N,
                                                 self.segment, ops._ptr(self._freq(idx.device)), ops._ptr(idx), ops._ptr(status),
                                                 ops._stream(idx)), "vbq_rans_map_decode_u16")

    _map_decode = _decode                                                # (the name the tests launch it by)

    def encode(self, idx, cls) -> Tuple[torch.Tensor, torch.Tensor]:
        """idx u16 [P, S, n] (plane p holds the symbols of class p: the encoder picks idx[cls[i], s, i]) or [S, n] (already
        selected); cls [n] integers in [0, P).  -> (words u16 [S, nseg, segment+2], sizes u32 [S, nseg])."""
        return super().encode(idx, _cls=cls)

    def sizes(self, idx, cls) -> torch.Tensor:
        """The sizes `encode` returns, without the words (vbq_rans_map_sizes_u16)."""
        return super().sizes(idx, _cls=cls)

    def decode(self, words, sizes, cls, n: int) -> torch.Tensor:
        """words, sizes and cls are untrusted: shapes are checked here, everything else in the kernel (a class >= P included);
        a damaged stream raises VBQError.  -> u16 indices [S, n]."""
        return super().decode(words, sizes, int(n), _cls=cls)

    def encode_packed(self, idx, cls) -> Tuple[np.ndarray, np.ndarray]:
        """encode + vbq_rans_pack_u16 on the device -> (sizes u32 [S, nseg], payload u16 [total]) on the host, in two
        device-to-host copies."""
        return super().encode_packed(idx, _cls=cls)

    def decode_packed(self, payload, sizes, cls, n: int) -> torch.Tensor:
        """vbq_rans_unpack_u16 + the mapped decoder, one status word for both: u16 indices [S, n]."""
        return super().decode_packed(payload, sizes, int(n), _cls=cls)


def _freq_host(freq) -> torch.Tensor:
    """A frequency table -- tensor on any device, NumPy array of any layout or integer dtype, nested lists -- as a u16 CPU
    tensor; ValueError for entries that are not integers in [0, 65535]."""
    f = freq.detach().cpu() if isinstance(freq, torch.Tensor) else ops.host_tensor(np.asarray(freq))
    if f.dtype != torch.uint16:
        wide = f.to(torch.int64)
        if f.dtype.is_floating_point or f.dtype == torch.bool or bool(((wide < 0) | (wide > 0xFFFF)).any()):
            raise ValueError(f"frequencies must be integers in [0, 65535], got {f.dtype}")
        f = wide.to(torch.uint16)
    return f
