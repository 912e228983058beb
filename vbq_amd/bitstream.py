"""Self-describing byte formats for ONE tensor coded at ONE rate (a compressed file).

Host-only: writing and strictly validating the headers.  Two formats hold one latent tensor at one lambda, coded per channel
(channel c holds its B = prod(shape) / C latents in row order: the [C, B] planes of rank indices):

    b"VBQb"  segments: every channel is a stream cut into segments of `segment` symbols, each an independent rANS stream; the
             payload is what `RansCodec.pack` returns, built on the device by vbq_rans_pack_u16 and taken apart by
             vbq_rans_unpack_u16 (include/vbq.h).  Fixed cost: 6 bytes and the word rounding per segment.
    b"VBQc"  compact: the C * B indices in channel-major order are cut every `part` symbols into P = ceil(C * B / part) parts
             coded by the wave-interleaved coder (include/vbq.h, vbq_rans_il_encode_u16; RansCodec.encode_interleaved /
             decode_interleaved); a part of m symbols takes 128 .. m + 128 words.  Fixed cost: 256 bytes per part.

ChannelwisePriorCDFQuantizer.compress_latents_to_bytes (layout="segments" / "interleaved") writes them and decompress_latents
reads either through `parse_latent`.  A third format (magic b"VBQe", further down) holds one compressed word-embedding matrix:
vbq_amd.embeddings.compress_to_bytes / CompressedEmbeddings, and a fourth (magic b"VBQr", at the end) a matrix whose rows were
quantized to one exact bit budget, as fixed-size records: compress_to_records / RecordEmbeddings.  latent_nbytes / compact_nbytes / embeddings_nbytes give the
exact length of a file without building it, and smallest_rate_within is the byte-budget rule of the rate-control calls
(coded_nbytes / *_to_budget on the quantizer and in vbq_amd.embeddings; smallest_rates_within is the same rule for the F files
of a batch at once).

Layout of the two latent files, every field little-endian (version 1); `unit` is the segment or the part:

    offset  size      field
    0       4         magic b"VBQb" / b"VBQc"
    4       1         version = 1
    5       1         N = max_bits_per_coord (1..10)
    6       1         ndim of the latent shape (>= 1)
    7       1         reserved = 0
    8       4         C, the number of channels (u32)
    12      4         symbols per unit (u32): segment in 1..65533 / part in 1..2^24
    16      8         lambda (f64, finite)
    24      8         n_words, payload length in 16-bit words (u64)
    32      16        digest: blake2b-128 of the sorted code-point table (f32 [C, T]) and the quantised frequency
                      table (u16 [C, T]) of this lambda -- exactly what decoding depends on
    48      8 * ndim  latent shape (u64 each, channel last: shape[-1] == C, every entry >= 1)
    then the size block, words per unit:
      VBQb  2 * C*nseg  segment sizes (u16, each in [2, segment + 2]), nseg = ceil(B / segment), stream-major (channel),
                        then segment
      VBQc  4 * P       part sizes (u32, part p in [128, m_p + 128], m_p = part but for a shorter last part), then 4 zero
                        bytes of padding when P is odd, so that the payload starts 8-byte aligned
    ...     2*n_words payload (u16): the valid words of every unit in the same order; sum(sizes) == n_words

The header is a multiple of 8 bytes long, so the sizes and the payload can be viewed in place.  The parsers raise ValueError
with a specific message on anything malformed -- never struct.error or IndexError -- and check every size with vectorised
NumPy before anything reaches the device (the kernels' own checks are the second line of defence).  `parse` rejects a compact
file by its magic and `parse_compact` rejects a file in segments.

A fifth format (magic b"VBQm", after the two latent files below) holds one latent tensor coded at SEVERAL lambdas: a palette
of up to four and a class per latent position saying which one applies there (a lambda map: compress_latents_to_bytes_mapped;
decompress_latents reads it by its magic).  write_mapped / parse_mapped / mapped_nbytes; `parse_latent` rejects it.
"""
from __future__ import annotations

import hashlib
import math
import struct
from collections import namedtuple
from dataclasses import dataclass
from typing import ClassVar, Tuple

import numpy as np

MAGIC = b"VBQb"
VERSION = 1
COMPACT_MAGIC = b"VBQc"
COMPACT_VERSION = 1
MAX_N = 10                                   # the coder's limit (vbq_rans_encode_u16)
MAX_SEGMENT = 65533                          # seg + 2 must fit in a u16 size
MAX_PART = 1 << 24                           # the coder's limit (vbq_rans_il_encode_u16)
MAX_CLASSES = 4                              # the coder's limit (vbq_rans_map_encode_u16); a class takes 2 bits in a VBQm file
PART_STATE_WORDS = 128                       # the 64 lane states every part begins with
_FIXED = struct.Struct("<4sBBBBIIdQ16s")     # the 48 bytes before the shape
assert _FIXED.size == 48


def digest(sorted_table, freq) -> bytes:
    """blake2b-128 over the sorted code points (f32 [C, T]) and the quantised frequencies (u16 [C, T]) of one lambda."""
    h = hashlib.blake2b(digest_size=16)
    h.update(np.ascontiguousarray(sorted_table, dtype="<f4").tobytes())
    h.update(np.ascontiguousarray(freq, dtype="<u2").tobytes())
    return h.digest()


def check_segment(segment, unit="segment", limit=MAX_SEGMENT):
    """ValueError unless 1 <= segment <= limit: the one statement of the range of a segment (and, through check_part, a part)."""
    if not 1 <= segment <= limit:
        raise ValueError(f"{unit} {segment} outside [1, {limit}]")


def check_part(part):
    check_segment(part, "part", MAX_PART)


# ---- what the three formats share: the checks of the size block and of the file's length
def _check_sizes(sizes: np.ndarray, unit: str, lo: int, hi, n_words: int):
    """Every size in [lo, hi] (hi: one bound, or one per size) and their sum n_words."""
    s = sizes.astype(np.int64)
    wrong = (s < lo) | (s > hi)
    if wrong.any():
        bad = int(np.flatnonzero(wrong)[0])
        raise ValueError(f"{unit} size {int(s[bad])} at position {bad} outside [{lo}, {int(np.broadcast_to(hi, s.shape)[bad])}]")
    total = int(s.sum())
    if total != n_words:
        raise ValueError(f"{unit} sizes add up to {total} words, the header says {n_words}")


def _flat_sizes(sizes, count: int, unit: str) -> np.ndarray:
    """A writer's sizes as a flat array of `count` entries."""
    sizes = np.asarray(sizes).reshape(-1)
    if sizes.size != count:
        raise ValueError(f"{sizes.size} {unit} sizes, the shape needs {count}")
    return sizes


def _checked_payload(payload, n_words: int) -> np.ndarray:
    payload = np.ascontiguousarray(payload, dtype="<u2").reshape(-1)
    if payload.size != n_words:
        raise ValueError(f"payload of {payload.size} words, the header says {n_words}")
    return payload


def _unpack_fixed(mv, fixed: struct.Struct):
    if len(mv) < fixed.size:
        raise ValueError(f"truncated: {len(mv)} bytes, the fixed header alone is {fixed.size}")
    return fixed.unpack_from(mv, 0)


def _read_shape(mv, fixed: struct.Struct, ndim: int, what: str) -> Tuple[int, ...]:
    hlen = fixed.size + 8 * ndim
    if len(mv) < hlen:
        raise ValueError(f"truncated in the {what} shape: {len(mv)} bytes, the header is {hlen}")
    return tuple(int(d) for d in np.frombuffer(mv, dtype="<u8", count=ndim, offset=fixed.size))


def _check_length(nbytes: int, need: int, parts: str):
    if nbytes < need:
        raise ValueError(f"truncated: {nbytes} bytes, {parts} need {need}")
    if nbytes > need:
        raise ValueError(f"{nbytes - need} trailing bytes after the payload")


# ---- the two latent files
@dataclass(frozen=True)
class _LatentHeader:
    """What the two latent headers share; a subclass adds its unit field (`segment` / `part`) and states what differs."""
    N: int
    C: int
    shape: Tuple[int, ...]
    lamb: float
    digest: bytes
    n_words: int

    @property
    def n_rows(self) -> int:
        """Symbols per stream: the latents of one channel."""
        return math.prod(self.shape) // self.C

    @property
    def nbytes(self) -> int:
        """Length of the header itself (where the sizes start)."""
        return _FIXED.size + 8 * len(self.shape)

    @property
    def unit(self) -> int:
        return getattr(self, self.UNIT)

    def check(self):
        N, C, shape, lamb = self.N, self.C, tuple(int(d) for d in self.shape), float(self.lamb)
        if not 1 <= N <= MAX_N:
            raise ValueError(f"N = {N} outside [1, {MAX_N}]")
        if C < 1:
            raise ValueError("zero channels")
        if not 1 <= len(shape) <= 255:
            raise ValueError(f"latent shape with {len(shape)} dimensions")
        if any(d < 1 for d in shape):
            raise ValueError(f"empty latent shape {shape}")
        if shape[-1] != C:
            raise ValueError(f"latent shape {shape} is not channel-last for C = {C}")
        if math.prod(shape) % C:
            raise ValueError(f"latent shape {shape}: {math.prod(shape)} elements are not a multiple of C = {C}")
        if math.prod(shape) >= 2 ** 62:
            raise ValueError(f"latent shape {shape} is too large")
        if not math.isfinite(lamb):
            raise ValueError(f"non-finite lambda {lamb}")
        check_segment(self.unit, self.UNIT, self.LIMIT)
        if len(self.digest) != 16:
            raise ValueError("digest must be 16 bytes")
        if self.n_words < 0:
            raise ValueError("negative payload length")


@dataclass(frozen=True)
class Header(_LatentHeader):
    segment: int
    MAGIC: ClassVar = MAGIC
    VERSION: ClassVar = VERSION
    KIND: ClassVar = ""                      # "not a VBQ bitstream", "unknown bitstream version"
    FOREIGN: ClassVar = {}
    UNIT: ClassVar = "segment"
    LIMIT: ClassVar = MAX_SEGMENT
    SIZE_DTYPE: ClassVar = "<u2"

    @property
    def nseg(self) -> int:
        return (self.n_rows + self.segment - 1) // self.segment

    @property
    def n_sizes(self) -> int:
        return self.C * self.nseg

    @property
    def sizes_nbytes(self) -> int:
        return 2 * self.n_sizes

    def size_range(self):
        return 2, self.segment + 2


@dataclass(frozen=True)
class CompactHeader(_LatentHeader):
    part: int
    MAGIC: ClassVar = COMPACT_MAGIC
    VERSION: ClassVar = COMPACT_VERSION
    KIND: ClassVar = "compact "
    FOREIGN: ClassVar = {Header.MAGIC: "a latent bitstream in segments (magic b'VBQb'), not a compact one"}
    UNIT: ClassVar = "part"
    LIMIT: ClassVar = MAX_PART
    SIZE_DTYPE: ClassVar = "<u4"

    @property
    def n_parts(self) -> int:
        return (math.prod(self.shape) + self.part - 1) // self.part

    n_sizes = n_parts

    @property
    def sizes_nbytes(self) -> int:
        """Length of the size block, padding included."""
        return 4 * self.n_parts + 4 * (self.n_parts & 1)

    def size_range(self):
        hi = np.full(self.n_parts, self.part + PART_STATE_WORDS, dtype=np.int64)
        hi[-1] = math.prod(self.shape) - (self.n_parts - 1) * self.part + PART_STATE_WORDS
        return PART_STATE_WORDS, hi


def _write_latent(h: _LatentHeader, sizes, payload) -> bytes:
    h.check()
    sizes = _flat_sizes(sizes, h.n_sizes, h.UNIT)
    _check_sizes(sizes, h.UNIT, *h.size_range(), h.n_words)
    payload = _checked_payload(payload, h.n_words)
    head = _FIXED.pack(h.MAGIC, h.VERSION, h.N, len(h.shape), 0, h.C, h.unit, float(h.lamb), h.n_words, h.digest)
    block = sizes.astype(h.SIZE_DTYPE).tobytes()
    return b"".join([head, np.asarray(h.shape, dtype="<u8").tobytes(), block, bytes(h.sizes_nbytes - len(block)),
                     payload.tobytes()])


def _latent_nbytes(cls, shape, C, unit, n_words) -> int:
    h = cls(N=MAX_N, C=int(C), shape=tuple(int(d) for d in shape), lamb=0.0, digest=bytes(16), n_words=int(n_words),
            **{cls.UNIT: int(unit)})
    h.check()
    return h.nbytes + h.sizes_nbytes + 2 * h.n_words


def _parse_latent(data, cls):
    mv = memoryview(data).cast("B")
    magic, version, N, ndim, reserved, C, unit, lamb, n_words, dig = _unpack_fixed(mv, _FIXED)
    if magic != cls.MAGIC:
        raise ValueError(cls.FOREIGN.get(magic) or f"not a {cls.KIND}VBQ bitstream (magic {magic!r})")
    if version != cls.VERSION:
        raise ValueError(f"unknown {cls.KIND}bitstream version {version}")
    if reserved != 0:
        raise ValueError(f"reserved header byte is {reserved}, not 0")
    if ndim < 1:
        raise ValueError("latent shape with 0 dimensions")
    shape = _read_shape(mv, _FIXED, ndim, "latent")
    h = cls(N=N, C=C, shape=shape, lamb=float(lamb), digest=bytes(dig), n_words=n_words, **{cls.UNIT: unit})
    h.check()
    start = h.nbytes + h.sizes_nbytes                                # of the payload
    _check_length(len(mv), start + 2 * n_words, f"header, {h.n_sizes} {cls.UNIT} sizes and {n_words} payload words")
    sizes = np.frombuffer(mv, dtype=cls.SIZE_DTYPE, count=h.n_sizes, offset=h.nbytes)
    if any(mv[h.nbytes + sizes.nbytes: start]):
        raise ValueError(f"padding after the {cls.UNIT} sizes is not zero")
    _check_sizes(sizes, cls.UNIT, *h.size_range(), n_words)
    return h, sizes, start


def write(header: Header, sizes, payload) -> bytes:
    """header + sizes (any integer array of C * nseg entries) + payload (u16 [n_words]) -> bytes.  Validates as `parse` does."""
    return _write_latent(header, sizes, payload)


def write_compact(header: CompactHeader, sizes, payload) -> bytes:
    """header + sizes (any integer array of P entries) + payload (u16 [n_words]) -> bytes.  Validates as `parse_compact` does."""
    return _write_latent(header, sizes, payload)


def latent_nbytes(shape, C, segment, n_words) -> int:
    """len(write(...)) of a latent tensor of `shape` (channel-last, C channels) in segments of `segment` symbols with a payload
    of n_words 16-bit words, without building the file.  ValueError for fields `write` rejects."""
    return _latent_nbytes(Header, shape, C, segment, n_words)


def compact_nbytes(shape, C, part, n_words) -> int:
    """The same for `write_compact`, in parts of `part` symbols."""
    return _latent_nbytes(CompactHeader, shape, C, part, n_words)


def parse(data) -> Tuple[Header, np.ndarray, int]:
    """bytes -> (header, sizes u16 [C * nseg] (a read-only view into `data`), byte offset of the payload).
    ValueError on anything malformed."""
    return _parse_latent(data, Header)


def parse_compact(data) -> Tuple[CompactHeader, np.ndarray, int]:
    """bytes -> (header, sizes u32 [P] (a read-only view into `data`), byte offset of the payload).
    ValueError on anything malformed."""
    return _parse_latent(data, CompactHeader)


def parse_latent(data):
    """What `parse_compact` returns for a compact file, and what `parse` returns -- or raises -- for everything else."""
    compact = bytes(memoryview(data).cast("B")[:4]) == COMPACT_MAGIC
    return _parse_latent(data, CompactHeader if compact else Header)


# ---- windows of a file in segments (ChannelwisePriorCDFQuantizer.decompress_latents_window / _batch; include/vbq.h, "Window
# decode").  The leading axes of a latent tensor (its shape without the channel axis) number the rows of every stream in row
# order; a region is one slice per leading axis, and the kernel follows a row's position in at most three nested levels.
def _region_axes(leading_shape, region):
    """The region normalised -> [(d, start, stop)] per leading axis, stop >= start."""
    shape = tuple(int(d) for d in leading_shape)
    if any(d < 1 for d in shape):
        raise ValueError(f"empty leading shape {shape}")
    region = () if region is None else (region,) if isinstance(region, slice) else tuple(region)
    if len(region) > len(shape):
        raise ValueError(f"a region of {len(region)} slices for {len(shape)} leading axes")
    axes = []
    for axis, d in enumerate(shape):
        sl = region[axis] if axis < len(region) else slice(None)
        if not isinstance(sl, slice):
            raise ValueError(f"region entry {axis} is {type(sl).__name__}, not a slice (an index would drop the axis)")
        if sl.step not in (None, 1):
            raise ValueError(f"region entry {axis} has step {sl.step}: only step 1 is a box")
        try:
            s, e, _ = sl.indices(d)
        except TypeError as err:
            raise ValueError(f"region entry {axis}: {err}") from None
        axes.append((d, s, max(e, s)))
    return axes


def _collapse(axes, full=None):
    """Nested levels [(D, lo, hi)] of a normalised region, greedily: an axis merges into the level before it when it is taken in
    full (full[axis] where given: several files that must share one collapse) or when that level has extent 1."""
    levels = []
    for axis, (d, s, e) in enumerate(axes):
        whole = (s == 0 and e == d) if full is None else full[axis]
        if levels and (whole or levels[-1][2] - levels[-1][1] == 1):
            D, lo, hi = levels[-1]
            levels[-1] = (D * d, lo * d + s, (hi - 1) * d + e)
        else:
            levels.append((d, s, e))
    return levels


def _three_levels(levels):
    if len(levels) > 3:
        raise ValueError(f"the region needs {len(levels)} nested levels, the window decode has three: take more axes in full "
                         "or at extent 1")
    levels = [(1, 0, 1)] * (3 - len(levels)) + levels
    return tuple(tuple(int(l[k]) for l in levels) for k in range(3))


def region_box(leading_shape, region):
    """A region of the leading axes -> (dims, lo, hi, extents): the box [lo[k], hi[k]) in a geometry of three nested levels
    dims = (D0, D1, D2) with prod(dims) == prod(leading_shape) and row b = (i0 D1 + i1) D2 + i2, and the extent of every
    ORIGINAL axis (the shape of the result).  `region` is a tuple of slices of step 1 or None, one per leading axis, normalised
    as slice.indices does; fewer than the axes leaves the trailing axes full.  ValueError for an int, another step, too many
    entries, and for a region that does not collapse to three levels."""
    axes = _region_axes(leading_shape, region)
    dims, lo, hi = _three_levels(_collapse(axes))
    return dims, lo, hi, tuple(e - s for _, s, e in axes)


def region_boxes(leading_shapes, regions):
    """region_box for several files whose boxes must have the same extents at every LEVEL (one launch decodes them all):
    -> ([(dims, lo, hi)] per file, extents).  The files share one collapse -- an axis merges when EVERY file takes it in full,
    or into a level of extent 1 -- so files of different shapes still agree on the box.  ValueError when the extents differ."""
    axes = [_region_axes(shape, region) for shape, region in zip(leading_shapes, regions)]
    if not axes:
        return [], ()
    extents = [tuple(e - s for _, s, e in a) for a in axes]
    for i, ext in enumerate(extents):
        if ext != extents[0]:
            raise ValueError(f"file {i}: a region of extents {ext}, file 0 has {extents[0]}: one call decodes boxes of one shape")
    full = [all(a[k][1] == 0 and a[k][2] == a[k][0] for a in axes) for k in range(len(axes[0]))]
    return [_three_levels(_collapse(a, full)) for a in axes], extents[0]


def box_segments(dims, lo, hi, segment) -> np.ndarray:
    """The segments of `segment` symbols that hold at least one row of the box (region_box) -> int32, ascending."""
    check_segment(segment)
    dims, lo, hi = (tuple(int(v) for v in t) for t in (dims, lo, hi))
    if not (len(dims) == len(lo) == len(hi) == 3) or any(not 0 <= l <= h <= d for d, l, h in zip(dims, lo, hi)):
        raise ValueError(f"box [{lo}, {hi}) does not lie in {dims}")
    if any(h == l for l, h in zip(lo, hi)):
        return np.zeros(0, np.int32)
    nseg = (math.prod(dims) + segment - 1) // segment
    if nseg > np.iinfo(np.int32).max:
        raise ValueError(f"{nseg} segments per stream are too many")
    # one run of consecutive rows per (i0, i1) of the box; the union of their segment ranges through a difference array
    i0 = np.arange(lo[0], hi[0], dtype=np.int64)[:, None]
    i1 = np.arange(lo[1], hi[1], dtype=np.int64)[None, :]
    first = ((i0 * dims[1] + i1) * dims[2]).reshape(-1)
    mark = np.zeros(nseg + 1, np.int64)
    np.add.at(mark, (first + lo[2]) // segment, 1)
    np.add.at(mark, (first + hi[2] - 1) // segment + 1, -1)
    return np.flatnonzero(np.cumsum(mark[:-1]) > 0).astype(np.int32)


# ---- batches of files in segments, written (ChannelwisePriorCDFQuantizer.compress_latents_to_bytes_batch; include/vbq.h, "Batch
# encode").  One encode launch codes every segment of every file: the plan says where a file's rows sit among the rows solved at
# its lambda, where its segments go, and which 64 segments share a workgroup.
ENCODE_BLOCK = 64                            # items per workgroup of vbq_rans_encode_files_u16
ENCODE_ROW_ALIGN = 8                         # a file's run of rows starts at a multiple of 8 rows: 16 bytes of u16 indices
MAX_BATCH_FILES = 65535                      # the kernel's limit (vbq_rans_encode_files_u16)
EncodePlan = namedtuple("EncodePlan", "nseg seg_base M row0 group_rows group_row_base n_rows files items")


def _plan_inputs(rows, tables, C, n_tables):
    """The checks encode_plan and compact_plan share -> (C, rows int64 [F], tables int64 [F], F, n_tables)."""
    C = int(C)
    if C < 1:
        raise ValueError("zero channels")
    n = np.asarray(rows, dtype=np.int64).reshape(-1)
    tab = np.asarray(tables, dtype=np.int64).reshape(-1)
    F = n.size
    if tab.size != F:
        raise ValueError(f"{tab.size} tables for {F} files")
    if F > MAX_BATCH_FILES:
        raise ValueError(f"{F} files: one call takes at most {MAX_BATCH_FILES}")
    if F and int(n.min()) < 1:
        raise ValueError(f"file {int(np.flatnonzero(n < 1)[0])} has no rows")
    n_tables = (int(tab.max()) + 1 if F else 0) if n_tables is None else int(n_tables)
    if F and (int(tab.min()) < 0 or int(tab.max()) >= n_tables):
        raise ValueError(f"table outside [0, {n_tables})")
    return C, n, tab, F, n_tables


def _row_groups(n, tab, n_tables):
    """The row layout of a batch (see encode_plan) -> (row0 [F], group_rows [n_tables], group_row_base [n_tables]): the files
    of a table next to each other in file order, each file's run of rows rounded up to ENCODE_ROW_ALIGN."""
    padded = (n + ENCODE_ROW_ALIGN - 1) // ENCODE_ROW_ALIGN * ENCODE_ROW_ALIGN
    row0 = np.zeros(n.size, np.int64)
    group_rows = np.zeros(n_tables, np.int64)
    for t in range(n_tables):
        fs = np.flatnonzero(tab == t)
        run = np.cumsum(padded[fs])
        row0[fs] = run - padded[fs]
        group_rows[t] = run[-1] if fs.size else 0
    return row0, group_rows, np.cumsum(group_rows) - group_rows


def encode_plan(rows, tables, segment, C, n_tables=None) -> EncodePlan:
    """What vbq_rans_encode_files_u16 reads, from the rows per channel n_f >= 1 of F files, their table numbers (the files'
    lambdas, 0 .. n_tables - 1; default n_tables: the largest + 1), the segment length and the number of channels C:

        nseg            int64 [F]         ceil(n_f / segment)
        seg_base, M     int64 [F], int    the file-major exclusive sum of C * nseg_f and its total: a file's size block is
                                          sizes[seg_base_f : seg_base_f + C * nseg_f] of the M slots
        row0            int64 [F]         the files of a table sit next to each other, in file order, in that table's group
                                          of rows; file f owns rows [row0_f, row0_f + n_f) of its group, row0_f a multiple of
                                          ENCODE_ROW_ALIGN (the rows up to the next file's are padding: solved, never coded)
        group_rows      int64 [n_tables]  B_g, the rows of every group, padding included (the index planes are [C, B_g])
        group_row_base  int64 [n_tables]  the rows of the groups before it; n_rows their total.  The indices of all groups
                                          are one array: group g's planes start at element C * group_row_base_g
        files           int64 [F, 6]      the descriptors: idx_base = C * group_row_base_g + row0_f, idx_stride = B_g, n_f,
                                          seg_base_f, table, 0
        items           int32 [n_items, 2]  the work items (file, segment): table by table, within a table file by file and
                                          segment by segment, every table's list padded with (-1, -1) to a multiple of
                                          ENCODE_BLOCK -- so every block of ENCODE_BLOCK items holds one table only

    ValueError for a bad segment, C < 1, a row count < 1, a table outside [0, n_tables) or more than MAX_BATCH_FILES files."""
    check_segment(segment)
    segment = int(segment)
    C, n, tab, F, n_tables = _plan_inputs(rows, tables, C, n_tables)
    nseg = (n + segment - 1) // segment
    if F and int(nseg.max()) > np.iinfo(np.int32).max:
        raise ValueError(f"{int(nseg.max())} segments per stream are too many")
    per_file = C * nseg
    seg_base = np.cumsum(per_file) - per_file
    row0, group_rows, group_row_base = _row_groups(n, tab, n_tables)
    lists = []
    for t in range(n_tables):
        fs = np.flatnonzero(tab == t)
        reps = nseg[fs]
        first = np.cumsum(reps) - reps
        item = np.stack([np.repeat(fs, reps), np.arange(int(reps.sum())) - np.repeat(first, reps)], axis=1)
        lists += [item, np.full((-item.shape[0] % ENCODE_BLOCK, 2), -1, np.int64)]
    items = (np.concatenate(lists) if lists else np.zeros((0, 2), np.int64)).astype(np.int32)
    files = np.stack([C * group_row_base[tab] + row0, group_rows[tab], n, seg_base, tab, np.zeros(F, np.int64)], axis=1) \
        if F else np.zeros((0, 6), np.int64)
    return EncodePlan(nseg, seg_base, int(per_file.sum()), row0, group_rows, group_row_base, int(group_rows.sum()),
                      np.ascontiguousarray(files, dtype=np.int64), np.ascontiguousarray(items))


# ---- batches of compact files, written and read (ChannelwisePriorCDFQuantizer.compress_latents_to_compact_batch /
# decompress_latents_compact_batch; include/vbq.h, "Compact batch").  One wave codes one part, so the plan lists every part of
# every file; the rows lie as encode_plan lays them.
COMPACT_FIELDS = 8                           # idx_base, idx_stride, n, part_base, table, part, word_base, n_words_f
CompactPlan = namedtuple("CompactPlan", "n_parts part_base P_all row0 group_rows group_row_base n_rows files items")


def compact_plan(rows, tables, parts, C, n_tables=None) -> CompactPlan:
    """What vbq_rans_il_sizes_files_u16 / _encode_files_u16 / _decode_files_u16 read, from the rows per channel n_f >= 1 of F
    files, their table numbers, their part lengths (one for all files or one per file) and the number of channels C:

        n_parts         int64 [F]         P_f = ceil(C * n_f / part_f)
        part_base, P_all  int64 [F], int  the file-major exclusive sum of P_f and its total: a file's size block is
                                          sizes[part_base_f : part_base_f + P_f] of the P_all entries
        row0, group_rows, group_row_base, n_rows   the row layout of encode_plan, unchanged: the files of a table next to each
                                          other, every file's run of rows starting at a multiple of ENCODE_ROW_ALIGN
        files           int64 [F, 8]      the descriptors: idx_base = C * group_row_base_g + row0_f, idx_stride = B_g, n_f,
                                          part_base_f, table, part_f, and word_base = n_words_f = 0 -- the reader fills the
                                          last two in from its files, the encode side does not read them
        items           int32 [P_all, 2]  the work items (file, part), file by file and part by part; no padding

    ValueError for a bad part, C < 1, a row count < 1, a table outside [0, n_tables) or more than MAX_BATCH_FILES files."""
    C, n, tab, F, n_tables = _plan_inputs(rows, tables, C, n_tables)
    part = np.asarray(parts).reshape(-1)
    if part.size == 1:
        part = np.repeat(part, F)
    if part.size != F:
        raise ValueError(f"{part.size} parts for {F} files")
    for v in part.tolist():
        check_part(v)
    part = part.astype(np.int64)
    n_parts = (C * n + part - 1) // part
    part_base = np.cumsum(n_parts) - n_parts
    P_all = int(n_parts.sum())
    if P_all > np.iinfo(np.int32).max:
        raise ValueError(f"{P_all} parts are too many")
    row0, group_rows, group_row_base = _row_groups(n, tab, n_tables)
    items = np.stack([np.repeat(np.arange(F), n_parts), np.arange(P_all) - np.repeat(part_base, n_parts)], axis=1) \
        if F else np.zeros((0, 2), np.int64)
    zero = np.zeros(F, np.int64)
    files = np.stack([C * group_row_base[tab] + row0, group_rows[tab], n, part_base, tab, part, zero, zero], axis=1) \
        if F else np.zeros((0, COMPACT_FIELDS), np.int64)
    return CompactPlan(n_parts, part_base, P_all, row0, group_rows, group_row_base, int(group_rows.sum()),
                       np.ascontiguousarray(files, dtype=np.int64), np.ascontiguousarray(items, dtype=np.int32))


def compact_file_words(sizes, plan: CompactPlan) -> np.ndarray:
    """The words of every file of `plan` from the part sizes u32 [..., P_all] (vbq_rans_il_sizes_files_u16, or one row per
    lambda from vbq_rans_il_rates_files_u16) -> int64 [..., F]: the sum of sizes[..., part_base_f : part_base_f + P_f]."""
    sizes = np.asarray(sizes)
    if sizes.ndim < 1 or sizes.shape[-1] != plan.P_all or sizes.dtype.kind not in "iu":
        raise ValueError(f"sizes must be an integer array [..., {plan.P_all}], got {sizes.dtype} {sizes.shape}")
    run = np.zeros(sizes.shape[:-1] + (plan.P_all + 1,), np.int64)
    np.cumsum(sizes, axis=-1, dtype=np.int64, out=run[..., 1:])
    return run[..., plan.part_base + plan.n_parts] - run[..., plan.part_base]


# ---------------------------------------------------------------------------------------------------------------------------
# The lambda-map latent file: ONE latent tensor coded at up to four lambdas (ChannelwisePriorCDFQuantizer.
# compress_latents_to_bytes_mapped).  A palette of P lambdas and a class per latent POSITION (the latent shape without its
# channel axis, B = prod(shape) / C positions in row order, shared by the C channels): channel c is stream c in segments as in
# a VBQb file, and its symbol b is coded with the frequency table of (lambda[class[b]], c) -- the class-mapped coder of
# include/vbq.h (vbq_rans_map_encode_u16).  The decoder needs no lambda, only the tables; the digests say which.
# Layout, every field little-endian (version 1):
#
#     offset  size      field
#     0       4         magic b"VBQm"
#     4       1         version = 1
#     5       1         N = max_bits_per_coord (1..10)
#     6       1         ndim of the latent shape (>= 1)
#     7       1         P, the number of classes (1..4)
#     8       4         C, the number of channels (u32)
#     12      4         segment, symbols per rANS segment (u32, 1..65533)
#     16      8         n_words, payload length in 16-bit words (u64)
#     24      8 * P     the lambdas (f64, finite, distinct), class 0 first
#     ...     16 * P    digests: `digest` of each lambda's tables, in the same order
#     ...     8 * ndim  latent shape (u64 each, channel last: shape[-1] == C, every entry >= 1)
#     ...               class block: 2 bits per position, position b in byte b // 4 at bits 2 (b % 4) and 2 (b % 4) + 1;
#                       ceil(B / 4) bytes, zero-padded to a multiple of 8 bytes; padding bits are zero, every class < P
#     ...     2*C*nseg  segment sizes (u16, each in [2, segment + 2]), nseg = ceil(B / segment), stream-major, as VBQb
#     ...     2*n_words payload (u16), as VBQb; sum(sizes) == n_words
#
# `parse_mapped` raises ValueError with a specific message on anything malformed, never struct.error or IndexError, and checks
# every class and size with vectorised NumPy before anything reaches the device.
# ---------------------------------------------------------------------------------------------------------------------------
MAPPED_MAGIC = b"VBQm"
MAPPED_VERSION = 1
_MAP_FIXED = struct.Struct("<4sBBBBIIQ")     # the 24 bytes before the lambdas
assert _MAP_FIXED.size == 24
_MAP_FOREIGN = {MAGIC: "a latent bitstream at one lambda (magic b'VBQb'), not a lambda-map file",
                COMPACT_MAGIC: "a compact latent bitstream (magic b'VBQc'), not a lambda-map file"}


def pack_classes(classes) -> bytes:
    """Classes (integers in [0, 4), any shape, row order) -> the class block of a VBQm file, padding included."""
    c = np.ascontiguousarray(classes).reshape(-1).astype(np.uint8)
    B = c.size
    q = np.zeros(4 * ((B + 3) // 4), dtype=np.uint8)
    q[:B] = c
    q = q.reshape(-1, 4)
    block = (q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)).astype(np.uint8).tobytes()
    return block + bytes(-len(block) % 8)


def unpack_classes(block, B: int) -> np.ndarray:
    """The first B classes of a class block (bytes or a u8 array) -> u8 [B]."""
    b = np.frombuffer(block, dtype=np.uint8, count=(B + 3) // 4)
    return ((b[:, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3).reshape(-1)[:B]


@dataclass(frozen=True)
class MappedHeader:
    N: int
    C: int
    shape: Tuple[int, ...]
    segment: int
    lambs: Tuple[float, ...]
    digests: Tuple[bytes, ...]
    n_words: int

    @property
    def P(self) -> int:
        return len(self.lambs)

    @property
    def n_rows(self) -> int:
        """B: latent positions = symbols per stream."""
        return math.prod(self.shape) // self.C

    @property
    def nseg(self) -> int:
        return (self.n_rows + self.segment - 1) // self.segment

    @property
    def n_sizes(self) -> int:
        return self.C * self.nseg

    @property
    def nbytes(self) -> int:
        """Length of the header itself (where the class block starts)."""
        return _MAP_FIXED.size + 24 * self.P + 8 * len(self.shape)

    @property
    def classes_nbytes(self) -> int:
        """Length of the class block, padding included."""
        return 8 * ((self.n_rows + 31) // 32)

    @property
    def sizes_offset(self) -> int:
        return self.nbytes + self.classes_nbytes

    @property
    def sizes_nbytes(self) -> int:
        return 2 * self.n_sizes

    @property
    def total_nbytes(self) -> int:
        return self.sizes_offset + self.sizes_nbytes + 2 * self.n_words

    def check(self):
        if not 1 <= self.P <= MAX_CLASSES:
            raise ValueError(f"P = {self.P} classes outside [1, {MAX_CLASSES}]")
        if len(self.digests) != self.P:
            raise ValueError(f"{len(self.digests)} digests for {self.P} lambdas")
        # what a latent file at one lambda checks: N, C, the shape, the segment, a 16-byte digest, n_words -- per lambda
        for lamb, dig in zip(self.lambs, self.digests):
            Header(N=self.N, C=self.C, shape=self.shape, lamb=lamb, digest=dig, n_words=self.n_words, segment=self.segment).check()
        if len(set(float(l) for l in self.lambs)) != self.P:
            raise ValueError(f"repeated lambda in the palette {tuple(float(l) for l in self.lambs)}")


def _mapped_header(h: MappedHeader) -> MappedHeader:
    h = MappedHeader(N=int(h.N), C=int(h.C), shape=tuple(int(d) for d in h.shape), segment=int(h.segment),
                     lambs=tuple(float(l) for l in h.lambs), digests=tuple(bytes(d) for d in h.digests), n_words=int(h.n_words))
    h.check()
    return h


def _check_classes(classes: np.ndarray, P: int):
    """classes: u8, any shape.  ValueError naming the first position whose class is >= P."""
    wrong = classes >= P
    if wrong.any():
        bad = int(np.flatnonzero(wrong)[0])
        raise ValueError(f"class {int(classes.reshape(-1)[bad])} at position {bad} is not below P = {P}")


def write_mapped(header: MappedHeader, classes, sizes, payload) -> bytes:
    """header + classes (integers in [0, P), B of them in any shape) + sizes (any integer array of C * nseg entries) + payload
    (u16 [n_words]) -> bytes.  Validates as `parse_mapped` does."""
    h = _mapped_header(header)
    classes = np.asarray(classes)
    if classes.dtype.kind not in "iu":
        raise ValueError(f"classes must be integers, got {classes.dtype}")
    classes = classes.reshape(-1)
    if classes.size != h.n_rows:
        raise ValueError(f"{classes.size} classes, the shape has {h.n_rows} positions")
    if classes.size and int(classes.min()) < 0:
        raise ValueError(f"negative class {int(classes.min())}")
    _check_classes(np.minimum(classes, 255).astype(np.uint8), h.P)
    sizes = _flat_sizes(sizes, h.n_sizes, "segment")
    _check_sizes(sizes, "segment", 2, h.segment + 2, h.n_words)
    payload = _checked_payload(payload, h.n_words)
    head = _MAP_FIXED.pack(MAPPED_MAGIC, MAPPED_VERSION, h.N, len(h.shape), h.P, h.C, h.segment, h.n_words)
    return b"".join([head, np.asarray(h.lambs, dtype="<f8").tobytes(), b"".join(h.digests), np.asarray(h.shape, dtype="<u8").tobytes(),
                     pack_classes(classes), sizes.astype("<u2").tobytes(), payload.tobytes()])


def mapped_nbytes(shape, C, segment, n_words, P) -> int:
    """len(write_mapped(...)) of a latent tensor of `shape` (channel-last, C channels) with a palette of P lambdas, in segments
    of `segment` symbols and a payload of n_words 16-bit words, without building the file.  ValueError for fields
    `write_mapped` rejects."""
    P = int(P)
    if not 1 <= P <= MAX_CLASSES:
        raise ValueError(f"P = {P} classes outside [1, {MAX_CLASSES}]")
    return _mapped_header(MappedHeader(N=MAX_N, C=C, shape=shape, segment=segment, lambs=tuple(float(p) for p in range(P)),
                                       digests=(bytes(16),) * P, n_words=n_words)).total_nbytes


# ---- batches of lambda-map files, written (ChannelwisePriorCDFQuantizer.compress_latents_to_bytes_mapped_batch; include/vbq.h,
# "Mapped batch encode").  encode_plan with a palette where it has a table: the files of a palette are solved together at the
# palette's P lambdas, and a block of items shares the palette's tables.
MAPPED_ENCODE_FIELDS = 8                     # idx_base, idx_stride, plane_stride, n, seg_base, palette, cls_base, 0
CLASS_ALIGN = 8                              # a file's class bytes start at a multiple of 8 bytes: one 8-byte load is 8 classes
MappedEncodePlan = namedtuple("MappedEncodePlan", "nseg seg_base M row0 group_rows group_row_base n_rows group_idx_base n_idx "
                                                  "cls_base n_cls files palettes items")


def mapped_encode_plan(rows, palettes, palette_sizes, segment, C) -> MappedEncodePlan:
    """What vbq_rans_map_encode_files_u16 / vbq_rans_map_sizes_files_u16 read, from the rows per channel n_f >= 1 of F files,
    their palette numbers (0 .. G - 1), the number of classes P_g (1..MAX_CLASSES) of each of the G palettes, the segment
    length and the number of channels C:

        nseg, seg_base, M   exactly encode_plan's: ceil(n_f / segment), the file-major exclusive sum of C * nseg_f, its total
        row0, group_rows, group_row_base, n_rows   the row layout of encode_plan with the palette in the place of the table: the
                                          files of a palette sit next to each other, in file order, in that palette's group of
                                          B_g rows, every file's run starting at a multiple of ENCODE_ROW_ALIGN (the latents
                                          of all groups are one array of n_rows rows)
        group_idx_base, n_idx  int64 [G], int  group g owns [P_g, C, B_g] index planes of the one index array, starting at
                                          element group_idx_base_g = the sum of P_h * C * B_h over the groups h before it;
                                          n_idx their total
        cls_base, n_cls     int64 [F], int  the file-major exclusive sum of the files' positions n_f, each rounded up to
                                          CLASS_ALIGN bytes, and its total: file f's class bytes are cls[cls_base_f : + n_f]
        files               int64 [F, 8]  the descriptors: idx_base = group_idx_base_g + row0_f, idx_stride = B_g, plane_stride
                                          = C * B_g, n_f, seg_base_f, palette, cls_base_f, 0
        palettes            int32 [G, 4]  a template of the kernel's palette rows: 0 for a class below P_g, -1 past it -- the
                                          caller writes its table numbers over the zeros
        items               int32 [n_items, 2]  exactly encode_plan's, palette by palette: every block of ENCODE_BLOCK items
                                          holds one palette only, padded with (-1, -1)

    ValueError for a bad segment, C < 1, a row count < 1, a palette outside [0, G), a palette size outside [1, MAX_CLASSES] or
    more than MAX_BATCH_FILES files."""
    P = np.asarray(palette_sizes, dtype=np.int64).reshape(-1)
    G = P.size
    if G and (int(P.min()) < 1 or int(P.max()) > MAX_CLASSES):
        raise ValueError(f"palette sizes {P.tolist()} outside [1, {MAX_CLASSES}]")
    base = encode_plan(rows, palettes, segment, C, G)
    C, n, pal, F, _ = _plan_inputs(rows, palettes, C, G)
    per_group = P * C * base.group_rows
    group_idx_base = np.cumsum(per_group) - per_group
    padded = (n + CLASS_ALIGN - 1) // CLASS_ALIGN * CLASS_ALIGN
    cls_base = np.cumsum(padded) - padded
    files = np.stack([group_idx_base[pal] + base.row0, base.group_rows[pal], C * base.group_rows[pal], n, base.seg_base, pal,
                      cls_base, np.zeros(F, np.int64)], axis=1) if F else np.zeros((0, MAPPED_ENCODE_FIELDS), np.int64)
    rows4 = np.where(np.arange(MAX_CLASSES)[None, :] < P[:, None], 0, -1).astype(np.int32)
    return MappedEncodePlan(base.nseg, base.seg_base, base.M, base.row0, base.group_rows, base.group_row_base, base.n_rows,
                            group_idx_base, int(per_group.sum()), cls_base, int(padded.sum()),
                            np.ascontiguousarray(files, dtype=np.int64), np.ascontiguousarray(rows4), base.items)


# ---- byte budgets over lambda maps (ChannelwisePriorCDFQuantizer.coded_nbytes_mapped_palettes_batch and the budget calls over
# it; include/vbq.h, "Mapped batch rates").  A budget call takes an ordered list of candidate palettes of one size P and keeps,
# per file, the FIRST candidate of the list whose file fits (smallest_rates_within(..., name="palette")): palettes have no natural
# order, so the order is the caller's.
def palette_ladder(lambs, steps):
    """The usual list of candidates: the relative quality between the classes held fixed while the whole palette slides up a
    ladder of lambdas.  lambs: the ladder, sorted ascending; steps: P (1..MAX_CLASSES) distinct non-negative integers, the rung
    of every class above the candidate's first.  Candidate j is tuple(lambs[j + s] for s in steps), for j = 0 .. len(lambs) - 1
    - max(steps).  ValueError for an empty result, repeated or negative steps, a ladder that is not ascending or P outside
    1..MAX_CLASSES."""
    lambs = [float(l) for l in lambs]
    for s in steps:
        if isinstance(s, (bool, np.bool_)) or not isinstance(s, (int, np.integer)):
            raise ValueError(f"steps must be integers, got {s!r}")
    steps = [int(s) for s in steps]
    if not 1 <= len(steps) <= MAX_CLASSES:
        raise ValueError(f"{len(steps)} steps: a palette has 1..{MAX_CLASSES} lambdas")
    if min(steps) < 0:
        raise ValueError(f"negative step in {steps}")
    if len(set(steps)) != len(steps):
        raise ValueError(f"repeated step in {steps}: the lambdas of a palette are distinct")
    if any(b <= a for a, b in zip(lambs, lambs[1:])):
        raise ValueError("the ladder of lambdas must be sorted ascending, without repeats")
    count = len(lambs) - max(steps)
    if count < 1:
        raise ValueError(f"a ladder of {len(lambs)} lambdas has no candidate with steps {steps}")
    return [tuple(lambs[j + s] for s in steps) for j in range(count)]


def candidate_chunks(rows, max_tables):
    """Cut a list of candidates into runs that can be sized from one solve.  rows: int [K, P], the candidates as indices into
    the L distinct lambdas; max_tables: how many lambdas one solve may hold.  Yields (k0, k1, tables): greedy runs [k0, k1) of
    consecutive candidates whose distinct lambdas -- tables, a sorted list -- number at most max_tables.  A chunk always holds
    at least one candidate, so a single candidate may bring up to P tables whatever the cap.  Every candidate is yielded once,
    in order."""
    rows = np.asarray(rows, dtype=np.int64)
    if rows.ndim != 2:
        raise ValueError(f"rows must be [K, P], got shape {rows.shape}")
    max_tables = int(max_tables)
    K = rows.shape[0]
    k0 = 0
    while k0 < K:
        tables = set(rows[k0].tolist())
        k1 = k0 + 1
        while k1 < K and len(tables | set(rows[k1].tolist())) <= max_tables:
            tables |= set(rows[k1].tolist())
            k1 += 1
        yield k0, k1, sorted(tables)
        k0 = k1


def parse_mapped(data) -> Tuple[MappedHeader, np.ndarray, np.ndarray, int]:
    """bytes -> (header, classes u8 [B], sizes u16 [C * nseg] (a read-only view into `data`), byte offset of the payload).
    ValueError on anything malformed."""
    mv = memoryview(data).cast("B")
    magic, version, N, ndim, P, C, segment, n_words = _unpack_fixed(mv, _MAP_FIXED)
    if magic != MAPPED_MAGIC:
        raise ValueError(_MAP_FOREIGN.get(magic) or f"not a VBQ lambda-map bitstream (magic {magic!r})")
    if version != MAPPED_VERSION:
        raise ValueError(f"unknown lambda-map bitstream version {version}")
    if not 1 <= P <= MAX_CLASSES:
        raise ValueError(f"P = {P} classes outside [1, {MAX_CLASSES}]")
    if ndim < 1:
        raise ValueError("latent shape with 0 dimensions")
    hlen = _MAP_FIXED.size + 24 * P + 8 * ndim
    if len(mv) < hlen:
        raise ValueError(f"truncated in the palette or the latent shape: {len(mv)} bytes, the header is {hlen}")
    lambs = tuple(float(l) for l in np.frombuffer(mv, dtype="<f8", count=P, offset=_MAP_FIXED.size))
    d0 = _MAP_FIXED.size + 8 * P
    digests = tuple(bytes(mv[d0 + 16 * p: d0 + 16 * p + 16]) for p in range(P))
    shape = tuple(int(d) for d in np.frombuffer(mv, dtype="<u8", count=ndim, offset=d0 + 16 * P))
    h = MappedHeader(N=N, C=C, shape=shape, segment=segment, lambs=lambs, digests=digests, n_words=n_words)
    h.check()
    _check_length(len(mv), h.total_nbytes, f"header, {h.n_rows} classes, {h.n_sizes} segment sizes and {n_words} payload words")
    B = h.n_rows
    block = np.frombuffer(mv, dtype=np.uint8, count=h.classes_nbytes, offset=h.nbytes)
    quads = (block[:, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3          # every 2-bit field, padding included
    if quads.reshape(-1)[B:].any():
        raise ValueError("padding bits after the classes are not zero")
    classes = quads.reshape(-1)[:B]
    _check_classes(classes, P)
    sizes = np.frombuffer(mv, dtype="<u2", count=h.n_sizes, offset=h.sizes_offset)
    _check_sizes(sizes, "segment", 2, segment + 2, n_words)
    return h, classes, sizes, h.sizes_offset + h.sizes_nbytes


# ---------------------------------------------------------------------------------------------------------------------------
# Second format: ONE compressed word-embedding matrix at ONE beta (vbq_amd.embeddings.compress_to_bytes / CompressedEmbeddings).
#
# One rANS stream holds every coordinate in row-major order (rows = slices along axis 0), cut into segments of `segment`
# symbols; by default a segment is a whole number of rows, so that looking up a row decodes only the segment that holds it.
# The frequency table is fitted to the matrix itself (coder.exact_frequencies: unused symbols get 0), so the file stores
# only the K symbols with a nonzero frequency.  Layout, every field little-endian (version 1):
#
#     offset  size      field
#     0       4         magic b"VBQe"
#     4       1         version = 1
#     5       1         N = max_bits_per_coord (1..10)
#     6       2         reserved = 0
#     8       4         segment, symbols per rANS segment (u32, 1..65533)
#     12      4         K, symbols with a nonzero frequency (u32, 2..T)
#     16      8         beta (f64, finite, >= 0)
#     24      8         n_words, payload length in 16-bit words (u64)
#     32      4         empirical_std (f32, informational: the scale of the code book)
#     36      4         ndim of the matrix shape (u32, 1..64)
#     40      8 * ndim  shape (u64 each, every entry >= 1)
#     ...     8 * K     the sparse table, one 8-byte record per symbol: rank (u16, strictly increasing, < T), frequency
#                       (u16, 1..2^15 - 1, summing to 2^15), value (f32, finite, non-decreasing with rank)
#     ...     2 * nseg  segment sizes (u16, each in [2, segment + 2]), nseg = ceil(prod(shape) / segment)
#     ...     2*n_words payload (u16): the valid words of every segment in order; sum(sizes) == n_words
#
# Every part before the sizes is a multiple of 8 bytes long.  `parse_embeddings` raises ValueError with a specific message
# on anything malformed, never struct.error or IndexError.
# ---------------------------------------------------------------------------------------------------------------------------
EMB_MAGIC = b"VBQe"
EMB_VERSION = 1
MAX_NDIM = 64
_EMB_FIXED = struct.Struct("<4sBBHIIdQfI")   # the 40 bytes before the shape
assert _EMB_FIXED.size == 40
TABLE_DTYPE = np.dtype([("rank", "<u2"), ("freq", "<u2"), ("value", "<f4")])
assert TABLE_DTYPE.itemsize == 8
PROB_ONE = 1 << 15                           # the coder's probability scale (coder.PROB_BITS)


@dataclass(frozen=True)
class EmbeddingHeader:
    N: int
    shape: Tuple[int, ...]
    segment: int
    beta: float
    empirical_std: float
    n_words: int
    K: int

    @property
    def n(self) -> int:
        """Coordinates in the matrix: the length of the one stream."""
        return math.prod(self.shape)

    @property
    def row_length(self) -> int:
        return math.prod(self.shape[1:])

    @property
    def nseg(self) -> int:
        return (self.n + self.segment - 1) // self.segment

    @property
    def nbytes(self) -> int:
        """Length of the header and the sparse table (where the sizes start)."""
        return _EMB_FIXED.size + 8 * len(self.shape) + TABLE_DTYPE.itemsize * self.K


def _check_emb_fields(N, shape, segment, beta, n_words, K):
    if not 1 <= N <= MAX_N:
        raise ValueError(f"N = {N} outside [1, {MAX_N}]")
    if not 1 <= len(shape) <= MAX_NDIM:
        raise ValueError(f"matrix shape with {len(shape)} dimensions")
    if any(d < 1 for d in shape):
        raise ValueError(f"empty matrix shape {tuple(shape)}")
    if math.prod(shape) >= 2 ** 62:
        raise ValueError(f"matrix shape {tuple(shape)} is too large")
    check_segment(segment)
    if not (math.isfinite(beta) and beta >= 0):
        raise ValueError(f"beta {beta} is not finite and >= 0")
    if n_words < 0:
        raise ValueError("negative payload length")
    T = 2 ** (N + 1) - 1
    if not 2 <= K <= T:
        raise ValueError(f"K = {K} symbols outside [2, {T}]")


def _check_table(table: np.ndarray, N: int):
    T = 2 ** (N + 1) - 1
    r = table["rank"].astype(np.int64)
    f = table["freq"].astype(np.int64)
    v = table["value"]
    if np.any(np.diff(r) <= 0):
        raise ValueError("table ranks are not strictly increasing")
    if r.size and int(r[-1]) >= T:
        raise ValueError(f"table rank {int(r[-1])} >= T = {T}")
    if np.any(f == 0):
        raise ValueError("table frequency 0 (only symbols with a nonzero frequency are stored)")
    if np.any(f >= PROB_ONE):
        raise ValueError(f"table frequency above {PROB_ONE - 1}")
    if int(f.sum()) != PROB_ONE:
        raise ValueError(f"table frequencies sum to {int(f.sum())}, not {PROB_ONE}")
    if not np.all(np.isfinite(v)):
        raise ValueError("non-finite table value")
    if np.any(np.diff(v) < 0):
        raise ValueError("table values decrease with rank")


def write_embeddings(header: EmbeddingHeader, table, sizes, payload) -> bytes:
    """header + table (TABLE_DTYPE [K]) + sizes (any integer array of nseg entries) + payload (u16 [n_words]) -> bytes.
    Validates as `parse_embeddings` does."""
    h = header
    shape = tuple(int(d) for d in h.shape)
    _check_emb_fields(h.N, shape, h.segment, float(h.beta), h.n_words, h.K)
    table = np.asarray(table)
    if table.dtype != TABLE_DTYPE or table.shape != (h.K,):
        raise ValueError(f"table must be {TABLE_DTYPE} [{h.K}], got {table.dtype} {table.shape}")
    _check_table(table, h.N)
    sizes = _flat_sizes(sizes, h.nseg, "segment")
    _check_sizes(sizes, "segment", 2, h.segment + 2, h.n_words)
    payload = _checked_payload(payload, h.n_words)
    head = _EMB_FIXED.pack(EMB_MAGIC, EMB_VERSION, h.N, 0, h.segment, h.K, float(h.beta), h.n_words,
                           float(h.empirical_std), len(shape))
    return b"".join([head, np.asarray(shape, dtype="<u8").tobytes(), np.ascontiguousarray(table).tobytes(),
                     sizes.astype("<u2").tobytes(), payload.tobytes()])


def embeddings_nbytes(shape, segment, K, n_words) -> int:
    """len(write_embeddings(...)) of a matrix of `shape` in segments of `segment` symbols, with K symbols in the table and a
    payload of n_words 16-bit words, without building the file.  ValueError for fields `write_embeddings` rejects."""
    shape = tuple(int(d) for d in shape)
    h = EmbeddingHeader(N=MAX_N, shape=shape, segment=int(segment), beta=0.0, empirical_std=0.0, n_words=int(n_words), K=int(K))
    _check_emb_fields(h.N, shape, h.segment, h.beta, h.n_words, h.K)
    return h.nbytes + 2 * h.nseg + 2 * h.n_words


# ---------------------------------------------------------------------------------------------------------------------------
# Rate control: the file of a byte budget.  One model serves every rate; a caller measures the exact length at each candidate
# rate (lambda or beta) and keeps the numerically SMALLEST candidate whose file fits.  The rule does not assume the length falls
# as the rate grows -- it usually does, not always -- so it is well defined on any set of candidates.
# ---------------------------------------------------------------------------------------------------------------------------
def check_budget(max_bytes) -> int:
    """max_bytes as an int: an integer >= 1 (bool and floats are rejected, TypeError; values below 1, ValueError)."""
    if isinstance(max_bytes, (bool, np.bool_)) or not isinstance(max_bytes, (int, np.integer)):
        raise TypeError(f"max_bytes must be an integer, got {type(max_bytes).__name__}")
    if max_bytes < 1:
        raise ValueError(f"max_bytes = {max_bytes}: a budget needs at least one byte")
    return int(max_bytes)


def smallest_rate_within(nbytes, max_bytes, name: str = "lambda"):
    """The numerically smallest key of `nbytes` (a mapping rate -> exact file length) whose length is <= max_bytes.  ValueError
    naming the smallest achievable length and its rate when none fits."""
    budget = check_budget(max_bytes)
    items = [(float(r), int(b), r) for r, b in nbytes.items()]
    if not items:
        raise ValueError(f"no candidate {name} to choose from")
    fits = [it for it in items if it[1] <= budget]
    if fits:
        return min(fits, key=lambda it: it[0])[2]
    _, least, rate = min(items, key=lambda it: (it[1], it[0]))
    raise ValueError(f"no {name} fits in {budget} bytes: the smallest file is {least} bytes, at {name} = {float(rate)!r}")


def check_budgets(budgets):
    """None for one budget for all files (an integer, checked), else the budgets of a sequence as a list, each checked by
    check_budget."""
    if np.ndim(budgets) == 0:
        check_budget(budgets)
        return None
    return [check_budget(b) for b in budgets]


def smallest_rates_within(nbytes, budgets, rates=None, name: str = "lambda") -> np.ndarray:
    """smallest_rate_within for F files at once.  nbytes: exact file lengths int64 [F, L], the columns in ascending order of
    the rate; budgets: one int for all files or a sequence of F (each checked by check_budget).  Returns int64 [F]: for every
    file the FIRST column -- the numerically smallest rate -- whose length is <= the file's budget; no monotonicity along a
    row is assumed.  ValueError naming the first file without a fit, its smallest length and that length's rate (rates[column]
    where `rates` is given, else the column index)."""
    nbytes = np.asarray(nbytes)
    if nbytes.ndim != 2 or nbytes.dtype.kind not in "iu":
        raise ValueError(f"nbytes must be an integer array [F, L], got {nbytes.dtype} {nbytes.shape}")
    nbytes = nbytes.astype(np.int64, copy=False)
    F, L = nbytes.shape
    each = check_budgets(budgets)
    budgets = [int(budgets)] * F if each is None else each
    if len(budgets) != F:
        raise ValueError(f"{len(budgets)} budgets for {F} files")
    if F == 0:
        return np.zeros(0, np.int64)
    if L == 0:
        raise ValueError(f"no candidate {name} to choose from")
    if rates is not None and len(rates) != L:
        raise ValueError(f"{len(rates)} rates for {L} columns")
    fits = nbytes <= np.array([min(b, np.iinfo(np.int64).max) for b in budgets], np.int64)[:, None]
    for f in np.flatnonzero(~fits.any(axis=1)):
        col = int(np.argmin(nbytes[f]))                           # the first of equal lengths: the smaller rate
        rate = repr(float(rates[col])) if rates is not None else f"column {col}"
        raise ValueError(f"file {int(f)}: no {name} fits in {budgets[f]} bytes: the smallest file is {int(nbytes[f, col])} bytes, "
                         f"at {name} = {rate}")
    return np.argmax(fits, axis=1).astype(np.int64)


def parse_embeddings(data) -> Tuple[EmbeddingHeader, np.ndarray, np.ndarray, int]:
    """bytes -> (header, table TABLE_DTYPE [K], sizes u16 [nseg], byte offset of the payload); the table and the sizes are
    read-only views into `data`.  ValueError on anything malformed."""
    mv = memoryview(data).cast("B")
    magic, version, N, reserved, segment, K, beta, n_words, std, ndim = _unpack_fixed(mv, _EMB_FIXED)
    if magic == MAGIC:
        raise ValueError("a latent bitstream (magic b'VBQb'), not a compressed embedding matrix")
    if magic != EMB_MAGIC:
        raise ValueError(f"not a VBQ embedding bitstream (magic {magic!r})")
    if version != EMB_VERSION:
        raise ValueError(f"unknown embedding bitstream version {version}")
    if reserved != 0:
        raise ValueError(f"reserved header bytes are {reserved}, not 0")
    if not 1 <= ndim <= MAX_NDIM:
        raise ValueError(f"matrix shape with {ndim} dimensions")
    shape = _read_shape(mv, _EMB_FIXED, ndim, "matrix")
    _check_emb_fields(N, shape, segment, beta, n_words, K)
    h = EmbeddingHeader(N=N, shape=shape, segment=segment, beta=float(beta), empirical_std=float(std), n_words=n_words, K=K)
    if len(mv) < h.nbytes:
        raise ValueError(f"truncated in the symbol table: {len(mv)} bytes, header and table need {h.nbytes}")
    table = np.frombuffer(mv, dtype=TABLE_DTYPE, count=K, offset=_EMB_FIXED.size + 8 * ndim)
    _check_table(table, N)
    _check_length(len(mv), h.nbytes + 2 * h.nseg + 2 * n_words,
                  f"header, table, {h.nseg} segment sizes and {n_words} payload words")
    sizes = np.frombuffer(mv, dtype="<u2", count=h.nseg, offset=h.nbytes)
    _check_sizes(sizes, "segment", 2, segment + 2, n_words)
    return h, table, sizes, h.nbytes + 2 * h.nseg


# ---------------------------------------------------------------------------------------------------------------------------
# Fourth format: ONE matrix whose rows were quantized to ONE exact bit budget (vbq_amd.quantize_rows_to_budget), stored as
# fixed-size records (vbq_amd.embeddings.compress_to_records / RecordEmbeddings).  Every row costs the same number of words, so
# row r sits at word r * record_words and decodes without an entropy coder; the price is the lengths stored at fixed width.
#
# One record.  A code point of bit length n has rank index q; with k = q + 1: n = N - ctz(k), its code is
# j = k >> (N - n + 1), an n-bit number, and q = ((2 j + 1) << (N - n)) - 1 (vbq_amd/tables.py).  W = N.bit_length().  Bit i of
# a record is bit i % 32 of little-endian u32 word i / 32.
#     length block  coordinate k's length n_k in bits [k W, (k+1) W), least significant bit first
#     code block    from bit K W: j_k takes n_k bits at K W + sum_{i<k} n_i, least significant bit first
#     padding       zero bits up to record_words = ceil((K W + total_bits) / 32) words
#
# Layout of the file, every field little-endian (version 1):
#
#     offset  size      field
#     0       4         magic b"VBQr"
#     4       1         version = 1
#     5       1         N (1..10)
#     6       1         ndim (>= 1)
#     7       1         reserved = 0
#     8       4         C: 1 (one code book) or K (one per column)
#     12      4         total_bits (0 .. K * N)
#     16      4         record_words (must equal the formula above; at most 8192: a record fits in LDS)
#     20      4         reserved = 0
#     24      8 * ndim  shape (u64 each, every entry >= 1); rows are the slices along axis 0, K = prod(shape[1:])
#     ...     4 * C*T   code points, f32 [C, T] in rank order, T = 2^(N+1) - 1, every value finite; then 4 zero bytes when
#                       C * T is odd, so that the records start 8-byte aligned
#     ...     4 * R * record_words   the records (u32 words) of rows 0 .. R - 1; nothing follows them
#
# `parse_records` raises ValueError with a specific message on anything malformed, never struct.error or IndexError.  What a
# record holds is checked on the device (vbq_records_unpack_f32), once, when RecordEmbeddings loads the file.
# ---------------------------------------------------------------------------------------------------------------------------
RECORDS_MAGIC = b"VBQr"
RECORDS_VERSION = 1
MAX_RECORD_WORDS = 8192                      # the kernels' limit (vbq_records_pack_u16): the LDS image of one record
_REC_FIXED = struct.Struct("<4sBBBBIIII")    # the 24 bytes before the shape
assert _REC_FIXED.size == 24
_REC_FOREIGN = {MAGIC: "a latent bitstream in segments (magic b'VBQb'), not a record file",
                COMPACT_MAGIC: "a compact latent bitstream (magic b'VBQc'), not a record file",
                EMB_MAGIC: "a compressed embedding matrix (magic b'VBQe'), not a record file"}


@dataclass(frozen=True)
class RecordsHeader:
    N: int
    shape: Tuple[int, ...]
    C: int
    total_bits: int

    @property
    def n(self) -> int:
        """Coordinates in the matrix."""
        return math.prod(self.shape)

    @property
    def n_rows(self) -> int:
        return self.shape[0]

    @property
    def row_length(self) -> int:
        """K: the coordinates of one row."""
        return math.prod(self.shape[1:])

    @property
    def length_bits(self) -> int:
        """W: the width of a length field."""
        return self.N.bit_length()

    @property
    def record_words(self) -> int:
        return (self.row_length * self.length_bits + self.total_bits + 31) // 32

    @property
    def T(self) -> int:
        return 2 ** (self.N + 1) - 1

    @property
    def nbytes(self) -> int:
        """Length of the header itself (where the code points start)."""
        return _REC_FIXED.size + 8 * len(self.shape)

    @property
    def table_nbytes(self) -> int:
        """Length of the code-point block, padding included."""
        return 4 * self.C * self.T + 4 * (self.C * self.T & 1)

    @property
    def records_offset(self) -> int:
        return self.nbytes + self.table_nbytes

    @property
    def total_nbytes(self) -> int:
        return self.records_offset + 4 * self.n_rows * self.record_words

    def check(self):
        N, shape = self.N, tuple(self.shape)
        if not 1 <= N <= MAX_N:
            raise ValueError(f"N = {N} outside [1, {MAX_N}]")
        if not 1 <= len(shape) <= 255:
            raise ValueError(f"matrix shape with {len(shape)} dimensions")
        if any(d < 1 for d in shape):
            raise ValueError(f"empty matrix shape {shape}")
        if math.prod(shape) >= 2 ** 62:
            raise ValueError(f"matrix shape {shape} is too large")
        K = self.row_length
        if self.C not in (1, K):
            raise ValueError(f"C = {self.C} is neither 1 (one code book) nor K = {K} (one per column)")
        if not 0 <= self.total_bits <= K * N:
            raise ValueError(f"total_bits {self.total_bits} outside [0, K*N = {K * N}]")
        if self.record_words > MAX_RECORD_WORDS:
            raise ValueError(f"a record of {self.record_words} words exceeds the limit of {MAX_RECORD_WORDS}")


def _records_header(shape, N, total_bits, C) -> RecordsHeader:
    h = RecordsHeader(N=int(N), shape=tuple(int(d) for d in shape), C=int(C), total_bits=int(total_bits))
    h.check()
    return h


def _check_codepoints(table: np.ndarray):
    if not np.all(np.isfinite(table)):
        raise ValueError("non-finite code point in the table")


def write_records(header: RecordsHeader, table, words) -> bytes:
    """header + table (f32 [C, T], rank order) + words (u32, R * record_words of them: the records of vbq_records_pack_u16)
    -> bytes.  Validates as `parse_records` does."""
    h = _records_header(header.shape, header.N, header.total_bits, header.C)
    table = np.ascontiguousarray(table, dtype="<f4")
    if table.size != h.C * h.T:
        raise ValueError(f"table of {table.size} code points, C * T = {h.C} * {h.T} needed")
    _check_codepoints(table)
    words = np.ascontiguousarray(words, dtype="<u4").reshape(-1)
    if words.size != h.n_rows * h.record_words:
        raise ValueError(f"{words.size} record words, {h.n_rows} rows of {h.record_words} words needed")
    head = _REC_FIXED.pack(RECORDS_MAGIC, RECORDS_VERSION, h.N, len(h.shape), 0, h.C, h.total_bits, h.record_words, 0)
    return b"".join([head, np.asarray(h.shape, dtype="<u8").tobytes(), table.tobytes(), bytes(h.table_nbytes - table.nbytes),
                     words.tobytes()])


def records_nbytes(shape, N, total_bits, C) -> int:
    """len(write_records(...)) of a matrix of `shape` at N, total_bits and C code books, without building the file.  ValueError
    for fields `write_records` rejects."""
    return _records_header(shape, N, total_bits, C).total_nbytes


def records_total_bits_within(shape, N, C, max_bytes) -> int:
    """The largest total_bits whose record file of a matrix of `shape` is <= max_bytes long (an integer >= 1).  The length is a
    closed form -- header, code points, R records of ceil((K W + total_bits) / 32) words -- so nothing is searched.  ValueError
    naming the smallest possible file when even total_bits = 0 does not fit."""
    budget = check_budget(max_bytes)
    h = _records_header(shape, N, 0, C)
    K, KW = h.row_length, h.row_length * h.length_bits
    words = min((budget - h.records_offset) // (4 * h.n_rows), MAX_RECORD_WORDS)      # per record
    if 32 * words < KW:
        raise ValueError(f"no total_bits fits in {budget} bytes: the smallest file (total_bits = 0) is {h.total_nbytes} bytes")
    return min(K * h.N, 32 * words - KW)


def parse_records(data) -> Tuple[RecordsHeader, np.ndarray, int]:
    """bytes -> (header, code points f32 [C, T] (a read-only view into `data`), byte offset of the records).  ValueError on
    anything malformed."""
    mv = memoryview(data).cast("B")
    magic, version, N, ndim, reserved, C, total_bits, record_words, reserved2 = _unpack_fixed(mv, _REC_FIXED)
    if magic != RECORDS_MAGIC:
        raise ValueError(_REC_FOREIGN.get(magic) or f"not a VBQ record file (magic {magic!r})")
    if version != RECORDS_VERSION:
        raise ValueError(f"unknown record file version {version}")
    if reserved != 0:
        raise ValueError(f"reserved header byte is {reserved}, not 0")
    if reserved2 != 0:
        raise ValueError(f"reserved header word is {reserved2}, not 0")
    shape = _read_shape(mv, _REC_FIXED, ndim, "matrix")
    h = RecordsHeader(N=N, shape=shape, C=C, total_bits=total_bits)
    h.check()
    if record_words != h.record_words:
        raise ValueError(f"record_words is {record_words}, K*W + total_bits = {h.row_length * h.length_bits + total_bits} "
                         f"bits need {h.record_words}")
    if len(mv) < h.records_offset:
        raise ValueError(f"truncated in the code-point table: {len(mv)} bytes, header and table need {h.records_offset}")
    table = np.frombuffer(mv, dtype="<f4", count=C * h.T, offset=h.nbytes).reshape(C, h.T)
    _check_codepoints(table)
    if any(mv[h.nbytes + table.nbytes: h.records_offset]):
        raise ValueError("padding after the code-point table is not zero")
    _check_length(len(mv), h.total_nbytes, f"header, table and {h.n_rows} records of {h.record_words} words")
    return h, table, h.records_offset
