"""Self-describing byte format for ONE latent tensor coded at ONE lambda (a compressed file).

Host-only: writing and strictly validating the header.  The payload is what `RansCodec.pack` returns for the coder's
streams (one per channel, each holding the B = prod(shape) / C latents of that channel, cut into segments of `segment`
symbols); the device builds it with vbq_rans_pack_u16 and takes it apart with vbq_rans_unpack_u16 (include/vbq.h).
ChannelwisePriorCDFQuantizer.compress_latents_to_bytes / decompress_latents are the users.

Layout, every field little-endian (version 1):

    offset  size      field
    0       4         magic b"VBQb"
    4       1         version = 1
    5       1         N = max_bits_per_coord (1..10)
    6       1         ndim of the latent shape (>= 1)
    7       1         reserved = 0
    8       4         C, the number of channels (u32)
    12      4         segment, symbols per rANS segment (u32, 1..65533)
    16      8         lambda (f64, finite)
    24      8         n_words, payload length in 16-bit words (u64)
    32      16        digest: blake2b-128 of the sorted code-point table (f32 [C, T]) and the quantised frequency
                      table (u16 [C, T]) of this lambda -- exactly what decoding depends on
    48      8 * ndim  latent shape (u64 each, channel last: shape[-1] == C, every entry >= 1)
    48+8nd  2 * C*nseg segment sizes (u16, each in [2, segment + 2]), nseg = ceil(prod(shape) / C / segment),
                      stream-major (channel), then segment
    ...     2*n_words payload (u16): the valid words of every segment in the same order; sum(sizes) == n_words

The header is a multiple of 8 bytes long, so the sizes and the payload can be viewed as u16 in place.  `parse` raises
ValueError with a specific message on anything malformed -- never struct.error or IndexError -- and checks every size
with vectorised NumPy before anything reaches the device (the unpack kernel's own checks are the second line of defence).
"""
from __future__ import annotations

import hashlib
import math
import struct
from dataclasses import dataclass
from typing import Tuple

import numpy as np

MAGIC = b"VBQb"
VERSION = 1
MAX_N = 10                                   # the coder's limit (vbq_rans_encode_u16)
MAX_SEGMENT = 65533                          # seg + 2 must fit in a u16 size
_FIXED = struct.Struct("<4sBBBBIIdQ16s")     # the 48 bytes before the shape
assert _FIXED.size == 48


@dataclass(frozen=True)
class Header:
    N: int
    C: int
    shape: Tuple[int, ...]
    lamb: float
    segment: int
    digest: bytes
    n_words: int

    @property
    def n_rows(self) -> int:
        """Symbols per stream: the latents of one channel."""
        return math.prod(self.shape) // self.C

    @property
    def nseg(self) -> int:
        return (self.n_rows + self.segment - 1) // self.segment

    @property
    def n_sizes(self) -> int:
        return self.C * self.nseg

    @property
    def nbytes(self) -> int:
        """Length of the header itself (where the sizes start)."""
        return _FIXED.size + 8 * len(self.shape)


def digest(sorted_table, freq) -> bytes:
    """blake2b-128 over the sorted code points (f32 [C, T]) and the quantised frequencies (u16 [C, T]) of one lambda."""
    h = hashlib.blake2b(digest_size=16)
    h.update(np.ascontiguousarray(sorted_table, dtype="<f4").tobytes())
    h.update(np.ascontiguousarray(freq, dtype="<u2").tobytes())
    return h.digest()


def _check_fields(N, C, shape, lamb, segment, dig, n_words):
    if not 1 <= N <= MAX_N:
        raise ValueError(f"N = {N} outside [1, {MAX_N}]")
    if C < 1:
        raise ValueError("zero channels")
    if not 1 <= len(shape) <= 255:
        raise ValueError(f"latent shape with {len(shape)} dimensions")
    if any(d < 1 for d in shape):
        raise ValueError(f"empty latent shape {tuple(shape)}")
    if shape[-1] != C:
        raise ValueError(f"latent shape {tuple(shape)} is not channel-last for C = {C}")
    if math.prod(shape) % C:
        raise ValueError(f"latent shape {tuple(shape)}: {math.prod(shape)} elements are not a multiple of C = {C}")
    if math.prod(shape) >= 2 ** 62:
        raise ValueError(f"latent shape {tuple(shape)} is too large")
    if not math.isfinite(lamb):
        raise ValueError(f"non-finite lambda {lamb}")
    if not 1 <= segment <= MAX_SEGMENT:
        raise ValueError(f"segment {segment} outside [1, {MAX_SEGMENT}]")
    if len(dig) != 16:
        raise ValueError("digest must be 16 bytes")
    if n_words < 0:
        raise ValueError("negative payload length")


def _check_sizes(sizes: np.ndarray, segment: int, n_words: int):
    if sizes.size and (int(sizes.min()) < 2 or int(sizes.max()) > segment + 2):
        bad = int(np.flatnonzero((sizes < 2) | (sizes > segment + 2))[0])
        raise ValueError(f"segment size {int(sizes[bad])} at position {bad} outside [2, {segment + 2}]")
    total = int(sizes.sum(dtype=np.int64))
    if total != n_words:
        raise ValueError(f"segment sizes add up to {total} words, the header says {n_words}")


def write(header: Header, sizes, payload) -> bytes:
    """header + sizes (any integer array of C * nseg entries) + payload (u16 [n_words]) -> bytes.  Validates as `parse` does."""
    h = header
    shape = tuple(int(d) for d in h.shape)
    _check_fields(h.N, h.C, shape, float(h.lamb), h.segment, h.digest, h.n_words)
    sizes = np.asarray(sizes).reshape(-1)
    if sizes.size != h.n_sizes:
        raise ValueError(f"{sizes.size} segment sizes, the shape needs {h.n_sizes}")
    _check_sizes(sizes, h.segment, h.n_words)
    payload = np.ascontiguousarray(payload, dtype="<u2").reshape(-1)
    if payload.size != h.n_words:
        raise ValueError(f"payload of {payload.size} words, the header says {h.n_words}")
    head = _FIXED.pack(MAGIC, VERSION, h.N, len(shape), 0, h.C, h.segment, float(h.lamb), h.n_words, h.digest)
    return b"".join([head, np.asarray(shape, dtype="<u8").tobytes(), sizes.astype("<u2").tobytes(), payload.tobytes()])


def parse(data) -> Tuple[Header, np.ndarray, int]:
    """bytes -> (header, sizes u16 [C * nseg] (a read-only view into `data`), byte offset of the payload).
    ValueError on anything malformed."""
    mv = memoryview(data).cast("B")
    if len(mv) < _FIXED.size:
        raise ValueError(f"truncated: {len(mv)} bytes, the fixed header alone is {_FIXED.size}")
    magic, version, N, ndim, reserved, C, segment, lamb, n_words, dig = _FIXED.unpack_from(mv, 0)
    if magic != MAGIC:
        raise ValueError(f"not a VBQ bitstream (magic {magic!r})")
    if version != VERSION:
        raise ValueError(f"unknown bitstream version {version}")
    if reserved != 0:
        raise ValueError(f"reserved header byte is {reserved}, not 0")
    if ndim < 1:
        raise ValueError("latent shape with 0 dimensions")
    hlen = _FIXED.size + 8 * ndim
    if len(mv) < hlen:
        raise ValueError(f"truncated in the latent shape: {len(mv)} bytes, the header is {hlen}")
    shape = tuple(int(d) for d in np.frombuffer(mv, dtype="<u8", count=ndim, offset=_FIXED.size))
    _check_fields(N, C, shape, lamb, segment, dig, n_words)
    h = Header(N=N, C=C, shape=shape, lamb=float(lamb), segment=segment, digest=bytes(dig), n_words=n_words)
    need = hlen + 2 * h.n_sizes + 2 * n_words
    if len(mv) < need:
        raise ValueError(f"truncated: {len(mv)} bytes, header, {h.n_sizes} segment sizes and {n_words} payload words "
                         f"need {need}")
    if len(mv) > need:
        raise ValueError(f"{len(mv) - need} trailing bytes after the payload")
    sizes = np.frombuffer(mv, dtype="<u2", count=h.n_sizes, offset=hlen)
    _check_sizes(sizes, segment, n_words)
    return h, sizes, hlen + 2 * h.n_sizes
