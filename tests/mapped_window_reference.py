"""What the mapped window decode must give, without a GPU: lambda-map files (magic b"VBQm") and files in segments (b"VBQb") written
on the host from the NumPy coder of tests/mapped_reference.py, the expected output of a window -- that coder's decode of the
whole file, the sorted code points, a slice --, and a restatement of the staging buffer of
ChannelwisePriorCDFQuantizer._mapped_window_plan from its documented layout (include/vbq.h, "Mapped window decode")."""
import numpy as np

import mapped_reference as MR
from vbq_amd import bitstream as bs


def host_quantizer(C, N, lambs, sigma=None, seed=0):
    """Code points and entropy models installed from arrays: nothing here touches a device.  The counts of each lambda pile up
    around another centre, so that the tables of a palette are far apart."""
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    q = ChannelwisePriorCDFQuantizer(C, N)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C), np.linspace(0.5, 2.0, C) if sigma is None else np.asarray(sigma)))
    T = q.quantization_levels
    rng = np.random.default_rng(seed)
    counts = {}
    for l, lamb in enumerate(lambs):
        centre = T * (l + 1) // (len(lambs) + 1)
        counts[lamb] = np.stack([np.bincount(np.clip(np.rint(rng.normal(centre, 1.5, 400)), 0, T - 1).astype(np.int64), minlength=T)
                                 for _ in range(C)])
    q._code_counts, q._add_n_smoothing = counts, 1
    q.entropy_models = {lamb: -np.log2((c + 1) / (c + 1).sum(axis=1, keepdims=True)).astype(np.float32) for lamb, c in counts.items()}
    return q


def tables_of(q, lambs, seg):
    """(freq u16 [P, C, T], digests) of a palette."""
    pairs = [q._coder_tables(q._lambda_key(l), seg) for l in lambs]
    return np.stack([c.freq_host.numpy() for c, _ in pairs]), tuple(d for _, d in pairs)


def draw_indices(freq, cls, rng):
    """idx u16 [C, B]: symbol b of channel c drawn from the table of its class (so a wrong class decodes something else)."""
    P, C, T = freq.shape
    idx = np.empty((C, cls.size), np.uint16)
    for c in range(C):
        for p in range(P):
            where = np.flatnonzero(cls == p)
            idx[c, where] = rng.choice(T, where.size, p=freq[p, c].astype(np.float64) / (1 << 15))
    return idx


def write_file(q, shape, lambs, cls, seg, rng, mapped=True):
    """A file of q written on the host -> (bytes, idx u16 [C, B]): `lambs` the palette, cls [B] in [0, P); mapped=False writes
    the b"VBQb" file of lambs[0] (cls all zero)."""
    freq, digests = tables_of(q, lambs, seg)
    cls = np.asarray(cls, np.uint8).reshape(-1)
    idx = draw_indices(freq, cls, rng)
    words, sizes = MR.encode(idx, cls, freq, seg)
    payload = words[np.arange(seg + 2)[None, None, :] < sizes[..., None].astype(np.int64)]
    kw = dict(N=q.max_bits_per_coord, C=q.num_channels, shape=tuple(shape), segment=seg, n_words=int(payload.size))
    if mapped:
        h = bs.MappedHeader(lambs=tuple(float(l) for l in lambs), digests=digests, **kw)
        return bs.write_mapped(h, cls, sizes, payload), idx
    assert len(lambs) == 1 and not cls.any()
    return bs.write(bs.Header(lamb=float(lambs[0]), digest=digests[0], **kw), sizes, payload), idx


def decode_file(q, data):
    """Z_hat of a whole file, shaped like the latents: mapped_reference.decode over the file's own classes, sizes and payload,
    then the sorted code points.  The status of the decode must be 0."""
    raw = memoryview(data).cast("B")
    if bytes(raw[:4]) == bs.MAPPED_MAGIC:
        h, cls, sizes, start = bs.parse_mapped(data)
        lambs = h.lambs
    else:
        h, sizes, start = bs.parse(data)
        cls, lambs = np.zeros(h.n_rows, np.uint8), (h.lamb,)
    freq, _ = tables_of(q, lambs, h.segment)
    sizes = sizes.astype(np.int64).reshape(h.C, h.nseg)
    pay = np.frombuffer(raw, dtype="<u2", count=h.n_words, offset=start)
    words = np.zeros((h.C, h.nseg, h.segment + 2), np.uint16)
    words[np.arange(h.segment + 2)[None, None, :] < sizes[..., None]] = pay
    idx, status = MR.decode(words, sizes, cls, freq, h.n_rows, h.segment)
    assert status == 0
    return np.take_along_axis(q.code_points_by_channel, idx.astype(np.int64), axis=1).T.reshape(h.shape)


def expected(q, files, regions, channels=None):
    """[F, *extents, C_sel]: decode_file(files[f])[regions[f]][..., channels]."""
    ch = slice(None) if channels is None else list(channels)
    return np.stack([decode_file(q, d)[tuple(r) if r is not None else ()][..., ch] for d, r in zip(files, regions)])


def restated_plan(q, files, regions, channels=None):
    """The staging buffer of the mapped window decode, part by part, from the documented layout -> dict of NumPy arrays and
    numbers: desc int64 [F, 16], segs int32 [F, n_sel], channels int32 [C_sel] or None, cls (bytes), sizes u16, payload u16,
    tables (the distinct lambdas, ascending), max_P."""
    heads = []
    for d in files:
        raw = bytes(d)
        if raw[:4] == bs.MAPPED_MAGIC:
            h, _, sizes, start = bs.parse_mapped(raw)
            heads.append((h, h.lambs, raw[h.nbytes: h.nbytes + 8 * ((h.n_rows + 31) // 32)], sizes, start, raw))
        else:
            h, sizes, start = bs.parse(raw)
            heads.append((h, (h.lamb,), None, sizes, start, raw))
    tables = sorted({float(l) for _, lambs, *_ in heads for l in lambs})
    boxes, extents = bs.region_boxes([h.shape[:-1] for h, *_ in heads], regions)
    seg = heads[0][0].segment
    lists = [bs.box_segments(dims, lo, hi, seg) for dims, lo, hi in boxes]
    n_sel = max(l.size for l in lists)
    F = len(files)
    desc, segs = np.zeros((F, 16), np.int64), np.full((F, n_sel), -1, np.int32)
    cls, seg_base = b"", 0
    for f, ((h, lambs, block, sizes, start, raw), (dims, lo, hi)) in enumerate(zip(heads, boxes)):
        desc[f, :8] = (seg_base, h.n_rows, dims[1], dims[2], lo[0], lo[1], lo[2], len(lambs))
        desc[f, 8: 8 + len(lambs)] = [tables.index(float(l)) for l in lambs]
        desc[f, 12] = -1 if block is None else len(cls)
        cls += block or b""
        seg_base += sizes.size
        segs[f, : lists[f].size] = lists[f]
    return dict(desc=desc, segs=segs, channels=None if channels is None else np.asarray(channels, np.int32), cls=cls,
                sizes=np.concatenate([s for _, _, _, s, _, _ in heads]),
                payload=np.concatenate([np.frombuffer(raw, "<u2", h.n_words, start) for h, _, _, _, start, raw in heads]),
                tables=tables, max_P=max(len(lambs) for _, lambs, *_ in heads), shape=(F,) + tuple(extents))
