"""Latent files that stay on the device (vbq_amd/store/vbq_store.h, libvbq_store.so): LatentStore uploads a set of b"VBQb" /
b"VBQm" files once and decodes boxes of them from file ids and origins that live on the device.  Per call: one
vbqs_plan_boxes launch (ids, origins -> descriptors and segment lists) and one launch of a window decoder of include/vbq.h
into it; no header is parsed, nothing is uploaded or read back, the host is not synchronised.  There is no CPU path: importing
this module without the built library raises VBQError."""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import _lib, _lib_store, bitstream, coder, ops

_lib_store.lib()                                 # a missing library is an error here, not at the first call

MAX_SAMPLES_PER_LAUNCH = bitstream.MAX_BATCH_FILES   # the decoders' limit on files per launch: a sample is a file to them
PLAN_CUT, PLAN_BAD_SAMPLE = 32, 128              # status bits 5 and 7 of vbqs_plan_boxes, as the decoders mean them


def max_listed_segments(dims, extents, segment) -> int:
    """An upper bound, from the host's knowledge alone, on the number of segments of `segment` symbols that hold a row of ANY
    box of `extents` = (w0, w1, w2) in the geometry dims = (D0, D1, D2): the smallest of the segments of a stream, w0 w1 runs
    of w2 rows each, and w0 spans of (w1 - 1) D2 + w2 rows each.  0 for an empty box."""
    (D0, D1, D2), (w0, w1, w2), seg = (int(d) for d in dims), (int(w) for w in extents), int(segment)
    if min(w0, w1, w2) <= 0:
        return 0
    nseg = (D0 * D1 * D2 + seg - 1) // seg
    return min(nseg, w0 * w1 * ((w2 + seg - 2) // seg + 1), w0 * (((w1 - 1) * D2 + w2 + seg - 2) // seg + 1))


def file_dims(shape):
    """The three nested levels of a latent of `shape` (channel-last): D1, D2 its last two leading axes, D0 the rest."""
    lead = (1, 1, 1) + tuple(int(d) for d in shape[:-1])
    return math.prod(lead[:-2]), lead[-2], lead[-1]


def plan_boxes(table, ids, origins, extents, *, seg, n_sel, desc=None, segs=None, status=None):
    """vbqs_plan_boxes: table int64 [F, 8 or 16], ids int64 [S], origins int64 [S, 3], extents (w0, w1, w2) -> (desc int64
    [S, fields], segs int32 [S, n_sel], status u32 [S]), on the stream of `ids`.  `status` is OR-ed into: zeroed here unless
    given.  With S == 0, an empty box or n_sel == 0 nothing is launched and new outputs stay as allocated."""
    table, ids, origins = ops._dev(table, torch.int64, "table"), ops._dev(ids, torch.int64, "ids"), ops._dev(origins, torch.int64, "origins")
    if table.dim() != 2 or ids.dim() != 1 or tuple(origins.shape) != (ids.shape[0], 3):
        raise ValueError(f"expected table [F, fields], ids [S] and origins [S, 3], got {tuple(table.shape)}, {tuple(ids.shape)} "
                         f"and {tuple(origins.shape)}")
    S, (F, fields), n_sel = ids.shape[0], table.shape, int(n_sel)
    w0, w1, w2 = (int(w) for w in extents)
    reads = (("table", table), ("ids", ids), ("origins", origins))
    desc = ops._out(desc, (S, fields), torch.int64, ids.device, "desc", True, reads)
    segs = ops._out(segs, (S, n_sel), torch.int32, ids.device, "segs", True, reads + (("desc", desc),))
    if status is None:
        status = torch.zeros(S, dtype=torch.uint32, device=ids.device)
    else:
        status = ops._status(status, S, ids.device, reads + (("desc", desc), ("segs", segs)))
    _lib_store.check(_lib_store.lib().vbqs_plan_boxes(ops._ptr(table), F, fields, ops._ptr(ids), ops._ptr(origins), S, w0, w1, w2,
                                                      int(seg), n_sel, ops._ptr(desc), ops._ptr(segs), ops._ptr(status),
                                                      ops._stream(ids)), "vbqs_plan_boxes")
    return desc, segs, status


class LatentStore:
    """A set of latent files of one quantizer, resident on its device.

        store = LatentStore(q, files)                    # every check, ONE upload, one offsets scan, one status read
        out, status = store.crops(ids, origins, extents) # two launches per 65535 samples; nothing read back, no synchronisation
        store.check(status, ids)                         # the one host read
        z = store.read(ids, origins, extents)            # crops + check
        ids, origins = store.sample(S, extents)          # uniform valid boxes, drawn on the device
        store.verify()                                   # every file in full

    `files`: b"VBQb" and b"VBQm" byte strings of `q`, mixed -- any built lambdas, any palettes, any latent shapes, ONE segment
    length.  Each gets the checks of decompress_latents_mapped_batch: ValueError naming the file's index for a compact file,
    another N / C / segment or a digest mismatch, KeyError for a lambda without a model.  A file's geometry is (D0, D1, D2) =
    file_dims(shape); sample s of a call is the box origins[s] + [0, extents) of file ids[s], and every value of it is
    bit-identical to decompress_latents(files[ids[s]]) reshaped to (D0, D1, D2, C) and sliced there.

    The store CLONES the frequency tables [n_tables, C, T] of the lambdas its files use and the sorted code points [C, T] at
    construction.  It therefore keeps answering with the models the files were written under, whatever `q` rebuilds or recycles
    later; it does not see a later change of `q`, and a file written after such a change belongs in a new store.

    One stream at a time: the store's scratch (descriptors, segment lists) is allocated per call on the caller's stream."""

    def __init__(self, q, files):
        files = q._window_inputs(files, None, None)[0]
        if not files:
            raise ValueError("a store needs at least one file")
        heads, starts, keys = q._mapped_window_headers(files)
        F, C = len(files), q.num_channels
        self.n_files, self.segment, self.device = F, int(heads[0].segment), q.device
        self.shapes = [tuple(int(d) for d in h.shape) for h in heads]
        self.dims = [file_dims(s) for s in self.shapes]
        self.num_channels, self._N = C, q.max_bits_per_coord
        for i, h in enumerate(heads):
            if h.n_sizes // C > np.iinfo(np.int32).max:
                raise ValueError(f"file {i}: {h.n_sizes // C} segments per stream are too many")
        mapped = [isinstance(h, bitstream.MappedHeader) for h in heads]
        fields = self._fields = 16 if any(mapped) else 8
        tables = sorted({k for palette in keys for k in palette}, key=float)
        self.max_classes = max(len(p) for p in keys)
        table = np.zeros((F, fields), np.int64)
        raws = [np.frombuffer(memoryview(d).cast("B"), dtype=np.uint8) for d in files]
        blocks, cls_bytes, base = [], 0, 0
        for f, (h, r, palette, dims) in enumerate(zip(heads, raws, keys, self.dims)):
            table[f, :4] = (base, h.n_rows, dims[1], dims[2])
            base += h.n_sizes
            if fields == 8:
                table[f, 7] = tables.index(palette[0])
                continue
            table[f, 7] = len(palette)
            table[f, 8: 8 + len(palette)] = [tables.index(k) for k in palette]
            table[f, 12] = -1
            if mapped[f]:
                table[f, 12] = cls_bytes
                blocks.append(r[h.nbytes: h.sizes_offset])
                cls_bytes += h.classes_nbytes
        M, n_words = base, sum(h.n_words for h in heads)
        host = np.concatenate([table.view(np.uint8).reshape(-1)] + blocks
                              + [r[s - 2 * h.n_sizes: s] for r, h, s in zip(raws, heads, starts)]    # (the sizes end where the
                              + [r[s: s + 2 * h.n_words] for r, h, s in zip(raws, heads, starts)])   # payload starts)
        cut = [int(c) for c in np.cumsum([0, table.nbytes, cls_bytes, 2 * M, 2 * n_words])]
        dev = self._dev = torch.from_numpy(host).to(self.device)                                      # the one upload
        self._table = dev[cut[0]:cut[1]].view(torch.int64).view(F, fields)
        self._cls = dev[cut[1]:cut[2]] if cls_bytes else None
        self._sizes, self._payload = dev[cut[2]:cut[3]].view(torch.uint16), dev[cut[3]:cut[4]].view(torch.uint16)
        self._offsets = torch.empty(M, dtype=torch.int64, device=self.device)
        scan = torch.zeros(1, dtype=torch.uint32, device=self.device)
        _lib.check(_lib.lib().vbq_rans_segment_offsets_u16(ops._ptr(self._sizes), M, self.segment, n_words, ops._ptr(self._offsets),
                                                            ops._ptr(scan), ops._stream(dev)), "vbq_rans_segment_offsets_u16")
        self._freq = q._coder_stack(tables, self.segment)._freq(self.device).view(len(tables), C, -1).clone()
        self._values = q._sorted_dev().clone()
        coder._raise_status(int(scan.cpu()[0]))                                                       # the one read
        self.nbytes = sum(t.numel() * t.element_size() for t in (dev, self._offsets, self._freq, self._values))
        self._cache = {}

    # ------------------------------------------------------------------ what the host knows: shapes only
    def _extents(self, extents):
        ext = tuple(int(w) for w in extents)
        if len(ext) not in (2, 3) or min(ext) < 0:
            raise ValueError(f"extents must be (w0, w1, w2) or (h, w), every one >= 0, got {tuple(extents)}")
        return ((1,) + ext if len(ext) == 2 else ext), len(ext) == 2

    def _n_sel(self, box):
        return max(max_listed_segments(d, box, self.segment) for d in self.dims)

    def _cached(self, key, make):
        hit = self._cache.get(key)
        if hit is None:
            if len(self._cache) >= 64:
                self._cache.clear()
            hit = self._cache[key] = make()
        return hit

    def _channels(self, channels):
        """(the channel list on the device or None for all, C_sel); a list is uploaded the first time it is seen."""
        C = self.num_channels
        if channels is None:
            return None, C
        ch = np.asarray(channels).reshape(-1)
        if ch.size and (ch.dtype.kind not in "iu" or int(ch.min()) < 0 or int(ch.max()) >= C):
            raise ValueError(f"channels must be integers in [0, {C})")
        if ch.size == 0:
            return None, 0
        ch = ch.astype(np.int32)
        return self._cached(("channels", ch.tobytes()), lambda: torch.from_numpy(ch).to(self.device)), int(ch.size)

    def _samples(self, ids, origins, short):
        """ids int64 [S] and origins int64 [S, 3] on the device; host values are uploaded, device tensors used where they are."""
        if not (isinstance(ids, torch.Tensor) and ids.is_cuda):
            ids = ops.upload(np.asarray(ids).reshape(-1), self.device, torch.int64)
        if not (isinstance(origins, torch.Tensor) and origins.is_cuda):
            host = np.asarray(origins)
            origins = ops.upload(host if host.ndim == 2 else host.reshape(-1, 2 if short else 3), self.device, torch.int64)
        if ids.dtype != torch.int64 or origins.dtype != torch.int64:
            raise ValueError(f"ids and origins must be int64, got {ids.dtype} and {origins.dtype}")
        S, k = ids.shape[0], 2 if short else 3
        if ids.dim() != 1 or tuple(origins.shape) not in ((S, 3), (S, k)):
            raise ValueError(f"expected ids [S] and origins [S, {k}], got {tuple(ids.shape)} and {tuple(origins.shape)}")
        if origins.shape[1] == 2:
            origins = torch.cat([torch.zeros((S, 1), dtype=torch.int64, device=origins.device), origins], dim=1)
        return ids.contiguous(), origins.contiguous()

    # ------------------------------------------------------------------ the calls
    def crops(self, ids, origins, extents, channels=None, out=None, status=None):
        """The boxes origins[s] + [0, extents) of the files ids[s] -> (out f32 [S, w0, w1, w2, C_sel], status u32 [S]).  `ids`
        int64 [S] and `origins` int64 [S, 3]: device tensors (used where they are; nothing is read back) or anything
        np.asarray takes (uploaded).  `extents`: Python ints; (h, w) with origins [S, 2] means origins (0, y, x) and extents
        (1, h, w), and the result is [S, h, w, C_sel].  `channels` as in decompress_latents_batch.  Per 65535 samples ONE
        vbqs_plan_boxes and ONE decode launch, into views of `out` and `status`.  `status` is OR-ed into (zeroed unless given):
        bit 7 (128) an id outside the store or a box outside its file, the other bits the decoders' (coder._raise_status).
        The values of a sample whose status is non-zero are unspecified; a given `out` keeps its content at an invalid one."""
        box, short = self._extents(extents)
        ch, C_sel = self._channels(channels)
        ids, origins = self._samples(ids, origins, short)
        S, dev = ids.shape[0], ids.device
        shape = (S,) + (box[1:] if short else box) + (C_sel,)
        out = ops._out(out, shape, torch.float32, dev, "out", True, (("ids", ids), ("origins", origins)))
        status = torch.zeros(S, dtype=torch.uint32, device=dev) if status is None else ops._status(
            status, S, dev, (("ids", ids), ("origins", origins), ("out", out)))
        if S == 0 or C_sel == 0 or 0 in box:
            return out, status
        n_sel = self._n_sel(box)
        desc = torch.empty((S, self._fields), dtype=torch.int64, device=dev)
        segs = torch.empty((S, n_sel), dtype=torch.int32, device=dev)
        full = out.view((S,) + box + (C_sel,))
        for s0 in range(0, S, MAX_SAMPLES_PER_LAUNCH):
            s1 = min(S, s0 + MAX_SAMPLES_PER_LAUNCH)
            plan_boxes(self._table, ids[s0:s1], origins[s0:s1], box, seg=self.segment, n_sel=n_sel, desc=desc[s0:s1],
                       segs=segs[s0:s1], status=status[s0:s1])
            if self._fields == 8:
                ops.rans_decode_window(self._payload, self._sizes, self._offsets, desc[s0:s1], segs[s0:s1], self._freq, self._values,
                                       box, seg=self.segment, N=self._N, channels=ch, status=status[s0:s1], out=full[s0:s1])
            else:
                ops.rans_map_decode_window(self._payload, self._sizes, self._offsets, desc[s0:s1], segs[s0:s1], self._freq,
                                           self._values, self._cls, box, seg=self.segment, max_classes=self.max_classes,
                                           N=self._N, channels=ch, status=status[s0:s1], out=full[s0:s1])
        return out, status

    def check(self, status, ids=None):
        """The one host read of a crops call: VBQError("sample i (file f): ...") for the first non-zero status word, ValueError
        naming the sample when that word has bit 7 -- an id outside the store or a box outside its file.  `ids`: what crops
        was given; without them the file is not named."""
        words = status.to(torch.int64).reshape(-1)
        if isinstance(ids, torch.Tensor) and ids.is_cuda:
            both = torch.stack([words, ids.reshape(-1)]).cpu().numpy()
            st, ids = both[0], both[1]
        else:
            st = words.cpu().numpy()
            ids = None if ids is None else np.asarray(ids).reshape(-1)
        bad = np.flatnonzero(st)
        if bad.size == 0:
            return
        i = int(bad[0])
        who = f"sample {i}" if ids is None else f"sample {i} (file {int(ids[i])})"
        if int(st[i]) & PLAN_BAD_SAMPLE:
            raise ValueError(f"{who}: no such file among the {self.n_files} resident ones, or a box that does not lie in it")
        try:
            coder._raise_status(int(st[i]))
        except _lib.VBQError as e:
            raise _lib.VBQError(f"{who}: {e}") from None

    def read(self, ids, origins, extents, channels=None, return_np=False):
        """crops, then check: the boxes, or the error of the first bad sample."""
        out, status = self.crops(ids, origins, extents, channels)
        self.check(status, ids)
        return out.cpu().numpy() if return_np else out

    def sample(self, S, extents, generator=None):
        """S uniform boxes of `extents`, drawn on the device: (ids int64 [S], origins int64 [S, 3], or [S, 2] for extents
        (h, w)).  File ids are uniform over the files that can hold the extents, origins uniform over each chosen file's own
        valid range; deterministic under `generator` (a generator of the store's device).  ValueError if no file can hold
        the extents."""
        box, short = self._extents(extents)

        def ranges():
            ok = [f for f, d in enumerate(self.dims) if all(w <= D for w, D in zip(box, d))]
            if not ok:
                raise ValueError(f"no resident file can hold a box of extents {tuple(extents)}")
            span = np.array([[D - w + 1 for w, D in zip(box, self.dims[f])] for f in ok], np.int64)
            if short:
                span[:, 0] = 1                                      # (h, w) boxes sit at i0 = 0
            return torch.from_numpy(np.array(ok, np.int64)).to(self.device), torch.from_numpy(span).to(self.device)
        ok, span = self._cached(("sample", box, short), ranges)
        S = int(S)
        pick = torch.randint(0, ok.shape[0], (S,), generator=generator, device=self.device)
        u = torch.rand((S, 3), dtype=torch.float64, generator=generator, device=self.device)
        room = span[pick]
        origins = torch.minimum((u * room).to(torch.int64), room - 1)
        return ok[pick], origins[:, 1:].contiguous() if short else origins

    def verify(self):
        """Every file decoded in full -- one crops per distinct geometry -- and checked: what crops leaves unseen, damage in
        segments no box touched, raises here (VBQError naming the file)."""
        groups = {}
        for f, d in enumerate(self.dims):
            groups.setdefault(d, []).append(f)
        for d, members in groups.items():
            if 0 in d:
                continue
            ids = torch.from_numpy(np.array(members, np.int64)).to(self.device)
            _, status = self.crops(ids, torch.zeros((len(members), 3), dtype=torch.int64, device=self.device), d)
            self.check(status, members)
