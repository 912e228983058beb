"""Every buffer a caller can hand the binding to be written: one parametrised case per ARG row of tests/written_buffers.py.

Per row, with the smallest valid arguments of its function (the scale of the `V` fixture of tests/test_gpu_ops_refusals.py; the
batch, window and store calls take the three-file builders of their own modules, with ONE file or sample made invalid by a
documented, range-checked refusal -- n < 1, a table or an id out of range -- so that its status word is not zero and its slots
are kept):

  refused      one defect at a time -- a dtype of smaller and of larger itemsize, one element short, one dimension off, on the
               host, every second element of a wider buffer, a stride-0 `expand`, and for the one-word statuses an empty tensor --
               raises ValueError (VBQError where the function already says so for a host tensor) while `_NoKernels` stands in for
               all five libraries: a missing check fails on the host with "was reached", never on the device.  The buffer is
               untouched.
  written      a valid buffer inside a footprint.Guarded at element offsets 0 and 1 (workspaces: exactly the bytes asked for, 256-
               byte aligned) comes back as the very object, the guards are intact, and the content is, bit for bit, the earlier
               content combined with what the call writes into a plain new tensor: assigned, `+` for counts, sums and totals, OR
               for status, kept for the slots no item names (found as the slots on which two different earlier contents survive).
               Where the call returns such a tensor when it is given nothing, that result is compared too.  The IN_PLACE rows
               run here, on the real library, with an earlier content that is not neutral; what the call gives from nothing is
               what each function's own module compares with its reference.
  overlap      through the stand-in: the buffer laid over each input's storage, over its first bytes by one element, over its
               last element, and over every other buffer of the call that the caller can supply, is refused with the sentence
               that names both.  Control: the buffer directly behind an input in one allocation (its first byte is the input's
               last byte + 1) is accepted by the real library and gives the right answer.
  inputs       after every valid call above every input holds the bits it held.

dist.CountsAllReduce runs in a process group of this one process (gloo, a file store): with one rank the sums are the counts, so
its row shows that wait() unpacks into the very tensor start() was given, not a changed value.

Nothing needs a tolerance.  Accumulating float outputs are compared at shapes where each output element receives one addition."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import footprint as FP  # noqa: E402
import written_buffers as WB  # noqa: E402
from test_gpu_ops_refusals import BASE, C, L, N, ROWS, T, V, _NoKernels, _need_gpu, _solve  # noqa: E402,F401  (V, _need_gpu: fixtures)

pytestmark = pytest.mark.gpu
DEV = "cuda"
QUERIES = ("vbq_records_words",)
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
SMALLER = {torch.uint8: torch.int8, torch.uint16: torch.uint8, torch.int16: torch.int8, torch.int32: torch.int16, torch.uint32: torch.uint16,
           torch.float32: torch.float16, torch.int64: torch.int32, torch.uint64: torch.uint32, torch.float64: torch.float32}
"""(uint8 has nothing smaller: the other one-byte integer stands in.)"""
LARGER = {torch.uint8: torch.uint16, torch.uint16: torch.uint32, torch.int32: torch.int64, torch.uint32: torch.uint64,
          torch.float32: torch.float64, torch.int64: torch.complex128, torch.uint64: torch.complex128, torch.float64: torch.complex128}


@pytest.fixture(autouse=True)
def _stop_at_a_device_error():
    """Nothing here is meant to fault.  Should the device report an error all the same, no later case may launch on it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error, the run ends here: {e}", 3)


class _Stand(_NoKernels):
    """_NoKernels, and the pure size queries that are not named *_workspace_bytes."""

    def __getattr__(self, name):
        return getattr(self._real, name) if name in QUERIES else super().__getattr__(name)


def _stand_in(monkeypatch):
    from vbq_amd import _lib, _lib_budget, _lib_ext, _lib_kmeans, _lib_store
    for m in (_lib, _lib_ext, _lib_budget, _lib_kmeans, _lib_store):
        real = m.lib()
        monkeypatch.setattr(m, "lib", lambda real=real: _Stand(real))


# ------------------------------------------------------------------------------------------------------------------ bits
def dev(a, dtype=None, shape=None):
    """A NumPy array as a device tensor of `dtype` (default: its own) with the same bytes."""
    a = np.ascontiguousarray(a)
    dtype = dtype or {np.dtype(v): k for k, v in FP._NP.items()}[a.dtype]
    raw = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to(DEV)
    return raw.view(dtype).view(a.shape if shape is None else shape)


def bits(t):
    """A dense tensor as unsigned integers of its element size (host)."""
    size = t.element_size()
    return t.reshape(-1).view(torch.uint8).cpu().numpy().view(UINT[size]).reshape(tuple(t.shape))


def pattern(buf, other=False):
    """An earlier content that is neither zero nor the canary, as the buffer's real NumPy dtype; `other`: a second one that
    differs from the first in every element."""
    n = int(np.prod(buf.shape, dtype=np.int64))
    npd = np.dtype(FP._NP[buf.dtype])
    if buf.kind == "or":
        a = ((1 << 20) << (np.arange(n) % 3)).astype(npd)
    elif npd.kind == "f":
        a = (3.0 + np.arange(n) % 5).astype(npd)
    else:
        a = (5 + np.arange(n) % 7).astype(npd)
    if other:
        a = (a.view(UINT[npd.itemsize]) ^ UINT[npd.itemsize](0x0101 & (256 ** npd.itemsize - 1))).view(npd) if npd.kind != "f" else (a + 8).astype(npd)
    return a.reshape(buf.shape)


# ------------------------------------------------------------------------------------------------------------------ faces
class Buf:
    """One buffer of a face.  kind: "assign", "add", "or", "keep", "state" (in/out, always required) or "ws"; pick(ret) -> the
    tensor of the call's result that must be the buffer (None: the call does not return it); init: the earlier content a
    required buffer starts from (NumPy); nothing: (extra keywords, pick) to get the call's own tensor when it is given none."""

    def __init__(self, shape, dtype, kind, pick=None, init=None, required=False, nothing=None, short=True, also=()):
        self.shape, self.dtype, self.kind, self.pick = tuple(int(s) for s in shape), dtype, kind, pick
        self.init, self.required, self.nothing, self.short = init, required or kind == "state", nothing, short
        self.also = also                                                    # the other dtypes the entry point takes
        self.itemsize = np.dtype(FP._NP[dtype]).itemsize
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.itemsize

    def start(self):
        """The neutral earlier content of a plain new tensor."""
        if self.init is not None:
            return np.ascontiguousarray(self.init, FP._NP[self.dtype]).reshape(self.shape)
        return np.zeros(self.shape, FP._NP[self.dtype])


class Face:
    """scratch: keywords of `fn` that stand for memory of the object under test which the call writes -- laid out like inputs,
    not expected to keep their bits."""

    def __init__(self, fn, kwargs, buffers, scratch=()):
        self.fn, self.kwargs, self.buffers, self.scratch = fn, kwargs, buffers, scratch

    def inputs(self, kwargs=None, scratch=True):
        return {k: v for k, v in (kwargs or self.kwargs).items() if isinstance(v, torch.Tensor) and (scratch or k not in self.scratch)}

    def run(self, given, kwargs=None, extra=None):
        kw = dict(self.kwargs if kwargs is None else kwargs)
        for name, b in self.buffers.items():
            if b.required and name not in given:
                kw[name] = dev(b.start())
        kw.update(given)
        kw.update(extra or {})
        ret = self.fn(**kw)
        torch.cuda.synchronize()
        return ret


_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _u16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16)).to(DEV)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _records():
    """Five records of K = 6 coordinates, N = 4: even rank indices have bit length N, so every row holds K * N bits."""
    def make():
        from vbq_amd import ops
        rng = np.random.default_rng(11)
        K, R = 6, 5
        idx = (2 * rng.integers(0, T // 2, (R, K))).astype(np.uint16)
        words = ops.records_pack(_u16(idx), K * N, N)
        table = _t(np.sort(rng.standard_normal(T)).astype(np.float32))
        emb = _t(rng.standard_normal((R, K)).astype(np.float32))
        return dict(K=K, R=R, total=K * N, idx=idx, words=words, table=table, emb=emb,
                    queries=_t(rng.standard_normal((2, K)).astype(np.float32)), RW=words.shape[1])
    return _once("records", make)


def _prior_case():
    def make():
        import test_gpu_bmshj as TB
        rng = np.random.default_rng(5)
        params = TB._prior(C, 10.0, seed=C)._params()
        xi = _t((rng.random((ROWS, C)) * 0.998 + 0.001).astype(np.float32))
        x_cb = _t((rng.standard_normal((C, ROWS)) * 2).astype(np.float32))
        return params, xi, x_cb
    return _once("prior", make)


def _budget(big):
    def make():
        rng = np.random.default_rng(9)
        R, K, Nb = (7, 300, 16) if big else (4, 3, 2)
        fhat = -np.abs(rng.standard_normal((Nb + 1, R * K)))
        fhat[1, K + 1] = np.nan                                             # row 1: status bit 0
        return _t(fhat), K, (1600 if big else 3), R, Nb
    return _once(("budget", big), make)


def _bad_file(files, col, value=0):
    files = np.array(files, np.int64)
    assert files.shape[0] >= 2, "a per-file status of one file is one word: no strided [F] view of it is strided"
    files[1, col] = value
    return _t(files)


def _window():
    def make():
        import test_gpu_mapped_window as MW
        import test_gpu_window as W
        from vbq_amd import bitstream as bs
        shapes = [(1, 17, 23), (1, 20, 30), (2, 9, 11)]
        k = W.Coded(shapes, [0, 1, 0], 2, 8, 64, 10, seed=5)
        boxes, _ = bs.region_boxes(shapes, MW.REGIONS3)
        lists = [bs.box_segments(d, lo, hi, k.seg) for d, lo, hi in boxes]
        segs = np.full((3, max(l.size for l in lists)), -1, np.int32)
        for f, l in enumerate(lists):
            segs[f, :l.size] = l
        files = np.array([[b, int(np.prod(s)), d[1], d[2], lo[0], lo[1], lo[2], t]
                          for b, s, (d, lo, hi), t in zip(k.seg_base, shapes, boxes, k.tables)], np.int64)
        box = tuple(h - l for l, h in zip(boxes[0][1], boxes[0][2]))
        rng = np.random.default_rng(17)
        m = MW.MappedCoded([(MW.SHAPES3[0], [2], None), (MW.SHAPES3[1], [0, 3], rng.integers(0, 2, 600).astype(np.uint8)),
                            (MW.SHAPES3[2], [1, 4, 0, 2], rng.integers(0, 4, 198).astype(np.uint8))], 5, 8, 64, 10, seed=11)
        m_files, m_segs, m_box, _, _ = m.stage(MW.REGIONS3)
        return k, files, segs, box, m, m_files, m_segs, m_box
    return _once("window", make)


def _store(mapped):
    """Three resident files of latents 1..3 of tests/test_gpu_store.py: all b"VBQb" (crops decodes through
    vbq_rans_decode_window_f32), or one b"VBQb" and two b"VBQm" with that module's palettes (16-field descriptors:
    vbq_rans_map_decode_window_f32)."""
    def make():
        import test_gpu_store as TS
        from vbq_amd.store import LatentStore
        q, lat, rng = _once("store quantizer", lambda: TS._quantizer(7))
        if not mapped:
            files = [q.compress_latents_to_bytes(*lat[i], TS.LAMBS[0], segment=TS.SEG) for i in (1, 2, 3)]
        else:
            files = [q.compress_latents_to_bytes(*lat[1], TS.PALETTES[1][0], segment=TS.SEG)] + [
                q.compress_latents_to_bytes_mapped(*lat[i], TS.PALETTES[i], rng.integers(0, len(TS.PALETTES[i]), TS.SHAPES[i][:-1]),
                                                   segment=TS.SEG) for i in (2, 3)]
        st = LatentStore(q, files)
        assert st._fields == (16 if mapped else 8)
        return st, TS.C32
    return _once(("store", mapped), make)


def _reducer():
    """A CountsAllReduce of six counters in a process group of this one process (gloo, a file store: no port, no child)."""
    def make():
        import tempfile
        import torch.distributed as dist
        from vbq_amd.dist import CountsAllReduce
        if not dist.is_initialized():
            dist.init_process_group("gloo", init_method="file://" + tempfile.mkdtemp(prefix="vbq_written_buffers_") + "/store", rank=0, world_size=1)
        red = CountsAllReduce(6, torch.device("cuda", torch.cuda.current_device()), max_global_count=1000)
        assert red.packed
        return red
    return _once("reducer", make)


@pytest.fixture(scope="module", autouse=True)
def _leave_no_process_group():
    yield
    import torch.distributed as dist
    if "reducer" in _CACHE and dist.is_initialized():
        dist.destroy_process_group()


def _codec_case():
    def make():
        from test_gpu_ops_refusals import _codec
        codec, idx = _codec()
        sz, pay = codec.encode_packed(_u16(idx))
        sz = sz.astype(np.uint16).reshape(-1)
        sz[3] = 40                                                          # more words than a segment of 32 symbols holds
        return codec, _t(pay), _t(sz)
    return _once("codec", make)


def face(name, entry, arg, V):
    """The Face of `name` for the row of the entry point `entry` and the Python parameter `arg`: the valid arguments and every
    buffer a caller can supply."""
    from vbq_amd import _lib, _lib_kmeans, kmeans1d, ops, store
    h = _lib.lib()
    f32, f64, u16, u32, u64, i32, i64, u8 = (torch.float32, torch.float64, torch.uint16, torch.uint32, torch.uint64, torch.int32,
                                             torch.int64, torch.uint8)
    lam = (L, ROWS, C)
    if name == "ops.quantize":
        kw = dict(_solve(V), **(dict(rows=(0, ROWS)) if entry == "vbq_quantize_rows_f32" else {}))
        second = lambda r: r[1]
        return Face(ops.quantize, kw, {
            "out_idx": Buf(lam, u16, "assign", lambda r: r, nothing=({}, lambda r: r)),
            "out_zhat": Buf(lam, f32, "assign", second, nothing=(dict(want_zhat=True), second)),
            "out_bits": Buf(lam, f32, "assign", second, nothing=(dict(want_bits=True), second)),
            "workspace": Buf((V["wsb"],), u8, "ws")})
    if name == "ops.level_counts":
        return Face(ops.level_counts, BASE["level_counts"](V), {
            "out": Buf((L, C, N + 1), i64, "add", lambda r: r, nothing=({}, lambda r: r)), "workspace": Buf((V["wsb"],), u8, "ws")})
    if name == "ops.code_lengths_from_counts":
        kw = dict(counts=V["level_counts"], lut=V["lut"], level_period=N + 1)
        return Face(ops.code_lengths_from_counts, kw, {
            "out_len": Buf((L, C, N + 1), f32, "assign", lambda r: r, nothing=({}, lambda r: r)),
            "out_model": Buf((L, C, N + 1), f32, "assign", lambda r: r[1], nothing=(dict(want_model=True), lambda r: r[1]))})
    if name == "ops.quantize_notebook":
        return Face(ops.quantize_notebook, BASE["quantize_notebook"](V), {
            "out_idx": Buf(lam, u16, "assign", lambda r: r[0], nothing=({}, lambda r: r[0]))})
    if name == "ops.histogram":
        kw = dict(BASE["histogram"](V), **(dict(rows=(0, ROWS)) if entry == "vbq_histogram_rows_u16" else {}))
        dt = i32 if entry == "vbq_histogram_u16_i32" else i64
        return Face(ops.histogram, kw, {"out": Buf((L, C, T), dt, "add", lambda r: r, nothing=(dict(dtype=dt), lambda r: r),
                                               also=(i32, i64))})
    if name == "ops.histogram_models":
        kw = dict(idx=V["idx"], n_ch=C, N=N, lut=V["lut"])
        return Face(ops.histogram_models, kw, {"counts": Buf((L, C, T), i32, "assign", lambda r: r[0], required=True, also=(i64,)),
                                               "models": Buf((L, C, T), f32, "assign", lambda r: r[1], required=True)})
    if name == "ops.moments":
        return Face(ops.moments, dict(x=V["mu"]), {"out": Buf((C, 2), f64, "add", lambda r: r, nothing=({}, lambda r: r))})
    if name == "ops.numpy_row_sums":
        x = V["models"]
        return Face(ops.numpy_row_sums, dict(x=x), {"workspace": Buf((h.vbq_numpy_row_sums_workspace_bytes(L, C * T),), u8, "ws")})
    if name == "ops.prep_planes":
        return Face(ops.prep_planes, BASE["prep_planes"](V), {
            "out_mu": Buf((C, ROWS), f32, "assign", lambda r: r[0], nothing=({}, lambda r: r[0])),
            "out_sigma": Buf((C, ROWS), f32, "assign", lambda r: r[1], nothing=({}, lambda r: r[1]))})
    if name == "ops.transpose":
        return Face(ops.transpose, dict(x=V["mu"]), {"out": Buf((C, ROWS), f32, "assign", lambda r: r, nothing=({}, lambda r: r))})
    if name == "ops.transpose_planes":
        return Face(ops.transpose_planes, dict(x=V["idx"]), {"out": Buf(lam, u16, "assign", lambda r: r, nothing=({}, lambda r: r))})
    if name == "ops.rd_sums":
        kw = dict(mu=V["mu_cb"], sigma=V["sigma_cb"], idx=V["idx"], tab_sorted=V["table_sorted"], n_ch=C, N=N, layout="cb", rate=V["models"])
        return Face(ops.rd_sums, kw, {"out": Buf((L, 2), f64, "add", lambda r: r, nothing=({}, lambda r: r))})
    if name in ("ops.bmshj_icdf_step", "ops.bmshj_icdf_chain"):
        params, xi, _ = _prior_case()
        chain = name.endswith("chain")
        flags = np.zeros((4, 2), np.uint32) if chain else np.array([0, 0x7f800000], np.uint32)
        state = {"left": Buf((ROWS, C), f32, "state", init=np.full((ROWS, C), -8.0)), "right": Buf((ROWS, C), f32, "state", init=np.full((ROWS, C), 8.0)),
                 "mid": Buf((ROWS, C), f32, "state"), "flags": Buf(flags.shape, u32, "state", init=flags)}
        kw = dict(params=params, xi=xi, **(dict(n_steps=3, tol=1e-9, first=True) if chain else {}))
        return Face(ops.bmshj_icdf_chain if chain else ops.bmshj_icdf_step, kw, state)
    if name == "ops.bmshj_nll_grad":
        params, _, x_cb = _prior_case()
        return Face(ops.bmshj_nll_grad, dict(params=params, x_cb=x_cb), {"out": Buf((C, 44), f64, "add", lambda r: r, nothing=({}, lambda r: r))})
    if name in ("ops.budget_dp", "ops.budget_dp_sweep"):
        fhat, K, budget, R, Nb = _budget(arg == "workspace")
        sweep = name.endswith("sweep")
        kw = dict(fhat=fhat, K=K, **(dict(budgets=[budget // 2, budget]) if sweep else dict(budget=budget)))
        wsb = h.vbq_budget_dp_workspace_bytes(R, K, Nb, budget)
        return Face(ops.budget_dp_sweep if sweep else ops.budget_dp, kw, {
            "status": Buf((1,), u32, "or"), "workspace": Buf((max(wsb, 16),), u8, "ws", short=False)})
    if name.startswith("ops.records_") or name in ("ops.topk", "ops.bag", "ops.scores"):
        r = _records()
        K, R = r["K"], r["R"]
        rec = dict(words=r["words"], K=K, N=N, total_bits=r["total"], table_sorted=r["table"])
        rows = rec if name.startswith("ops.records_") else dict(emb=r["emb"])
        if name == "ops.records_pack":
            idx = r["idx"].copy()
            idx[1, 2] = T + 9                                               # status bit 0: an index >= T
            return Face(ops.records_pack, dict(idx=_u16(idx), total_bits=r["total"], N=N), {
                "out": Buf((R, r["RW"]), u32, "assign", lambda x: x, nothing=({}, lambda x: x)), "status": Buf((1,), u32, "or")})
        if name == "ops.records_unpack":
            return Face(ops.records_unpack, dict(rec, row_ids=_t(np.array([0, R + 3, 2], np.int64))), {"status": Buf((1,), u32, "or")})
        if name in ("ops.records_topk", "ops.topk"):
            damaged = r["words"].clone()
            damaged[1] = 0xFFFFFFFF                                          # a record no packer writes: bits 0..2
            kw = dict(dict(rows, words=damaged) if "words" in rows else rows, queries=r["queries"], k=2)
            bufs = {"workspace": Buf((h.vbq_topk_workspace_bytes(R, K, 2, 2, 0),), u8, "ws")}
            if name == "ops.records_topk":
                bufs["status"] = Buf((1,), u32, "or")
            return Face(getattr(ops, name[4:]), kw, bufs)
        if name in ("ops.records_bag", "ops.bag"):
            kw = dict(rows, ids=_t(np.array([0, 3, R + 2, 1, 4], np.int64)), offsets=_t(np.array([0, 2, 5], np.int64)))
            return Face(getattr(ops, name[4:]), kw, {"out": Buf((2, K), f32, "assign", lambda x: x, nothing=({}, lambda x: x)),
                                                    "status": Buf((1,), u32, "or")})
        kw = dict(rows, queries=r["queries"], ids=_t(np.array([[0, R + 1, 2], [4, 4, 1]], np.int64)))
        return Face(getattr(ops, name[4:]), kw, {"out": Buf((2, 3), f32, "assign", lambda x: x, nothing=({}, lambda x: x)),
                                                "status": Buf((1,), u32, "or")})
    if name in ("ops.rans_decode_window", "ops.rans_map_decode_window"):
        k, files, segs, box, m, m_files, m_segs, m_box = _window()
        if name == "ops.rans_decode_window":
            kw = dict(payload=k.payload, sizes=k.sizes, offsets=k.offsets, files=_bad_file(files, 7, 99), segs=_t(segs), freq=k.d_freq,
                      values=k.d_values, box=box, seg=k.seg, N=k.bits)
        else:
            kw = dict(payload=m.payload, sizes=m.sizes, offsets=m.offsets, files=_bad_file(m_files, 8, 99), segs=_t(m_segs), freq=m.d_freq,
                      values=m.d_values, classes=_t(m.area_host), box=m_box, seg=m.seg, max_classes=m.max_P, N=m.bits)
        return Face(getattr(ops, name[4:]), kw, {"out": Buf((3,) + tuple(kw["box"]) + (8,), f32, "keep", lambda r: r[0]),
                                                "status": Buf((3,), u32, "or", lambda r: r[1], nothing=({}, lambda r: r[1]))})
    if name == "ops.rans_encode_files":
        import test_gpu_encode_files as EF
        rows, tables, n_tables, C_, seg, nbits, _ = EF.KERNEL_CASES["rows-and-tables"]
        k = _once("EF", lambda: EF.Batch(rows, tables, n_tables, C_, seg, nbits, seed=3, tight=True))
        F, M = len(rows), k.plan.M
        kw = dict(idx=k.d_idx, files=_bad_file(k.files, 2), items=_t(k.plan.items), freq=k.d_freq, M=M, seg=seg, N=nbits)
        return Face(ops.rans_encode_files, kw, {"words": Buf((M, seg + 2), u16, "keep", lambda r: r[0]),
                                                "sizes": Buf((M,), u32, "keep", lambda r: r[1]),
                                                "status": Buf((F,), u32, "or", lambda r: r[2], nothing=({}, lambda r: r[2]))})
    if name == "ops.rans_sizes_files":
        import test_gpu_budget_batch as BB
        rows, L_, C_, seg, nbits, _ = BB.KERNEL_CASES["rows-and-lambdas"]
        k = _once("BB", lambda: BB.Batch(rows, L_, C_, seg, nbits, seed=4, tight=True))
        items = np.concatenate([k.plan.items, np.full((-k.plan.items.shape[0] % 64, 2), -1, np.int32)])
        F = len(rows)
        kw = dict(idx=k.d_idx, files=_bad_file(k.files, 2), items=_t(items), freq=k.d_freq, lambda_stride=k.stride_l, seg=seg, N=nbits)
        return Face(ops.rans_sizes_files, kw, {"totals": Buf((L_, F), u64, "add", lambda r: r[0], nothing=({}, lambda r: r[0])),
                                               "status": Buf((F,), u32, "or", lambda r: r[1], nothing=({}, lambda r: r[1]))})
    if name in ("ops.rans_map_encode_files", "ops.rans_map_sizes_files"):
        import test_gpu_mapped_batch as MB
        k = _once("MB", lambda: MB.fitted_batch(**MB.MIXED, bits=10, seed=11, round_=1, tight=True))
        M, F = k.plan.M, len(k.rows)
        kw = dict(idx=k.d_idx, classes=k.d_cls, files=_bad_file(k.files, 3), palettes=_t(k.pal_rows), items=_t(k.plan.items), freq=k.d_freq,
                  M=M, seg=k.seg, max_classes=k.max_classes, N=k.bits)
        if name == "ops.rans_map_encode_files":
            return Face(ops.rans_map_encode_files, kw, {"words": Buf((M, k.seg + 2), u16, "keep", lambda r: r[0]),
                                                        "sizes": Buf((M,), u32, "keep", lambda r: r[1]),
                                                        "status": Buf((F,), u32, "or", lambda r: r[2], nothing=({}, lambda r: r[2]))})
        return Face(ops.rans_map_sizes_files, kw, {"sizes": Buf((M,), u32, "keep", lambda r: r[0]),
                                                   "status": Buf((F,), u32, "or", lambda r: r[1], nothing=({}, lambda r: r[1]))})
    if name == "ops.rans_map_rates_files":
        import test_gpu_mapped_budget as MG
        r = _once("MG", lambda: MG.fitted(MG.SIX[2], 5, seed=21, tight=True))
        K_, F = len(r.cands), len(r.rows)
        kw = dict(idx=r.d_idx, classes=r.d_cls, files=_bad_file(r.files, 3), palettes=_t(r.rows4()), items=_t(r.plan.items), freq=r.d_freq,
                  lambda_stride=r.stride_l, seg=r.seg, max_classes=2, N=r.bits)
        return Face(ops.rans_map_rates_files, kw, {"totals": Buf((K_, F), u64, "add", lambda x: x[0], nothing=({}, lambda x: x[0])),
                                                   "status": Buf((F,), u32, "or", lambda x: x[1], nothing=({}, lambda x: x[1]))})
    if name in ("ops.rans_il_sizes_files", "ops.rans_il_encode_files", "ops.rans_il_decode_files"):
        import test_gpu_compact_files as CF
        b = _once("CF", lambda: CF.Batch(*CF._three(10), 10))
        files, items, freq = _bad_file(b.files, 2), _t(b.items), _t(b.freq)
        st = Buf((b.F,), u32, "or", lambda r: r[1], nothing=({}, lambda r: r[1]))
        if name == "ops.rans_il_sizes_files":
            kw = dict(idx=_t(b.matrix.reshape(-1)), files=files, items=items, freq=freq, P_all=b.P_all, N=b.N)
            return Face(ops.rans_il_sizes_files, kw, {"sizes": Buf((b.P_all,), u32, "keep", lambda r: r[0]), "status": st})
        if name == "ops.rans_il_encode_files":
            kw = dict(idx=_t(b.matrix.reshape(-1)), files=files, items=items, freq=freq, sizes=_t(b.sizes), offsets=_t(b.offsets), N=b.N)
            return Face(ops.rans_il_encode_files, kw, {"payload": Buf((b.payload.size,), u16, "keep", lambda r: r[0], required=True, short=False),
                                                       "status": st})
        kw = dict(payload=_t(b.payload), sizes=_t(b.sizes), offsets=_t(b.offsets), files=files, items=items, freq=freq, N=b.N)
        return Face(ops.rans_il_decode_files, kw, {"idx": Buf((b.C * b.W,), u16, "keep", lambda r: r[0], required=True, short=False),
                                                   "status": st})
    if name == "ops.rans_il_rates_files":
        import test_gpu_compact_rates_files as CR
        r = _once("CR", lambda: CR.Planes(*CR._fitted(10), 10))
        kw = dict(idx=_t(r.array), files=_bad_file(r.files, 2), items=_t(r.items), freq=_t(r.freq), P_all=r.P_all, lambda_stride=r.stride, N=r.N)
        return Face(ops.rans_il_rates_files, kw, {"sizes": Buf((CR.L_, r.P_all), u32, "keep", lambda x: x[0]),
                                                  "status": Buf((r.F,), u32, "or", lambda x: x[1], nothing=({}, lambda x: x[1]))})
    if name == "ops.compress_latents":
        return Face(ops.compress_latents, BASE["compress_latents"](V), {"workspace": Buf((V["wsb_latents"],), u8, "ws")})
    if name in ("kmeans1d.kmeans1d_dp", "kmeans1d.nearest_code_channels"):
        def make():
            rng = np.random.default_rng(3)
            x = rng.standard_normal((16, C)).astype(np.float32)
            _, shift, S1, S2 = kmeans1d.prefix_sums(_t(x))
            S1 = S1.clone()
            S1[0, -1] = float("nan")                                        # channel 0: status bit 0
            return _t(x), shift, S1, S2, _t(np.sort(rng.standard_normal((C, 3)), axis=1))
        x, shift, S1, S2, codes = _once("kmeans", make)
        if name == "kmeans1d.kmeans1d_dp":
            wsb = _lib_kmeans.lib().vbqk_kmeans1d_workspace_bytes(16, C, 3)
            return Face(kmeans1d.kmeans1d_dp, dict(S1=S1, S2=S2, shift=shift, levels=[2, 3]),
                        {"status": Buf((1,), u32, "or"), "workspace": Buf((wsb,), u8, "ws", short=False)})
        return Face(kmeans1d.nearest_code_channels, dict(x=x, codes=codes), {"counts": Buf((C, 3), i64, "add")})
    if name == "coder.RansCodec.unpack_device":
        codec, payload, sizes = _codec_case()
        return Face(codec.unpack_device, dict(payload=payload, sizes=sizes, n=70), {
            "status": Buf((1,), u32, "or", lambda r: r[2], nothing=({}, lambda r: r[2]))})
    if name == "store.plan_boxes":
        import store_reference as SR
        import test_gpu_store as TS
        rng = np.random.default_rng(2)
        table = SR.synthetic_table(TS.K_DIMS, 8, 64, rng)
        box = (1, 2, 5)
        ids, origins = SR.random_samples(TS.K_DIMS, box, 3, rng)
        ids[1] = len(TS.K_DIMS) + 2                                         # sample 1: no such file, bit 7
        n_sel = max(SR.max_listed_segments(d, box, 64) for d in TS.K_DIMS)
        kw = dict(table=_t(table), ids=_t(ids), origins=_t(origins), extents=box, seg=64, n_sel=n_sel)
        return Face(store.plan_boxes, kw, {"desc": Buf((3, 8), i64, "assign", lambda r: r[0], nothing=({}, lambda r: r[0])),
                                           "segs": Buf((3, n_sel), i32, "assign", lambda r: r[1], nothing=({}, lambda r: r[1])),
                                           "status": Buf((3,), u32, "or", lambda r: r[2], nothing=({}, lambda r: r[2]))})
    if name == "dist.CountsAllReduce.start":
        red = _reducer()

        def reduce(counts, words):                                          # `words`: the reducer's own scratch, laid where the case wants it
            red.words = words
            red.start(counts).wait()
            return red._counts                                              # what wait() unpacked into
        kw = dict(words=torch.zeros(red.nw + 1, dtype=i64, device=DEV))
        return Face(reduce, kw, {"counts": Buf((6,), i32, "state", lambda r: r, init=np.array([3, 0, 7, 400, 1, 9]), short=True)},
                    scratch=("words",))
    if name == "store.LatentStore.crops":
        st, C32 = _store(entry == "vbq_rans_map_decode_window_f32")
        kw = dict(ids=_t(np.array([0, 7, 2], np.int64)), origins=_t(np.array([[0, 1, 2], [0, 0, 0], [0, 3, 4]], np.int64)), extents=(1, 3, 5))
        return Face(st.crops, kw, {"out": Buf((3, 1, 3, 5, C32), f32, "keep", lambda r: r[0]),
                                   "status": Buf((3,), u32, "or", lambda r: r[1], nothing=({}, lambda r: r[1]))})
    raise AssertionError(f"no arguments for {name}: a new ARG row needs its smallest valid set here")


ROWS_ = [pytest.param(e, p, f, a, id=f"{f}-{a}-{e}") for e, p, f, a, via in WB.arg_rows()
         if via != "store.plan_boxes:status"]
"""(LatentStore.crops hands its one status to vbqs_plan_boxes and to the decoder in the same call: its two decoder rows, on a plain
and on a mixed store, are that call.)"""


# ------------------------------------------------------------------------------------------------------------------ refused
def _defects(buf, one_word):
    """name -> (tensor to hand in, the tensor that owns its memory)."""
    shape, dt = buf.shape, buf.dtype
    out = {}

    def own(t):
        return t, t
    small, large = SMALLER[dt], LARGER[dt]
    small, large = (SMALLER[small] if small in buf.also else small), (LARGER[large] if large in buf.also else large)
    out["smaller dtype"] = own(torch.zeros(shape, dtype=small, device=DEV))
    out["larger dtype"] = own(torch.zeros(shape, dtype=large, device=DEV))
    if buf.short:
        n = int(np.prod(shape))
        out["one element short"] = own(torch.zeros(max(n - 1, 0), dtype=dt, device=DEV))
        if buf.kind != "ws":
            out["one dimension off"] = own(torch.zeros(shape[:-1] + (shape[-1] + 1,), dtype=dt, device=DEV))
    out["on the host"] = own(torch.zeros(shape, dtype=dt))
    wide = torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=dt, device=DEV)
    out["every second element"] = (wide[..., ::2], wide)
    one = torch.zeros(1, dtype=dt, device=DEV)
    if int(np.prod(shape)) > 1:                                             # (one element expanded to one element is itself)
        out["stride 0"] = (one.expand(shape), one)
    if one_word:
        out["empty"] = own(torch.zeros(0, dtype=dt, device=DEV))
    return out


@pytest.mark.parametrize("entry,param,name,arg", ROWS_)
def test_a_defective_buffer_is_refused_before_the_library(monkeypatch, V, entry, param, name, arg):
    from vbq_amd._lib import VBQError
    fc = face(name, entry, arg, V)
    buf = fc.buffers[arg]
    before = {k: bits(v) for k, v in fc.inputs(scratch=False).items()}
    _stand_in(monkeypatch)
    defects = _defects(buf, one_word=buf.shape == (1,) and buf.kind == "or")
    assert {"smaller dtype", "larger dtype", "on the host", "every second element"} <= set(defects)
    for what, (given, owner) in defects.items():
        owner.view(torch.uint8).fill_(0xA5) if owner.numel() else None
        with pytest.raises((ValueError, VBQError)) as e:
            fc.run({arg: given})
        assert type(e.value) in (ValueError, VBQError), (what, e.value)
        assert "was reached" not in str(e.value)
        assert bool((owner.view(torch.uint8) == 0xA5).all()), f"{name}({arg}) {what}: the refused buffer was written"
    for k, v in fc.inputs(scratch=False).items():
        assert np.array_equal(bits(v), before[k]), f"{name}: input {k} changed"


# ------------------------------------------------------------------------------------------------------------------ written
def _tensors(ret):
    if isinstance(ret, torch.Tensor):
        return [ret]
    if isinstance(ret, (tuple, list)):
        return [t for r in ret for t in _tensors(r)]
    return []


def _expect(fc, arg, kwargs=None):
    """-> check(first, second): given the buffer's bits after a call that started from pattern(buf) and after one that started
    from pattern(buf, other=True), assert what the row's kind says, against a call into a plain new tensor."""
    buf = fc.buffers[arg]
    npd = np.dtype(FP._NP[buf.dtype])
    plain = dev(buf.start())
    ret = fc.run({arg: plain} if buf.kind != "ws" else {}, kwargs)
    base = bits(plain)
    outputs = [bits(t) for t in _tensors(ret)]
    if buf.nothing is not None:                                              # the call's own tensor, when it is given none
        extra, pick = buf.nothing
        own = pick(fc.run({}, kwargs, extra))
        if buf.kind != "keep":
            assert np.array_equal(bits(own), base), f"{arg}: a plain given tensor and the call's own differ"

    def check(first, second, ret_first, what):
        u = UINT[npd.itemsize]
        p, q = pattern(buf), pattern(buf, other=True)
        if buf.kind in ("assign", "state"):
            assert np.array_equal(first, base), f"{what}: content differs from a plain tensor's"
        elif buf.kind == "add":
            for got, start in ((first, p), (second, q)):
                assert np.array_equal(got, (start + base.view(npd)).view(u)), f"{what}: not earlier content + what the call adds"
        elif buf.kind == "or":
            assert base.any(), f"{what}: the case sets no status bit: it cannot tell a copy from the caller's tensor"
            for got, start in ((first, p), (second, q)):
                assert np.array_equal(got, start.view(u) | base), f"{what}: not earlier content | what the call sets"
        elif buf.kind == "keep":
            kept = first != second
            assert kept.any() and not kept.all(), f"{what}: the case keeps nothing, or everything"
            assert np.array_equal(first[kept], p.view(u)[kept]) and np.array_equal(second[kept], q.view(u)[kept]), f"{what}: kept slots changed"
            assert np.array_equal(first[~kept], base[~kept]), f"{what}: written slots differ from a plain tensor's"
        else:                                                                # a workspace: the call's results are the check
            got = [bits(t) for t in _tensors(ret_first)]
            assert len(got) == len(outputs) and all(np.array_equal(a, b) for a, b in zip(got, outputs)), f"{what}: results differ"
    return check


def _placed(buf, off):
    if buf.kind == "ws":
        return FP.guarded_workspace(buf.nbytes, DEV)
    return FP.Guarded(buf.shape, buf.dtype, DEV, off)


@pytest.mark.parametrize("entry,param,name,arg", ROWS_)
def test_a_valid_buffer_is_written_where_it_was_given(V, entry, param, name, arg):
    fc = face(name, entry, arg, V)
    buf = fc.buffers[arg]
    before = {k: bits(v) for k, v in fc.inputs(scratch=False).items()}
    check = _expect(fc, arg)
    for off in ((0,) if buf.kind == "ws" else (0, 1)):
        got, rets = [], []
        for other in (False, True):
            g = _placed(buf, off)
            if buf.kind in ("add", "or", "keep"):
                g.fill(pattern(buf, other))
            elif buf.kind == "state" or buf.init is not None:
                g.fill(buf.start())
            ret = fc.run({arg: g.view})
            if buf.pick is not None:
                back = buf.pick(ret)
                assert back is g.view or (back.data_ptr() == g.ptr and tuple(back.shape) == buf.shape), f"{name}({arg}): not the tensor given"
            g.assert_outside_intact(f"{name}({arg}) offset {off}")
            got.append(g.bits()), rets.append(ret)
        check(got[0], got[1], rets[0], f"{name}({arg}) offset {off}")
    for k, v in fc.inputs(scratch=False).items():
        assert np.array_equal(bits(v), before[k]), f"{name}: input {k} changed"


# ------------------------------------------------------------------------------------------------------------------ overlap
def _arena(x, buf, where):
    """One allocation that holds a copy of the tensor x and a view of the buffer's shape and dtype laid `where` relative to it
    -> (the copy of x, the buffer view).  "behind": the buffer starts 256-byte aligned at the copy's last byte + 1; otherwise the
    copy starts 256-byte aligned."""
    e, nb, nx = buf.itemsize, buf.nbytes, x.numel() * x.element_size()
    room = -(-(max(nb, nx) + 256) // 256) * 256
    raw = torch.zeros(3 * room + 512, dtype=torch.uint8, device=DEV)
    mark = room + (-(raw.data_ptr() + room)) % 256                          # a 256-byte aligned address with `room` before it
    a = mark - nx if where == "behind" else mark
    start = {"over": a, "its first bytes": a - nb + e, "its last element": a + (nx - 1) // e * e, "behind": mark}[where]
    assert start % e == 0 and start >= 0 and a >= 0 and (raw.data_ptr() + a) % x.element_size() == 0
    copy = raw[a:a + nx].view(x.dtype).view(x.shape)
    copy.copy_(x)
    return copy, raw[start:start + nb].view(buf.dtype).view(buf.shape)


@pytest.mark.parametrize("entry,param,name,arg", ROWS_)
def test_a_buffer_that_overlaps_anything_else_is_refused(monkeypatch, V, entry, param, name, arg):
    fc = face(name, entry, arg, V)
    buf = fc.buffers[arg]
    _stand_in(monkeypatch)
    tried = 0
    for k, x in fc.inputs().items():
        if x.numel() == 0 or not x.is_contiguous():
            continue
        for where in ("over", "its first bytes", "its last element"):
            copy, given = _arena(x, buf, where)
            with pytest.raises(ValueError, match=rf"^{arg} overlaps \w+: a tensor the call writes must share no memory") as e:
                fc.run({arg: given}, dict(fc.kwargs, **{k: copy}))
            assert "was reached" not in str(e.value)
            tried += 1
    assert tried >= 3, f"{name}: no input to overlap"
    for other, b2 in fc.buffers.items():                                     # two written buffers over each other
        if other == arg:
            continue
        raw = torch.zeros(max(buf.nbytes, b2.nbytes) + 512, dtype=torch.uint8, device=DEV)
        a = (-raw.data_ptr()) % 256
        mine, theirs = raw[a:a + buf.nbytes].view(buf.dtype).view(buf.shape), raw[a:a + b2.nbytes].view(b2.dtype).view(b2.shape)
        with pytest.raises(ValueError, match=rf"^({arg} overlaps {other}|{other} overlaps {arg}): ") as e:
            fc.run({arg: mine, other: theirs})
        assert "was reached" not in str(e.value)


@pytest.mark.parametrize("entry,param,name,arg", ROWS_)
def test_a_buffer_directly_behind_an_input_is_accepted_and_right(V, entry, param, name, arg):
    """The control for the interval arithmetic, on the real library: the ranges touch and do not intersect."""
    fc = face(name, entry, arg, V)
    buf = fc.buffers[arg]
    k = next(k for k, x in fc.inputs().items() if x.numel() and x.is_contiguous())
    got, rets = [], []
    for other in (False, True):
        copy, given = _arena(fc.kwargs[k], buf, "behind")
        assert given.data_ptr() == copy.data_ptr() + copy.numel() * copy.element_size()
        if buf.kind in ("add", "or", "keep"):
            given.copy_(dev(pattern(buf, other)))
        else:
            given.copy_(dev(buf.start()))
        kwargs = dict(fc.kwargs, **{k: copy})
        rets.append(fc.run({arg: given}, kwargs))
        got.append(bits(given))
        assert k in fc.scratch or np.array_equal(bits(copy), bits(fc.kwargs[k])), f"{name}: the input before the buffer changed"
    _expect(fc, arg)(got[0], got[1], rets[0], f"{name}({arg}) behind {k}")
