"""ChannelwisePriorCDFQuantizer with the reference's call surface
(img-compression/quantizer.py:13-256), running on the HIP kernels.

Same constructor, method names, argument meaning, returned dict layout and state attributes
as the reference class, so `post_process.build_cdf_qzer` / `utils.evaluate_compression_quantizer`
(post_process.py:99-107, utils.py:542-554) can use it unchanged.  What differs is inside:

* the whole of get_all_N_bit_intervals -> candidate assembly -> batch_quantize_indep_dims ->
  qidx lookup (quantizer.py:65-80, 156-188, 135/223) is ONE kernel launch (K1) for all lambdas;
* per-channel bincounts (quantizer.py:104-105, 138-140) are one histogram launch (K2);
* latents live on the GPU as channel-major planes [C, B]: every workgroup then works on one
  channel -> one 8 KB code-point table in LDS and wave-uniform penalties.

Arrays may be NumPy arrays or torch tensors; results are NumPy arrays (as in the reference,
whose np.reshape moves everything to the host, quantizer.py:237) unless `return_np=False`.
There is no CPU path: without the HIP extension and a ROCm device the methods raise.
"""
from __future__ import annotations

from collections import namedtuple
from collections.abc import MutableMapping
from typing import Dict, Optional

import numpy as np
import torch

from . import bitstream
from . import entropy as _entropy
from . import ops
from .tables import n_bit_binary_floats


RATE_SCRATCH_BYTES = 1 << 30                 # the batch rate calls: the u16 indices of one chunk of lambdas stay below this


def _to_numpy(a):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().numpy()
    if hasattr(a, "numpy") and not isinstance(a, np.ndarray):      # e.g. a TF eager tensor
        return np.asarray(a.numpy())
    return np.asarray(a)


# What the two latent files (vbq_amd.bitstream) do their own way.  `unit` is the segment / part length of the file; idx is u16
# [C, B] (`encode`) or [L, C, B] (`words`); buf (`decode`) is the file from its sizes on, as u16 on the device.
_Layout = namedtuple("_Layout", "unit header write nbytes check segment encode words decode")
_LAYOUTS = {
    "segments": _Layout(
        "segment", bitstream.Header, bitstream.write, bitstream.latent_nbytes, bitstream.check_segment,
        segment=lambda unit: unit,                               # of the codec
        encode=lambda codec, idx, unit: codec.encode_packed(idx),
        # payload words per lambda, on the device: ONE sizes launch over the L x C streams
        words=lambda q, keys, idx, unit: q._coder_stack(keys, unit).sizes(idx).view(torch.int32).view(len(keys), -1)
                                          .sum(dim=1, dtype=torch.int64),
        decode=lambda codec, buf, h: codec.decode_packed(buf[h.n_sizes:], buf[: h.n_sizes], h.n_rows)),
    "interleaved": _Layout(
        "part", bitstream.CompactHeader, bitstream.write_compact, bitstream.compact_nbytes, bitstream.check_part,
        segment=lambda unit: None,                               # the interleaved coder has no segments
        encode=lambda codec, idx, unit: codec.encode_interleaved(idx, unit),
        # one sizes launch per lambda: a part never holds symbols of two lambdas
        words=lambda q, keys, idx, unit: torch.stack([
            q._coder_tables(k)[0].sizes_interleaved(idx[l], unit).view(torch.int32).sum(dtype=torch.int64) for l, k in enumerate(keys)]),
        decode=lambda codec, buf, h: codec.decode_interleaved(buf[h.sizes_nbytes // 2:], buf[: 2 * h.n_parts].view(torch.uint32),
                                                              h.n_rows, h.part)),    # (the header is a multiple of 8 bytes)
}


class DeviceModels(MutableMapping):
    """dict[lamb] -> NumPy array [C, K] whose rows live ON THE DEVICE until somebody reads them on the host.

    build_entropy_models leaves its three tables -- entropy_models, raw_code_length_entropy_models and the integer
    histograms behind them -- where the kernels wrote them: compress_latents reads them there, and the 67 MB of models plus
    the counts (Kodak-24, C = 256, 32 lambdas) cross PCIe only if a caller actually looks at them (`models[lamb]`, iteration
    over values / items, pickling, `save`).  The first host read copies the whole stack once and runs the build's deferred
    checks (EntropyModelBuild.check: histogram totals, host stages); the arrays are read-only, as the eager ones were (an
    in-place edit would leave the device copy stale).  Assigning `models[lamb] = array` works as on a dict; the device
    stack is then no longer used for the lookups (`device_rows` returns None and the caller rebuilds its copy)."""

    def __init__(self, keys, stack: torch.Tensor, companions=None, on_read=None):
        self._keys = list(keys)
        self._index = {k: i for i, k in enumerate(self._keys)}
        self._stack = stack
        self._companions = dict(companions or {})
        self._on_read = on_read
        self._host = None
        self._over = {}                      # entries the caller replaced or added
        self._gone = set()
        self._subsets = {}                   # device rows of key subsets already gathered (an evaluation loop asks again and again)

    @property
    def on_device(self) -> bool:
        """True while no host copy has been made."""
        return self._host is None

    def _materialise(self):
        if self._host is None:
            if self._on_read is not None:
                self._on_read()
            h = self._stack.cpu().numpy()
            h.setflags(write=False)
            self._host = h
            # ONE view object per key, made once: callers that key caches on the arrays' identities (_keyed_dev) see the same
            # object on every read instead of a fresh view per __getitem__ (which re-uploaded the whole table per image)
            self._rows = [h[i] for i in range(h.shape[0])]
        return self._host

    def __getitem__(self, k):
        if k in self._over:
            return self._over[k]
        if k in self._gone:
            raise KeyError(k)
        i = self._index[k]                   # KeyError as a dict
        self._materialise()
        return self._rows[i]

    def __setitem__(self, k, v):
        self._over[k] = v
        self._gone.discard(k)
        self._subsets.clear()

    def __delitem__(self, k):
        self._subsets.clear()
        if k in self._over:
            del self._over[k]
            if k in self._index:
                self._gone.add(k)
        elif k in self._index and k not in self._gone:
            self._gone.add(k)
        else:
            raise KeyError(k)

    def __iter__(self):
        for k in self._keys:
            if k not in self._gone:
                yield k
        for k in self._over:
            if k not in self._index:
                yield k

    def __len__(self):
        return len(self._keys) - len(self._gone) + sum(1 for k in self._over if k not in self._index)

    def __contains__(self, k):
        return k in self._over or (k in self._index and k not in self._gone)

    def device_rows(self, keys, companion=None):
        """The rows of `keys` as a device tensor [len(keys), C, K] (of the companion stack when named), or None when an
        entry was replaced by the caller (the device stack no longer tells the whole story).  KeyError for unknown keys."""
        keys = list(keys)
        for k in keys:
            if k not in self:
                raise KeyError(k)
        if any(k in self._over for k in keys):
            return None
        t = self._stack if companion is None else self._companions[companion]
        if keys == self._keys:
            return t
        which = (companion, tuple(self._index[k] for k in keys))
        sub = self._subsets.get(which)
        if sub is None:
            if len(self._subsets) > 8:
                self._subsets.clear()
            sub = self._subsets[which] = t[list(which[1])].contiguous()
        return sub

    def to_dict(self):
        return {k: self[k] for k in self}

    def __reduce__(self):                    # pickles as the plain dict of NumPy arrays it stands for
        return (dict, (self.to_dict(),))

    def __repr__(self):
        return f"DeviceModels({len(self)} lambdas, {'device-resident' if self.on_device else 'host copy made'})"


class ChannelwisePriorCDFQuantizer:
    """The reference's quantizer (quantizer.py) on HIP kernels: code points from a prior, entropy models fitted on latents,
    compression of latents and images to arrays, byte strings and files.

    A public call that raises leaves the quantizer answering every later call exactly as it did before the failed one: the
    transitions (build_code_points, build_entropy_models*, load) compute into locals and assign their state only once every
    step has succeeded, and a refused probe changes no table, model or cache entry another call's answer depends on."""

    def __init__(self, num_channels, max_bits_per_coord, float_type="float32", int_type="int32", device=None,
                 validate_inputs=False):
        if float_type != "float32":
            raise ValueError("only float_type='float32' is supported (the reference default, quantizer.py:14)")
        self.max_bits_per_coord = int(max_bits_per_coord)
        self.num_channels = int(num_channels)
        self.float_type = float_type
        self.int_type = int_type
        self.quantization_levels = 2 ** (self.max_bits_per_coord + 1) - 1          # quantizer.py:20
        self.raw_code_length_entropy_models = None
        self.entropy_models = None
        self.process_group = None          # set to a torch.distributed group to all-reduce the histograms
        self._device = device
        # True: every batch is checked on the device for NaN / infinite means and non-positive / non-finite standard
        # deviations before it is solved (ValueError; costs one synchronisation per call).  The reference has no such
        # check -- NaNs flow through tf.argmax there -- so it is off by default.
        self.validate_inputs = bool(validate_inputs)
        self._dev_cache: Dict[str, torch.Tensor] = {}

    # ------------------------------------------------------------------ state / pickling
    def __getstate__(self):
        st = dict(self.__dict__)
        st["_dev_cache"] = {}
        st["_device"] = None
        st["process_group"] = None
        for k, v in list(st.items()):          # device-resident tables travel as the dicts of NumPy arrays they stand for
            if isinstance(v, DeviceModels):
                st[k] = v.to_dict()
        return st

    def __setstate__(self, st):
        self.__dict__.update(st)
        self._dev_cache = {}

    # ------------------------------------------------------------------ on-disk format
    def save(self, path):
        """Portable alternative to the reference's pickle (post_process.py:106-107): one .npz holding the
        code-point table, the two entropy-model dicts (keys = lambdas as float64) and the histograms."""
        if not hasattr(self, "all_code_points"):
            raise ValueError("nothing to save: build_code_points() first")
        d = dict(format=np.array("vbq_amd.quantizer/1"), num_channels=self.num_channels,
                 max_bits_per_coord=self.max_bits_per_coord, all_code_points=self.all_code_points)
        if self.entropy_models:
            lambs = self.lambs
            d["lambdas"] = np.array([float(l) for l in lambs], dtype=np.float64)
            d["entropy_models"] = np.stack([self.entropy_models[l] for l in lambs])
            if self.raw_code_length_entropy_models:
                d["raw_code_length_entropy_models"] = np.stack([self.raw_code_length_entropy_models[l] for l in lambs])
            if hasattr(self, "_code_counts"):
                d["code_counts"] = np.stack([self._code_counts[l] for l in lambs])
                d["add_n_smoothing"] = np.array(self._add_n_smoothing)
        np.savez_compressed(path, **d)

    @classmethod
    def load(cls, path, device=None):
        z = np.load(path, allow_pickle=False)
        if str(z["format"]) != "vbq_amd.quantizer/1":
            raise ValueError(f"{path}: unknown format {z['format']}")
        q = cls(int(z["num_channels"]), int(z["max_bits_per_coord"]), device=device)

        class _Table:
            def __init__(self, pts):
                self.pts = pts

            def inverse_cdf(self, xi):
                return self.pts
        q.build_code_points(_Table(np.ascontiguousarray(z["all_code_points"].T)))
        if "lambdas" in z:
            lambs = [float(v) for v in z["lambdas"]]
            q.entropy_models = {l: z["entropy_models"][i] for i, l in enumerate(lambs)}
            if "raw_code_length_entropy_models" in z:
                q.raw_code_length_entropy_models = {l: z["raw_code_length_entropy_models"][i] for i, l in enumerate(lambs)}
            if "code_counts" in z:
                q._code_counts = {l: z["code_counts"][i] for i, l in enumerate(lambs)}
                q._add_n_smoothing = z["add_n_smoothing"].item()
        return q

    @property
    def device(self):
        if self._device is None:
            self._device = ops.current_device("the VBQ quantizer")
        return self._device

    def _dev(self, name: str, builder):
        t = self._dev_cache.get(name)
        if t is None or t.device != self.device:
            t = builder().to(self.device)
            self._dev_cache[name] = t
        return t

    # ------------------------------------------------------------------ tables (quantizer.py:25-63)
    def build_code_points(self, prior_model, **kwargs):
        N, C = self.max_bits_per_coord, self.num_channels
        all_bin_floats = np.hstack([n_bit_binary_floats(n) for n in range(N + 1)])
        all_bin_floats_rep = np.repeat(all_bin_floats[:, None], C, axis=1)          # T x C
        pts = _to_numpy(prior_model.inverse_cdf(all_bin_floats_rep, **kwargs))
        if pts.shape != (self.quantization_levels, C):
            raise ValueError(f"prior.inverse_cdf returned shape {pts.shape}, expected {(self.quantization_levels, C)}")
        # everything is computed into locals and checked first: a prior that is refused leaves the quantizer as it was
        all_code_points = np.ascontiguousarray(pts.astype(np.float32).T)            # C x T, level-major
        code_points_by_channel = np.sort(all_code_points, axis=1)                   # MUST BE SORTED (:37)
        code_points_by_bits = [[all_code_points[c, 2 ** n - 1: 2 ** (n + 1) - 1] for n in range(N + 1)] for c in range(C)]
        grids = np.empty((C, N + 1, 2 ** N), dtype=np.float32)
        for c in range(C):
            for n in range(N + 1):
                lvl = code_points_by_bits[c][n]
                pad = 2 ** (N - 1) - 1 if n == 0 else 2 ** (N - 1) - 2 ** (n - 1)
                grids[c, n] = np.pad(np.array([lvl[0]] * 2) if n == 0 else lvl, (pad,), "edge")
        # The kernels need the merged table to be non-decreasing in xi (then rank order == sorted order).
        from .tables import rank_of_slot
        in_rank_order = np.empty_like(all_code_points)
        in_rank_order[:, rank_of_slot(N)] = all_code_points
        if not np.all(np.diff(in_rank_order, axis=1) >= 0):
            raise ValueError("prior.inverse_cdf is not monotone in xi after the float32 cast; the reference's "
                             "per-level searchsorted (quantizer.py:74) is undefined on such tables")
        strict = bool(np.all(np.diff(in_rank_order, axis=1) > 0))
        # canonical index of quantizer.py:135/223: first sorted position holding the same value
        canon = (np.stack([np.searchsorted(r, r, side="left") for r in in_rank_order]).astype(np.int64)
                 if not strict else None)
        self.all_code_points, self.code_points_by_channel, self.code_points_by_bits = all_code_points, code_points_by_channel, code_points_by_bits
        self._search_grids, self._strict, self._canon = grids, strict, canon
        self._dev_cache = {}

    def _table_dev(self):
        return self._dev("table_lm", lambda: torch.from_numpy(self.all_code_points))

    def _sorted_dev(self):
        return self._dev("sorted", lambda: torch.from_numpy(self.code_points_by_channel))

    # ------------------------------------------------------------------ compat helper (quantizer.py:65-80)
    def get_all_N_bit_intervals(self, Z):
        """Left/right n-bit neighbours, C x (N+1) x B (device tensors).  Kept for API compatibility only: the
        solve below never materialises these tensors (vbq_n_bit_intervals_f32)."""
        from . import _lib
        Zt = torch.as_tensor(_to_numpy(Z) if not isinstance(Z, torch.Tensor) else Z, dtype=torch.float32).to(self.device)
        if Zt.dim() != 2 or Zt.shape[1] != self.num_channels:
            raise ValueError(f"expected Z of shape [B, {self.num_channels}], got {tuple(Zt.shape)}")
        z_cb = ops.transpose(Zt.contiguous())                                       # [C, B] (quantizer.py:73)
        C, B, N = self.num_channels, Zt.shape[0], self.max_bits_per_coord
        left = torch.empty((C, N + 1, B), dtype=torch.float32, device=self.device)
        right = torch.empty_like(left)
        _lib.check(_lib.lib().vbq_n_bit_intervals_f32(ops._ptr(z_cb), B, C, ops._ptr(self._table_dev()), N, ops._ptr(left),
                                                      ops._ptr(right), ops._stream(z_cb)), "vbq_n_bit_intervals_f32")
        return left, right

    # ------------------------------------------------------------------ the solve
    def _prep(self, batch_means, batch_spread, spread="sigma"):
        """Channel-major planes [C, B] of the means and the standard deviations, both in one launch; `spread` says what
        batch_spread holds ('sigma', or 'logvar': sigma = exp(.) ** 0.5 is taken on the way, quantizer.py:87,92)."""
        mu, sp = self._batch_dev(batch_means, batch_spread)
        if getattr(self, "validate_inputs", False):
            ops.check_inputs(mu.contiguous(), (sp if spread == "sigma" else torch.exp(sp) ** 0.5).contiguous())
        return ops.prep_planes(mu, sp, spread=spread)

    def _keyed_dev(self, name: str, arrays, builder):
        """Device copy of a table assembled from per-lambda model arrays, rebuilt only when one of those arrays is
        replaced.  Keyed on the arrays' identities; the cache entry holds the arrays, so an id cannot be reused by a
        new object while the entry lives.  An edit IN PLACE would leave the device copy stale without a trace, so the
        cached arrays are made read-only: such an edit now raises (NumPy's "assignment destination is read-only");
        replace the dict entry with a new array instead and the copy is rebuilt."""
        arrays = list(arrays)
        hit = self._dev_cache.get(name)
        if (hit is not None and len(hit[0]) == len(arrays) and all(a is b for a, b in zip(hit[0], arrays))
                and hit[1].device == self.device):
            return hit[1]
        t = builder().to(self.device)
        for a in arrays:
            if isinstance(a, np.ndarray):
                try:
                    a.setflags(write=False)
                except ValueError:
                    pass
        self._dev_cache[name] = (arrays, t)
        return t

    def _level_len_dev(self, lambs) -> Optional[torch.Tensor]:
        """quantizer.py:166,171-175: None for raw lengths, else f32 [L, C, N+1] = n + overhead."""
        rm = self.raw_code_length_entropy_models
        if not rm:
            return None
        if isinstance(rm, DeviceModels):       # still where the build wrote it: no host round trip
            t = rm.device_rows(lambs, "level_len")                                  # KeyError as in the reference
            if t is not None:
                return t
        arrays = [rm[lamb] for lamb in lambs]                                       # KeyError as in the reference
        return self._keyed_dev("level_len", arrays, lambda: self._level_len_host(lambs))

    def _level_len_host(self, lambs) -> torch.Tensor:
        N = self.max_bits_per_coord
        lv = np.arange(N + 1, dtype=np.int32).astype(np.float32)
        rows = []
        for lamb in lambs:
            model = np.asarray(self.raw_code_length_entropy_models[lamb])            # C x (N+1), KeyError as in the reference
            rows.append(lv[None, :].astype(model.dtype) + model)
        return torch.from_numpy(np.stack(rows).astype(np.float32))

    def _solve_idx(self, mu_cb, sg_cb, lambs, level_len, out_idx=None):
        """u16 rank indices [L, C, B] on the device (written into out_idx where given)."""
        return ops.quantize(mu_cb, sg_cb, self._table_dev(), [float(l) for l in lambs], N=self.max_bits_per_coord,
                            level_len=level_len, layout="cb", out_idx=out_idx)

    def _workspace(self, name: str, nbytes: int) -> torch.Tensor:
        """A persistent device workspace, grown on demand (planes + index planes of the per-image call)."""
        ws = self._dev_cache.get(name)
        if ws is None or ws.numel() < nbytes or ws.device != self.device:
            ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.device)
            self._dev_cache[name] = ws
        return ws

    def _stager(self):
        """The pinned staging blocks behind the lazy per-image results (vbq_amd.lazy.HostStager), one set per quantizer."""
        st = self._dev_cache.get("_stager")
        if st is None:
            from .lazy import HostStager
            st = self._dev_cache["_stager"] = HostStager()
        return st

    def _latents_call(self, means_bc, spread_bc, lambs, *, spread, level_len, models):
        """vbq_compress_latents_f32: planes, solve and the fused lookups of one batch in ONE C call (three launches).
        -> (Z_hat, raw_num_bits, num_bits | None), channel-last [L, B, C] device tensors."""
        from . import _lib
        N, C = self.max_bits_per_coord, self.num_channels
        if getattr(self, "validate_inputs", False):
            sig = spread_bc if spread == "sigma" else (torch.exp(spread_bc) ** 0.5 if spread == "logvar" else torch.sqrt(spread_bc))
            ops.check_inputs(means_bc.contiguous(), sig.contiguous())
        B = means_bc.shape[0]
        ws = self._workspace("_ws_latents", _lib.lib().vbq_compress_latents_workspace_bytes(B, C, len(lambs), N))
        return ops.compress_latents(means_bc, spread_bc, self._table_dev(), self._sorted_dev(), [float(l) for l in lambs], N=N,
                                    spread=spread, level_len=level_len, models=models, workspace=ws)

    def _f32_dev(self, a) -> torch.Tensor:
        """A NumPy array (or anything _to_numpy takes) or a tensor as an f32 tensor on the device."""
        t = a if isinstance(a, torch.Tensor) else ops.host_tensor(_to_numpy(a))     # any layout, read-only too: as api.quantize
        return t.to(self.device, torch.float32)

    def _batch_dev(self, batch_means, batch_stds):
        mu, sg = self._f32_dev(batch_means), self._f32_dev(batch_stds)
        if mu.dim() != 2 or mu.shape[1] != self.num_channels or mu.shape != sg.shape:
            raise ValueError(f"expected means/stds of shape [B, {self.num_channels}], got {tuple(mu.shape)} / {tuple(sg.shape)}")
        return mu, sg

    def compress_batch_channel_latents(self, batch_means, batch_stds, lambs, return_np=True, **kwargs):
        """quantizer.py:156-188 -> (Z_hat_dict, num_bits_dict), each dict[lamb] -> [B, C].
        num_bits is int32 (raw bit lengths) before the raw-length entropy models exist and
        float32 (n + overhead) afterwards, as in the reference."""
        lambs = list(lambs)
        mu, sg = self._batch_dev(batch_means, batch_stds)
        zhat, bits, _ = self._latents_call(mu, sg, lambs, spread="sigma", level_len=self._level_len_dev(lambs), models=None)
        if return_np:
            # ndarray-like views over the device tensors (vbq_amd.lazy): what is read on the host crosses PCIe, nothing else
            from .lazy import DeviceStack, group
            zs, bs = group([DeviceStack("batch_Z_hat", zhat, self._stager()), DeviceStack("batch_num_bits", bits, self._stager())])
            return dict(zip(lambs, zs.rows())), dict(zip(lambs, bs.rows()))
        return {lamb: zhat[i] for i, lamb in enumerate(lambs)}, {lamb: bits[i] for i, lamb in enumerate(lambs)}

    # ------------------------------------------------------------------ entropy models (quantizer.py:82-150)
    def _encode(self, X, vae):
        posterior_means, posterior_logvars = vae.encode(X)
        return self._f32_dev(posterior_means), self._f32_dev(posterior_logvars)

    def build_entropy_models(self, X, vae, lambs, add_n_smoothing):
        means, logvars = self._encode(X, vae)
        C = logvars.shape[-1]
        assert C == self.num_channels                                               # quantizer.py:89
        # batch_stds = exp(posterior_logvars) ** 0.5 (quantizer.py:87,92) is taken inside the planes kernel
        return self.build_entropy_models_from_latents(means.reshape(-1, C), logvars.reshape(-1, C), lambs, add_n_smoothing,
                                                      spread="logvar")

    def build_entropy_models_from_latents(self, batch_means, batch_stds, lambs, add_n_smoothing, spread="sigma"):
        """The body of quantizer.py:94-150 on (B x C) means/stds: vbq_amd.pipeline.EntropyModelBuild (pass 1 = solve +
        bit-length histogram in one kernel, length table on the device, pass 2 = solve + rank histogram + models).
        NOTHING here waits for the device: the three tables stay where the kernels wrote them behind dict-like views
        (`DeviceModels`) and reach NumPy when a caller reads them -- compress_latents never does.
        A rebuild starts from raw lengths again.  (In the reference a second build on the same object would feed the
        float "n + overhead" lengths of the first one to np.bincount, :96,104,166, which raises TypeError; starting
        over is the documented divergence)"""
        from .pipeline import EntropyModelBuild
        lambs = list(lambs)
        N, C = self.max_bits_per_coord, self.num_channels
        mu_bc, sp_bc = self._batch_dev(batch_means, batch_stds)
        if getattr(self, "validate_inputs", False):
            ops.check_inputs(mu_bc.contiguous(), (sp_bc if spread == "sigma" else torch.exp(sp_bc) ** 0.5).contiguous())
        B = mu_bc.shape[0]
        B_global, distributed = B, self.process_group is not None
        if distributed:
            import torch.distributed as dist
            t = torch.tensor([B], dtype=torch.int64, device=self.device)
            dist.all_reduce(t, group=self.process_group)
            B_global = int(t.item())
        # the index planes, the workspaces and the -log2 tables are kept between builds of one shape; the OUTPUT tensors are
        # new every time (the dicts of an earlier build keep theirs)
        build = EntropyModelBuild(B, C, [float(l) for l in lambs], self._table_dev(), N=N, add_n_smoothing=add_n_smoothing,
                                  global_rows=B_global, distributed=distributed, group=self.process_group,
                                  counts_dtype=torch.int32 if B_global < 2 ** 31 else torch.int64, keep_models=self._strict,
                                  buffers=self._dev_cache.setdefault("_build_buffers", {}))
        # (a rebuild starts from raw lengths: both passes below get their lengths as arguments and never read
        # self.raw_code_length_entropy_models, which -- like everything else of the quantizer -- changes only once they succeeded)
        if build.one_call_ok and B > 0:
            # one GPU, tabulated -log2: planes, both passes, the histogram and the models behind ONE C call
            build.run_one_call(mu_bc, sp_bc, spread)
            level_len, raw_models, counts = build.level_len, build.raw_models, build.counts
        else:
            mu_cb, sg_cb = ops.prep_planes(mu_bc, sp_bc, spread=spread)
            build.pass1(mu_cb, sg_cb, None)
            level_len, raw_models = build.lengths()
            # pass 2: corrected lengths -> per-channel histogram of the code points (:118-148)
            _, counts = build.pass2(mu_cb, sg_cb, level_len)
        models_dev = build.finish_models()
        if models_dev is not None:
            state = {"done": False}

            def deferred_checks():           # first host read of any of the three tables (synchronises)
                if not state["done"]:
                    state["done"] = True
                    build.check()

            if build.has_host_stages:        # a failed NumPy stage must not go unnoticed by device-only callers either
                deferred_checks()
            self._add_n_smoothing = add_n_smoothing
            self._dev_cache.pop("entropy_models", None)
            self._dev_cache.pop("level_len", None)
            self.raw_code_length_entropy_models = DeviceModels(lambs, raw_models, {"level_len": level_len}, deferred_checks)
            self.entropy_models = DeviceModels(lambs, models_dev, None, deferred_checks)
            # kept for the entropy coder (vbq_amd.coder): the integer histograms behind the models
            self._code_counts = DeviceModels(lambs, counts, None, deferred_checks)
            return None
        # repeated f32 code points (or a model table too large to keep): the counts go to the host
        build.wait()
        torch.cuda.synchronize(self.device)
        build.check()
        raw_models = raw_models.cpu().numpy()
        counts = counts.cpu().numpy()
        if not self._strict:   # qidx is the FIRST sorted position of a repeated value (:135)
            merged = np.zeros_like(counts)
            for c in range(self.num_channels):
                np.add.at(merged[:, c, :], (slice(None), self._canon[c]), counts[:, c, :])
            counts = merged
        models = _entropy.neg_log2_freq(counts, add_n_smoothing)                    # [L, C, T] f32
        self._add_n_smoothing = add_n_smoothing
        self._dev_cache.pop("entropy_models", None)
        self.raw_code_length_entropy_models = {lamb: raw_models[i] for i, lamb in enumerate(lambs)}
        self.entropy_models = {lamb: models[i] for i, lamb in enumerate(lambs)}
        self._code_counts = {lamb: counts[i] for i, lamb in enumerate(lambs)}
        self._dev_cache["level_len"] = ([self.raw_code_length_entropy_models[lamb] for lamb in lambs], level_len)
        for d in (self.entropy_models, self.raw_code_length_entropy_models):
            for a in d.values():
                a.setflags(write=False)          # see _keyed_dev: in-place edits must not go unnoticed
        return None

    @property
    def lambs(self):
        return list(sorted(self.entropy_models.keys()))

    # ------------------------------------------------------------------ compression (quantizer.py:190-256)
    def _models_dev(self, lambs) -> torch.Tensor:
        """entropy_models of `lambs` as f32 [L, C, T] on the device, indexed by RANK."""
        em = self.entropy_models
        if isinstance(em, DeviceModels):
            t = em.device_rows(lambs)                                                # KeyError as in the reference
            if t is not None:
                return t

        def models_host():
            models = np.stack([np.asarray(em[lamb]) for lamb in lambs]).astype(np.float32)               # [L, C, T]
            if not self._strict:   # the reference indexes with the canonical qidx; same value either way once
                models = np.stack([np.take_along_axis(mm, self._canon, axis=1) for mm in models])        # mapped per rank
            return torch.from_numpy(models)
        return self._keyed_dev("entropy_models", [em[lamb] for lamb in lambs], models_host)

    def compress_latents(self, posterior_means, posterior_logvars, lambs, return_np=True):
        """quantizer.py:190-240 as ONE C call = three launches (vbq_compress_latents_f32: planes with the
        `exp(posterior_logvars) ** 0.5` of :197,202 folded in, the solve, and one pass over the indices that writes Z_hat,
        raw_num_bits and num_bits channel-last); no torch arithmetic anywhere in it.  return_np=False keeps the per-lambda results on the device (torch tensors shaped like the
        latents): no 150 MB device-to-host copy per Kodak image x 32 lambdas, which is what bounds the NumPy form (PCIe).
        The reference returns NumPy arrays (np.reshape moves to the CPU, :237); that is the default here too."""
        lambs = list(lambs)
        C = self.num_channels
        shape = tuple(np.shape(posterior_means))
        m, lv = self._f32_dev(posterior_means), self._f32_dev(posterior_logvars)
        assert lv.shape[-1] == C                                                     # quantizer.py:195
        # sigma = exp(logvar) ** 0.5 (quantizer.py:197,202) is taken inside the planes kernel
        zhat, raw_bits, num_bits = self._latents_call(m.reshape(-1, C), lv.reshape(-1, C), lambs, spread="logvar",
                                                      level_len=self._level_len_dev(lambs), models=self._models_dev(lambs))
        out_keys = ("Z_hat", "raw_num_bits", "num_bits_cl", "num_bits")
        output = {key: dict() for key in out_keys}
        L = len(lambs)
        if not return_np:
            arrs = {"Z_hat": zhat.reshape((L,) + shape), "raw_num_bits": raw_bits.reshape((L,) + shape),
                    "num_bits": num_bits.reshape((L,) + shape)}
        else:
            # NumPy-like views over the device tensors (vbq_amd.lazy): a quantity crosses PCIe -- through a persistent pinned
            # staging block, all its lambdas at once -- when somebody first READS it on the host; a caller that hands Z_hat back
            # to a decoder on the device and sums num_bits there (compress / vbq_amd.utils.evaluate_*) copies nothing.
            from .lazy import DeviceStack, group
            stager = self._stager()
            stacks = group([DeviceStack("Z_hat", zhat.reshape((L,) + shape), stager),
                            DeviceStack("raw_num_bits", raw_bits.reshape((L,) + shape), stager),
                            DeviceStack("num_bits", num_bits.reshape((L,) + shape), stager)])
            arrs = {st.name: st.rows() for st in stacks}
        has_cl = bool(self.raw_code_length_entropy_models)
        for i, lamb in enumerate(lambs):
            output["Z_hat"][lamb] = arrs["Z_hat"][i]
            output["raw_num_bits"][lamb] = arrs["raw_num_bits"][i]
            if has_cl:
                output["num_bits_cl"][lamb] = output["raw_num_bits"][lamb]          # :231-232
            output["num_bits"][lamb] = arrs["num_bits"][i]
        return output

    def compress_replay(self, X, vae, lambs, clip=True):
        """`compress(X, vae, lambs, clip)` AND what the evaluation loop reads of it (utils.py:547-556) as ONE HIP graph replay per
        image shape (vbq_amd.replay): -> (the result dict, (sums of num_bits, sums of num_bits_cl, uint8 X_hat) on the host).
        The dict's arrays live in the graph's static tensors: valid until the next call with the same shape.  Falls back to
        `compress` + `utils.evaluation_reads` when the VAE cannot be captured (NumPy VAEs, decoders that synchronise)."""
        from .replay import CompressReplay
        X = _to_numpy(X) if not isinstance(X, np.ndarray) else X      # (a tensor on any device, also one that requires grad)
        lambs = list(lambs)                                       # an ndarray, a tuple, ...: `list == ndarray` below would be an array
        cache = self._dev_cache.setdefault("_replays", {})
        last = self._dev_cache.get("_replay_last")                # the loop's common case: the same shape, settings and VAE as last time
        if last is not None and last[0] == X.shape and last[1] is vae and last[2] == lambs and last[3] == bool(clip) and last[4] == X.dtype:
            key, rp = last[5], last[6]
        else:
            key = (X.shape, X.dtype.str, tuple(lambs), bool(clip), id(vae))
            rp = cache.get(key)
        fp = self._replay_fingerprint(lambs)
        if rp is None or rp.vae is not vae or rp.fingerprint != fp:
            if len(cache) >= 8:
                cache.clear()
            rp = CompressReplay(self, vae, X, lambs, clip)
            rp.fingerprint = self._replay_fingerprint(lambs)      # (after the capture: its warm-up may have grown the workspace)
            cache[key] = rp
        self._dev_cache["_replay_last"] = (X.shape, vae, lambs, bool(clip), X.dtype, key, rp)
        return rp.run(X)

    def _replay_fingerprint(self, lambs):
        """Addresses of everything a captured per-image graph reads besides its own static tensors: a new table, a rebuilt model
        or a workspace another shape made grow means a new capture."""
        ll, ws = self._level_len_dev(lambs), self._dev_cache.get("_ws_latents")
        return (self._table_dev().data_ptr(), self._sorted_dev().data_ptr(), None if ll is None else ll.data_ptr(),
                self._models_dev(lambs).data_ptr(), None if ws is None else (ws.data_ptr(), ws.numel()))

    # ------------------------------------------------------------------ real bits
    def _need_entropy_models(self):
        if self.entropy_models is None or not hasattr(self, "_code_counts"):
            raise ValueError("build_entropy_models() first")

    def codec(self, lambs, segment=1024):
        """rANS codec whose frequency tables are the histograms behind entropy_models[lamb]
        (one table per (lambda, channel)); see vbq_amd.coder."""
        from .coder import RansCodec, quantize_frequencies
        self._need_entropy_models()
        counts = np.stack([self._code_counts[lamb] for lamb in lambs])              # [L, C, T]
        freq = quantize_frequencies(counts, add_n_smoothing=self._add_n_smoothing)
        return RansCodec(freq.reshape(-1, self.quantization_levels), N=self.max_bits_per_coord, segment=segment)

    def encode_batch(self, batch_means, batch_stds, lambs, segment=1024):
        """Solve + entropy-code: returns (words, sizes, codec); total size = codec.compressed_bits(sizes).
        Streams are ordered [lambda][channel], each holding the B indices of that channel."""
        lambs = list(lambs)
        mu_cb, sg_cb = self._prep(batch_means, batch_stds)
        idx = self._solve_idx(mu_cb, sg_cb, lambs, self._level_len_dev(lambs))     # [L, C, B]
        if not self._strict:
            # repeated f32 code points: K1 may emit any rank of a run of equal values, the histogram behind the
            # frequency tables is the canonical one (first position, :135) -- code the canonical index (same Z_hat)
            canon = self._dev("canon", lambda: torch.from_numpy(self._canon))       # [C, T] int64
            idx = torch.gather(canon[None].expand(len(lambs), -1, -1), 2, idx.to(torch.int64)).to(torch.uint16)
        cdc = self.codec(lambs, segment)
        words, sizes = cdc.encode(idx)
        return words, sizes, cdc

    def decode_batch(self, words, sizes, codec, n_rows, lambs, return_np=True):
        """Inverse of encode_batch: dict[lamb] -> Z_hat [B, C]."""
        lambs = list(lambs)
        C = self.num_channels
        idx = codec.decode(words, sizes, n_rows).reshape(len(lambs), C, n_rows)
        zhat = ops.gather(idx, self._sorted_dev(), C, N=self.max_bits_per_coord, layout="cb", out_layout="bc")
        return {lamb: (zhat[i].cpu().numpy() if return_np else zhat[i]) for i, lamb in enumerate(lambs)}

    # ------------------------------------------------------------------ byte strings (vbq_amd.bitstream)
    def _check_coder_bits(self):
        if self.max_bits_per_coord > 10:
            raise ValueError(f"max_bits_per_coord = {self.max_bits_per_coord}: the rANS coder supports at most 10")

    def _lambda_key(self, lamb):
        """The key of entropy_models equal to `lamb` as a float64 (KeyError otherwise, as compress_latents)."""
        self._need_entropy_models()
        for k in self.lambs:
            if float(k) == float(lamb):
                return k
        raise KeyError(lamb)

    def _coder_tables(self, lamb, segment=None):
        """(codec, digest) of one lambda; segment=None: a codec without one, for the interleaved layout.  The quantised
        frequencies and the digest are cached per lambda, keyed on the identity of the `_code_counts` object a build installs
        (as _keyed_dev keys on identities): a rebuild of the entropy models -- or build_code_points, which clears the device
        cache -- invalidates them.  The codecs are cached under their lambda, per segment."""
        from .coder import RansCodec, quantize_frequencies
        cc = self._code_counts
        hit = self._dev_cache.get("_coder_tables")
        if hit is None or hit[0] is not cc or hit[1] != self._add_n_smoothing:
            hit = self._dev_cache["_coder_tables"] = (cc, self._add_n_smoothing, {})
        per = hit[2]
        ent = per.get(lamb)
        if ent is None:
            rows = cc.device_rows([lamb]) if isinstance(cc, DeviceModels) else None     # one lambda's rows, not the whole stack
            counts = rows[0].cpu().numpy() if rows is not None else np.asarray(cc[lamb])
            freq = quantize_frequencies(counts, add_n_smoothing=self._add_n_smoothing)    # [C, T]
            ent = per[lamb] = {"freq": freq, "digest": bitstream.digest(self.code_points_by_channel, freq), "codecs": {}}
        codec = ent["codecs"].get(segment)
        if codec is None:
            codec = ent["codecs"][segment] = RansCodec(ent["freq"], N=self.max_bits_per_coord, segment=segment)
        return codec, ent["digest"]

    def _file_layout(self, posterior_means, posterior_logvars, layout, segment, part):
        """(latent shape, layout, its segment or part) of a file: the shape channel-last and one for both inputs; ValueError
        otherwise, for an unknown layout, or for a bad segment (layout "segments") or part (layout "interleaved")."""
        C = self.num_channels
        shape = tuple(int(d) for d in np.shape(posterior_means))
        if tuple(np.shape(posterior_logvars)) != shape or not shape or shape[-1] != C:
            raise ValueError(f"expected channel-last latents [..., {C}] of one shape, got {shape} / {tuple(np.shape(posterior_logvars))}")
        lay = _LAYOUTS.get(layout) if isinstance(layout, str) else None
        if lay is None:
            raise ValueError(f"layout {layout!r}: expected 'segments' or 'interleaved'")
        unit = part if lay.unit == "part" else segment
        lay.check(unit)
        return shape, lay, int(unit)

    def _file_indices(self, posterior_means, posterior_logvars, keys):
        """The u16 indices [L, C, B] a file codes: one solve of every lambda of `keys` with sigma = exp(logvar) ** 0.5, and the
        canonical index of a run of equal code points when the table has any (see encode_batch)."""
        C = self.num_channels
        m, lv = self._f32_dev(posterior_means), self._f32_dev(posterior_logvars)
        mu_cb, sg_cb = self._prep(m.reshape(-1, C), lv.reshape(-1, C), spread="logvar")
        idx = self._solve_idx(mu_cb, sg_cb, keys, self._level_len_dev(keys))                  # [L, C, B]
        if not self._strict:
            # one lambda at a time, in place: the int64 gather index and result stay [C, B] (16 lambdas of Kodak-24 at once
            # would be two 1.2 GB temporaries)
            canon = self._dev("canon", lambda: torch.from_numpy(self._canon))                 # [C, T] int64
            for l in range(idx.shape[0]):
                idx[l] = torch.gather(canon, 1, idx[l].to(torch.int64)).to(torch.uint16)
        return idx

    def compress_latents_to_bytes(self, posterior_means, posterior_logvars, lamb, segment=1024, layout="segments",
                                  part=1 << 17) -> bytes:
        """compress_latents at ONE lambda, entropy-coded into a self-describing byte string (format: vbq_amd.bitstream).
        Same inputs and sigma = exp(logvar) ** 0.5 as compress_latents; the indices come from the same solve (the canonical
        index of a repeated code point, as encode_batch).  Solve, encode and pack run on the device; two device-to-host
        copies (the total with the segment sizes, then the payload).
        layout="interleaved" writes the compact file instead (magic b"VBQc": the wave-interleaved coder in parts of `part`
        symbols, `segment` unused): the same indices and tables in fewer bytes -- 256 bytes of fixed cost per part where the
        default layout pays 6 bytes and the word rounding per segment.  decompress_latents reads either."""
        self._check_coder_bits()
        key = self._lambda_key(lamb)
        shape, lay, unit = self._file_layout(posterior_means, posterior_logvars, layout, segment, part)
        codec, dig = self._coder_tables(key, lay.segment(unit))
        idx = self._file_indices(posterior_means, posterior_logvars, [key])[0]                 # [C, B]
        sizes, payload = lay.encode(codec, idx, unit)
        h = lay.header(N=self.max_bits_per_coord, C=self.num_channels, shape=shape, lamb=float(key), digest=dig,
                       n_words=int(payload.size), **{lay.unit: unit})
        return lay.write(h, sizes, payload)

    def decompress_latents(self, data, return_np=True):
        """Inverse of compress_latents_to_bytes: Z_hat shaped like the latents (NumPy, or a device tensor with
        return_np=False), bit-identical to compress_latents(...)["Z_hat"][lamb].  ValueError for a malformed header or
        a stream made with another quantizer / entropy model (digest), KeyError for a lambda this quantizer has no
        model for, VBQError for a damaged payload.  A lambda-map file (magic b"VBQm", compress_latents_to_bytes_mapped) is
        read by its magic: bit-identical to compress_latents_mapped(...)["Z_hat"]."""
        self._check_coder_bits()
        if bytes(memoryview(data).cast("B")[:4]) == bitstream.MAPPED_MAGIC:
            return self._decompress_latents_mapped(data, return_np)
        h, _, _ = bitstream.parse_latent(data)
        lay = next(l for l in _LAYOUTS.values() if l.header is type(h))
        if h.N != self.max_bits_per_coord or h.C != self.num_channels:
            raise ValueError(f"stream is for N = {h.N}, C = {h.C}; this quantizer has N = {self.max_bits_per_coord}, "
                             f"C = {self.num_channels}")
        key = self._lambda_key(h.lamb)
        codec, dig = self._coder_tables(key, lay.segment(h.unit))
        if dig != h.digest:
            raise ValueError("stream was compressed with a different quantizer or entropy model (digest mismatch)")
        tail = np.frombuffer(memoryview(data).cast("B"), dtype="<u2", count=h.sizes_nbytes // 2 + h.n_words, offset=h.nbytes)
        idx = lay.decode(codec, torch.from_numpy(tail.copy()).to(self.device), h)           # sizes, then payload: one upload
        zhat = ops.gather(idx[None], self._sorted_dev(), self.num_channels, N=self.max_bits_per_coord, layout="cb",
                          out_layout="bc")                                                # [1, B, C]
        zhat = zhat.reshape(h.shape)
        return zhat.cpu().numpy() if return_np else zhat

    # ------------------------------------------------------------------ windows and batches (include/vbq.h, "Window decode")
    def _window_headers(self, files):
        """The parsed headers of `files` with the checks of decompress_latents on each, (headers, sizes, payload offsets, keys);
        ValueError naming the index of a file that is no b"VBQb" file of this quantizer or has another segment."""
        heads, sizes, starts, keys = [], [], [], []
        for i, data in enumerate(files):
            magic = bytes(memoryview(data).cast("B")[:4])
            foreign = {bitstream.COMPACT_MAGIC: "a compact file (magic b'VBQc'): its parts are not addressable",
                       bitstream.MAPPED_MAGIC: "a lambda-map file (magic b'VBQm'): it has a table per symbol"}.get(magic)
            if foreign:
                raise ValueError(f"file {i} is {foreign}; windows and batches read files in segments (magic b'VBQb')")
            h, sz, start, key = self._batch_file_header(i, data, bitstream.parse, heads[0].segment if heads else None)
            heads.append(h), sizes.append(sz), starts.append(start), keys.append(key)
        return heads, sizes, starts, keys

    def _batch_file_header(self, i, data, parse, segment=None):
        """File i of a batch parsed by `parse` (bitstream.parse / parse_compact) with the checks of decompress_latents ->
        (header, sizes, payload offset, key); ValueError naming i for a malformed file, one of another N or C, another segment
        length than `segment` (where given) or another digest; KeyError for a lambda without a model."""
        try:
            h, sz, start = parse(data)
        except ValueError as e:
            raise ValueError(f"file {i}: {e}") from None
        return h, sz, start, self._batch_header_keys(i, h, segment)[0]

    def _batch_header_keys(self, i, h, segment=None):
        """The checks of _batch_file_header on the parsed header h of file i -> the keys of its lambdas: one, or the palette of
        a lambda-map file, whose digests are checked class by class."""
        if h.N != self.max_bits_per_coord or h.C != self.num_channels:
            raise ValueError(f"file {i} is for N = {h.N}, C = {h.C}; this quantizer has N = {self.max_bits_per_coord}, "
                             f"C = {self.num_channels}")
        if segment is not None and h.segment != segment:
            raise ValueError(f"file {i} is in segments of {h.segment} symbols, file 0 in segments of {segment}: "
                             "one call decodes files of one segment length")
        palette = isinstance(h, bitstream.MappedHeader)
        keys = [self._lambda_key(l) for l in (h.lambs if palette else (h.lamb,))]
        for p, (key, dig) in enumerate(zip(keys, h.digests if palette else (h.digest,))):
            if self._coder_tables(key, getattr(h, "segment", None))[1] != dig:
                where = f"digest mismatch in class {p} of its palette" if palette else "digest mismatch"
                raise ValueError(f"file {i} was compressed with a different quantizer or entropy model ({where})")
        return keys

    def decompress_latents_batch(self, files, regions=None, channels=None, return_np=False):
        """The same-sized boxes of many latent files in ONE launch: f32 [F, *extents, C_sel], every value bit-identical to
        decompress_latents(files[f])[regions[f]][..., channels].  `files`: b"VBQb" byte strings of this quantizer -- any built
        lambdas and any latent shapes, one `segment`; each gets the checks of decompress_latents (ValueError naming the
        file's index, KeyError for a lambda without a model).  `regions`: None (whole files, whose shapes must then agree), ONE
        region for all files -- a tuple of slices of step 1, one per leading axis (bitstream.region_box) -- or a list with one
        such tuple (or None) per file; the extents must agree.  `channels`: None or channel numbers, any order, repeats
        allowed.  Work: one staging buffer and one upload, one vbq_rans_segment_offsets_u16 over all sizes, one
        vbq_rans_decode_window_f32 over the segments that hold a row of a box, one read of the status words.  A damaged
        file raises VBQError naming the index of the first one; damage in segments no box touches is not seen."""
        return self._window_call(self._window_plan(files, regions, channels), self._window_run, return_np)

    def _window_call(self, plan, run, return_np):
        """The one upload of plan.host, `run` (_window_run or _mapped_window_run) and the one read of the status words:
        VBQError naming the first damaged file."""
        from . import _lib, coder
        if plan.host is None:                                      # no file, no channel or an empty extent: nothing to launch
            out = torch.empty(plan.shape, dtype=torch.float32, device=self.device)
            return out.cpu().numpy() if return_np else out
        out, status = run(plan, torch.from_numpy(plan.host).to(self.device))
        st = status.cpu().numpy()
        for f in np.flatnonzero(st[:-1]):
            try:
                coder._raise_status(int(st[f]))
            except _lib.VBQError as e:
                raise _lib.VBQError(f"file {int(f)}: {e}") from None
        coder._raise_status(int(st[-1]))
        return out.cpu().numpy() if return_np else out

    _WindowPlan = namedtuple("_WindowPlan", "shape host cut F n_sel C_sel M n_words segment tables box")

    def _window_plan(self, files, regions, channels):
        """The host side of decompress_latents_batch: every check, the boxes, the segment lists and the ONE staging buffer
        (plan.host, u8; None when there is nothing to decode): descriptors int64 [F, 8], segment lists int32 [F, n_sel] and
        channels int32 [C_sel] (each padded to 8 bytes), then all sizes u16 [M], then all payloads u16 -- the last two straight
        from the files.  plan.cut: where each part starts."""
        files, regions, ch, C_sel = self._window_inputs(files, regions, channels)
        heads, sizes, starts, keys = self._window_headers(files)
        F = len(files)
        shape, boxes, geometry, seg_ids, chans, n_sel = self._window_geometry(heads, regions, ch, C_sel)
        if seg_ids is None:
            return self._WindowPlan(shape, None, None, F, 0, C_sel, 0, 0, None, [], None)
        segment = heads[0].segment
        tables = sorted(set(keys), key=float)                      # (a stable tag for the codec cache of _coder_stack)
        M, n_words = sum(h.n_sizes for h in heads), sum(h.n_words for h in heads)
        desc = np.empty((F, 8), np.int64)
        desc[:, :7] = geometry
        desc[:, 7] = [tables.index(k) for k in keys]
        head = [desc.view(np.uint8).reshape(-1), seg_ids.view(np.uint8), chans.view(np.uint8)]
        raws = [np.frombuffer(memoryview(d).cast("B"), dtype=np.uint8) for d in files]
        host = np.concatenate(head + [r[h.nbytes: h.nbytes + 2 * h.n_sizes] for r, h in zip(raws, heads)]
                              + [r[s: s + 2 * h.n_words] for r, h, s in zip(raws, heads, starts)])
        cut = [int(c) for c in np.cumsum([0, head[0].size, head[1].size, head[2].size, 2 * M, 2 * n_words])]
        box = tuple(h - l for l, h in zip(boxes[0][1], boxes[0][2]))
        return self._WindowPlan(shape, host, cut, F, n_sel, C_sel, M, n_words, segment, tables, box)

    def _window_inputs(self, files, regions, channels):
        """What both window plans do before they read a file: (files as a list, one region per file, the channel list as int32
        or None, C_sel); ValueError for a wrong count of regions or a channel outside [0, C)."""
        self._check_coder_bits()
        files = list(files)
        F, C = len(files), self.num_channels
        one = regions is None or isinstance(regions, slice) or (isinstance(regions, (tuple, list)) and
                                                                 all(isinstance(r, slice) for r in regions))
        regions = [regions] * F if one else list(regions)
        if len(regions) != F:
            raise ValueError(f"{len(regions)} regions for {F} files")
        ch = None
        if channels is not None:
            ch = np.asarray(channels).reshape(-1)
            if ch.size and (ch.dtype.kind not in "iu" or int(ch.min()) < 0 or int(ch.max()) >= C):
                raise ValueError(f"channels must be integers in [0, {C})")
            ch = ch.astype(np.int32)
        return files, regions, ch, C if ch is None else int(ch.size)

    @staticmethod
    def _window_geometry(heads, regions, ch, C_sel):
        """What both window plans stage alike, from the parsed headers (of one segment length): (output shape, boxes, the
        descriptors' first seven fields int64 [F, 7] -- seg_base, n, D1, D2, a0, a1, a2 --, segment lists int32 padded with -1 to
        [F, n_sel] and to 8 bytes, channels int32 padded to 8 bytes, n_sel).  Everything after the shape is None when there is
        nothing to decode: no file, no channel or an empty extent."""
        F = len(heads)
        boxes, extents = bitstream.region_boxes([h.shape[:-1] for h in heads], regions)
        shape = (F,) + tuple(extents) + (C_sel,)
        if F == 0 or C_sel == 0 or 0 in extents:
            return shape, None, None, None, None, 0
        lists = [bitstream.box_segments(dims, lo, hi, heads[0].segment) for dims, lo, hi in boxes]
        n_sel = max(l.size for l in lists)
        geometry = np.empty((F, 7), np.int64)
        base = 0
        for f, (h, (dims, lo, hi)) in enumerate(zip(heads, boxes)):
            geometry[f] = (base, h.n_rows, dims[1], dims[2], lo[0], lo[1], lo[2])
            base += h.n_sizes
        seg_ids = np.full(F * n_sel + (F * n_sel & 1), -1, np.int32)
        for f, l in enumerate(lists):
            seg_ids[f * n_sel: f * n_sel + l.size] = l
        chans = np.zeros(0, np.int32) if ch is None else np.concatenate([ch, np.zeros(C_sel & 1, np.int32)])
        return shape, boxes, geometry, seg_ids, chans, n_sel

    def _window_run(self, plan, dev):
        """The device side: `dev` is plan.host on the device.  One vbq_rans_segment_offsets_u16 over all sizes and one
        vbq_rans_decode_window_f32 -> (out f32 plan.shape, status u32 [F + 1]: per file, then the scan's); nothing is read
        back."""
        d_files, d_segs, d_ch, d_sizes, d_payload, offsets, status, freq = self._window_device(plan, dev, 8, 3)
        out, _ = ops.rans_decode_window(d_payload, d_sizes, offsets, d_files, d_segs, freq, self._sorted_dev(), plan.box,
                                        seg=plan.segment, N=self.max_bits_per_coord, channels=d_ch, status=status[:plan.F])
        return out.view(plan.shape), status

    def _window_device(self, plan, dev, fields, k):
        """The views of a window plan's staging buffer on the device -- descriptors [F, fields], segment lists, channels (None
        for all), sizes and payload at plan.cut[k:] --, the offsets of vbq_rans_segment_offsets_u16 over the sizes, the zeroed
        status words u32 [F + 1] (the last one the scan's) and the frequency stack [n_tables, C, T]."""
        from . import _lib
        F, C, cut = plan.F, self.num_channels, plan.cut
        d_files = dev[cut[0]:cut[1]].view(torch.int64).view(F, fields)
        d_segs = dev[cut[1]:cut[1] + 4 * F * plan.n_sel].view(torch.int32).view(F, plan.n_sel)
        d_ch = dev[cut[2]:cut[2] + 4 * plan.C_sel].view(torch.int32) if cut[3] > cut[2] else None
        d_sizes, d_payload = dev[cut[k]:cut[k + 1]].view(torch.uint16), dev[cut[k + 1]:cut[k + 2]].view(torch.uint16)
        offsets = torch.empty(plan.M, dtype=torch.int64, device=dev.device)
        status = torch.zeros(F + 1, dtype=torch.uint32, device=dev.device)
        _lib.check(_lib.lib().vbq_rans_segment_offsets_u16(ops._ptr(d_sizes), plan.M, plan.segment, plan.n_words,
                                                            ops._ptr(offsets), ops._ptr(status[F:]), ops._stream(dev)),
                   "vbq_rans_segment_offsets_u16")
        freq = self._coder_stack(plan.tables, plan.segment)._freq(dev.device).view(len(plan.tables), C, -1)
        return d_files, d_segs, d_ch, d_sizes, d_payload, offsets, status, freq

    def decompress_latents_window(self, data, region, channels=None, return_np=True):
        """decompress_latents(data)[region][..., channels] without decoding the rest: the batch of one file
        (decompress_latents_batch) with the file axis dropped.  Only the segments that hold a row of the region are decoded --
        and checked: damage elsewhere in the file goes unseen."""
        return self.decompress_latents_batch([data], regions=[region], channels=channels, return_np=return_np)[0]

    # ------------------------------------------------------- windows and batches of lambda-map files ("Mapped window decode")
    def decompress_latents_mapped_batch(self, files, regions=None, channels=None, return_np=False):
        """decompress_latents_batch for lambda-map files: f32 [F, *extents, C_sel], every value bit-identical to
        decompress_latents(files[f])[regions[f]][..., channels].  `files`: b"VBQm" files (compress_latents_to_bytes_mapped) and
        b"VBQb" files of this quantizer, mixed in any order -- any built lambdas, any palettes of 1..4 of them, any latent
        shapes, one `segment`; each gets the checks of decompress_latents, the digest of every class of a palette included
        (ValueError naming the file's index, also for a compact file; KeyError for a lambda without a model).  `regions` and
        `channels` as in decompress_latents_batch.  Work: one staging buffer and one upload -- the class blocks go as the
        files pack them, 2 bits per position --, one vbq_rans_segment_offsets_u16, one vbq_rans_map_decode_window_f32, one read
        of the status words.  A damaged file raises VBQError naming the index of the first one; damage in segments no box
        touches is not seen."""
        return self._window_call(self._mapped_window_plan(files, regions, channels), self._mapped_window_run, return_np)

    def decompress_latents_mapped_window(self, data, region, channels=None, return_np=True):
        """decompress_latents(data)[region][..., channels] of a lambda-map file (or a file in segments) without decoding the
        rest: the batch of one file (decompress_latents_mapped_batch) with the file axis dropped."""
        return self.decompress_latents_mapped_batch([data], regions=[region], channels=channels, return_np=return_np)[0]

    def _mapped_window_headers(self, files):
        """_window_headers for lambda-map files and files in segments mixed: (headers, payload offsets, the keys of each file's
        palette -- one key for a b"VBQb" file); ValueError naming the index of a file that is neither, is not of this quantizer
        or has another segment."""
        heads, starts, keys = [], [], []
        for i, data in enumerate(files):
            segment = heads[0].segment if heads else None
            magic = bytes(memoryview(data).cast("B")[:4])
            if magic == bitstream.COMPACT_MAGIC:
                raise ValueError(f"file {i} is a compact file (magic b'VBQc'): its parts are not addressable; windows and batches "
                                 "read lambda-map files (magic b'VBQm') and files in segments (magic b'VBQb')")
            if magic == bitstream.MAPPED_MAGIC:
                try:
                    h, _, _, start = bitstream.parse_mapped(data)
                except ValueError as e:
                    raise ValueError(f"file {i}: {e}") from None
                palette = self._batch_header_keys(i, h, segment)
            else:
                h, _, start, key = self._batch_file_header(i, data, bitstream.parse, segment)
                palette = [key]
            heads.append(h), starts.append(start), keys.append(palette)
        return heads, starts, keys

    _MappedWindowPlan = namedtuple("_MappedWindowPlan", "shape host cut F n_sel C_sel M n_words segment tables box max_P cls_bytes")

    def _mapped_window_plan(self, files, regions, channels):
        """The host side of decompress_latents_mapped_batch, as _window_plan: every check and the ONE staging buffer (plan.host,
        u8; None when there is nothing to decode): descriptors int64 [F, 16], segment lists int32 [F, n_sel] and channels int32
        [C_sel] (each padded to 8 bytes), then the class blocks of the lambda-map files (each a multiple of 8 bytes), all sizes
        u16 [M] and all payloads u16 -- the last three straight from the files.  plan.cut: where each part starts;
        plan.tables: the distinct lambdas of all files and palettes, the rows of the frequency stack."""
        files, regions, ch, C_sel = self._window_inputs(files, regions, channels)
        heads, starts, keys = self._mapped_window_headers(files)
        F = len(files)
        shape, boxes, geometry, seg_ids, chans, n_sel = self._window_geometry(heads, regions, ch, C_sel)
        if seg_ids is None:
            return self._MappedWindowPlan(shape, None, None, F, 0, C_sel, 0, 0, None, [], None, 0, 0)
        tables = sorted({k for palette in keys for k in palette}, key=float)
        M, n_words = sum(h.n_sizes for h in heads), sum(h.n_words for h in heads)
        desc = np.zeros((F, 16), np.int64)
        desc[:, :7] = geometry
        raws = [np.frombuffer(memoryview(d).cast("B"), dtype=np.uint8) for d in files]
        blocks, cls_bytes = [], 0
        for f, (h, r, palette) in enumerate(zip(heads, raws, keys)):
            desc[f, 7] = len(palette)
            desc[f, 8: 8 + len(palette)] = [tables.index(k) for k in palette]
            desc[f, 12] = -1
            if isinstance(h, bitstream.MappedHeader):
                desc[f, 12] = cls_bytes
                blocks.append(r[h.nbytes: h.sizes_offset])
                cls_bytes += h.classes_nbytes
        head = [desc.view(np.uint8).reshape(-1), seg_ids.view(np.uint8), chans.view(np.uint8)]
        host = np.concatenate(head + blocks + [r[s - 2 * h.n_sizes: s] for r, h, s in zip(raws, heads, starts)]    # (the sizes end
                              + [r[s: s + 2 * h.n_words] for r, h, s in zip(raws, heads, starts)])                 # where the payload starts)
        cut = [int(c) for c in np.cumsum([0, head[0].size, head[1].size, head[2].size, cls_bytes, 2 * M, 2 * n_words])]
        box = tuple(h - l for l, h in zip(boxes[0][1], boxes[0][2]))
        return self._MappedWindowPlan(shape, host, cut, F, n_sel, C_sel, M, n_words, heads[0].segment, tables, box,
                                      max(len(p) for p in keys), cls_bytes)

    def _mapped_window_run(self, plan, dev):
        """The device side, as _window_run: one vbq_rans_segment_offsets_u16 over all sizes and one
        vbq_rans_map_decode_window_f32 -> (out f32 plan.shape, status u32 [F + 1]); nothing is read back."""
        d_files, d_segs, d_ch, d_sizes, d_payload, offsets, status, freq = self._window_device(plan, dev, 16, 4)
        d_cls = dev[plan.cut[3]:plan.cut[4]] if plan.cls_bytes else None
        out, _ = ops.rans_map_decode_window(d_payload, d_sizes, offsets, d_files, d_segs, freq, self._sorted_dev(), d_cls, plan.box,
                                            seg=plan.segment, max_classes=plan.max_P, N=self.max_bits_per_coord, channels=d_ch,
                                            status=status[:plan.F])
        return out.view(plan.shape), status

    def compress_to_bytes(self, X, vae, lamb, segment=1024, layout="segments", part=1 << 17) -> bytes:
        """`vae.encode(X)`, then compress_latents_to_bytes."""
        posterior_means, posterior_logvars = vae.encode(X)
        return self.compress_latents_to_bytes(posterior_means, posterior_logvars, lamb, segment=segment, layout=layout, part=part)

    # ------------------------------------------------------------------ batches of files, written (include/vbq.h, "Batch encode")
    def _batch_file_shapes(self, pairs, unit, layout="segments"):
        """The latent shape of every file of a batch, channel-last; ValueError naming the file's index for what is not a pair
        of one such shape, or for more than 65535 files.  `unit`: the segment, or the part of layout "interleaved"."""
        F = len(pairs)
        if F > bitstream.MAX_BATCH_FILES:
            raise ValueError(f"{F} files: one call takes at most {bitstream.MAX_BATCH_FILES}")
        shapes = []
        for i, pair in enumerate(pairs):
            try:
                means, logvars = pair
            except (TypeError, ValueError):
                raise ValueError(f"file {i}: expected a pair (posterior_means, posterior_logvars)") from None
            try:
                shapes.append(self._file_layout(means, logvars, layout, unit, unit)[0])
            except ValueError as e:
                raise ValueError(f"file {i}: {e}") from None
            if 0 in shapes[-1]:
                raise ValueError(f"file {i}: empty latent shape {shapes[-1]}")
        return shapes

    def _batch_file_inputs(self, latents, lambs, segment, layout="segments"):
        """Every check of compress_latents_to_bytes_batch, before any device work -> (pairs, shapes, keys, segment); with
        layout "interleaved" those of compress_latents_to_compact_batch, `segment` being its part."""
        self._check_coder_bits()
        _LAYOUTS[layout].check(segment)
        pairs = list(latents)
        F = len(pairs)
        lambs = [lambs] * F if np.ndim(lambs) == 0 else list(lambs)
        if len(lambs) != F:
            raise ValueError(f"{len(lambs)} lambdas for {F} files")
        shapes = self._batch_file_shapes(pairs, segment, layout)
        keys = [self._lambda_key(l) for l in lambs] if F else []
        return pairs, shapes, keys, int(segment)

    def compress_latents_to_bytes_batch(self, latents, lambs, segment=1024):
        """[compress_latents_to_bytes(means_f, logvars_f, lambs[f], segment=segment) for f], byte for byte, with ONE encode
        launch for all files.  `latents`: a sequence of F pairs (posterior_means, posterior_logvars), channel-last [..., C],
        NumPy or tensors, on the host or the device; shapes and numbers of leading axes may differ from file to file.  `lambs`:
        one built lambda for all files or a sequence of F, repeats and any order allowed.  Files in segments only (magic
        b"VBQb"); the table may have repeated code points.  F == 0 returns [].  Errors are those of the one-file call, raised
        before any device work: ValueError naming the file's index for a bad shape pair, ValueError for a bad `segment`, for
        len(lambs) != F or for more than 65535 files, KeyError for a lambda without a model.
        Work per call, L the number of DISTINCT lambdas: one staging buffer and one upload (the plan of bitstream.encode_plan,
        zeroed sizes and status words, and -- for inputs that are not all device tensors -- the latents; all-device inputs are
        joined by one torch.cat instead); per distinct lambda one vbq_prep_planes_f32 and one solve over the rows of the files
        that use it (their rows are adjacent, each file's run rounded up to 8 rows of mean 0, logvar 0 that are solved and
        never coded; no latent is solved at a lambda its file does not use); ONE vbq_rans_encode_files_u16 over every segment
        of every file; ONE vbq_rans_pack_u16 over all of them (two launches): 2 L + 3 launches.  Two device-to-host copies:
        the total, all segment sizes and the status words, then the first `total` payload words.  The F files are assembled
        on the host (bitstream.Header / bitstream.write); a file's n_words and payload slice come from the cumulative sum of
        the sizes already there."""
        from . import _lib
        b = self._encode_batch_plan(latents, lambs, segment)
        if b is None:
            return []
        plan, C, N = b.plan, self.num_channels, self.max_bits_per_coord
        d_host, lat = self._encode_batch_upload(b)
        payload = self._encode_batch_run(b, d_host, lat)
        F, M = len(b.keys), plan.M
        h = d_host[:b.back].cpu().numpy()
        total, sizes, status = int(h[:8].view(np.uint64)[0]), h[8:8 + 4 * M].view(np.uint32), h[8 + 4 * M:].view(np.uint32)
        for f in np.flatnonzero(status):
            raise _lib.VBQError(f"file {int(f)}: the batch encoder refused its descriptor (status {int(status[f])})")
        pay = payload[:total].cpu().numpy()
        ends = np.cumsum(sizes, dtype=np.int64)[plan.seg_base + C * plan.nseg - 1]      # of every file's words in `pay`
        out = []
        for f in range(F):
            n_words = int(ends[f] - (ends[f - 1] if f else 0))
            hd = bitstream.Header(N=N, C=C, shape=b.shapes[f], lamb=float(b.keys[f]), digest=b.digests[b.keys[f]],
                                  n_words=n_words, segment=b.segment)
            sz = sizes[int(plan.seg_base[f]): int(plan.seg_base[f] + C * plan.nseg[f])]
            out.append(bitstream.write(hd, sz, pay[int(ends[f]) - n_words: int(ends[f])]))
        return out

    _EncodeBatch = namedtuple("_EncodeBatch", "plan shapes keys tables digests segment rows pairs on_device host cut back group")

    def _encode_batch_plan(self, latents, lambs, segment):
        """The host side of compress_latents_to_bytes_batch: every check, the plan of bitstream.encode_plan and the ONE staging
        buffer (b.host, a host tensor u8, see _encode_stage): total u64 | sizes u32 [M] | status u32 [F] -- what comes back
        first (b.back bytes), zeroed by the upload -- | descriptors int64 [F, 6] | items int32 [n_items, 2] | and, unless every
        input is a device tensor, means f32 [R, C] | logvars f32 [R, C] with every file's rows where the plan puts them.
        b.cut: where each part after the first starts.  None when there is no file."""
        pairs, shapes, keys, segment = self._batch_file_inputs(latents, lambs, segment)
        F, C = len(pairs), self.num_channels
        if F == 0:
            return None
        tables = sorted(set(keys), key=float)                     # (a stable tag for the codec cache of _coder_stack)
        digests = {k: self._coder_tables(k, segment)[1] for k in tables}
        rows = [int(np.prod(sh[:-1], dtype=np.int64)) for sh in shapes]
        plan = bitstream.encode_plan(rows, [tables.index(k) for k in keys], segment, C, len(tables))
        return self._batch_stage(plan, shapes, keys, tables, digests, segment, rows, pairs, 8 + 4 * plan.M + 4 * F)

    def _batch_stage(self, plan, shapes, keys, tables, digests, segment, rows, pairs, back, group=None, extra=()):
        """The ONE staging buffer of a batch call (see _encode_batch_plan), filled: `back` zeroed bytes that the device writes
        and the host reads back | the plan's descriptors | its items | every array of `extra` (u8, each a multiple of 8 bytes:
        b.cut[3:] say where they end) | the latents unless every input is a device tensor.  `group`: the row group of every
        file (default: the table of its descriptor)."""
        C, R = self.num_channels, plan.n_rows
        group = plan.files[:, 4] if group is None else group
        cut = [int(c) for c in np.cumsum([back + (-back % 8), plan.files.nbytes, plan.items.nbytes] + [e.nbytes for e in extra])]
        on_device = all(isinstance(a, torch.Tensor) and a.is_cuda for pair in pairs for a in pair)
        host_t = self._encode_stage(cut[-1] + (0 if on_device else 8 * R * C))
        host = host_t.numpy()
        host[:cut[0]] = 0
        host[cut[0]:cut[1]] = plan.files.view(np.uint8).reshape(-1)
        host[cut[1]:cut[2]] = plan.items.view(np.uint8).reshape(-1)
        for k, e in enumerate(extra):
            host[cut[2 + k]:cut[3 + k]] = e
        if not on_device:
            stage = host[cut[-1]:].view(np.float32).reshape(2, R, C)
            row_base = plan.group_row_base[group] + plan.row0                     # of every file among the R staged rows
            for f, (means, logvars) in enumerate(pairs):
                r0, r1 = int(row_base[f]), int(row_base[f]) + rows[f]
                stage[0, r0:r1] = _to_numpy(means).reshape(-1, C)
                stage[1, r0:r1] = _to_numpy(logvars).reshape(-1, C)
                stage[:, r1:r1 + (-rows[f] % bitstream.ENCODE_ROW_ALIGN)] = 0     # the padding rows: mean 0, logvar 0
        return self._EncodeBatch(plan, shapes, keys, tables, digests, segment, rows, pairs, on_device, host_t, cut, back, group)

    def _encode_stage(self, nbytes: int) -> torch.Tensor:
        """The staging buffer of _encode_batch_plan, a host tensor u8 [nbytes]: a view of ONE pinned block kept between calls and grown on
        demand (no page faults of a new allocation per call, and the upload is one DMA transfer), up to 1 GiB; a larger
        batch stages in pageable memory.  Not cleared: the plan writes every byte it uploads.  A plan's buffer is valid
        until the next plan of this quantizer."""
        if nbytes > 1 << 30:
            return torch.empty(nbytes, dtype=torch.uint8)
        st = self._dev_cache.get("_encode_stage")
        if st is None or st.numel() < nbytes:
            st = self._dev_cache["_encode_stage"] = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, pin_memory=True)
        return st[:nbytes]

    def _encode_batch_upload(self, b):
        """-> (b.host on the device, the latents f32 [2, R, C] on the device): the one upload; inputs that are all device
        tensors are joined by one torch.cat, each file's run padded to a multiple of 8 rows with zeros."""
        dev, C, plan = self.device, self.num_channels, b.plan
        d_host = b.host.to(dev)
        if not b.on_device:
            return d_host, d_host[b.cut[-1]:].view(torch.float32).view(2, plan.n_rows, C)
        row_base = plan.group_row_base[b.group] + plan.row0
        zeros = self._dev("_pad_rows", lambda: torch.zeros((bitstream.ENCODE_ROW_ALIGN, C), dtype=torch.float32))
        pieces = [[], []]
        for f in np.argsort(row_base, kind="stable"):
            for which in (0, 1):
                pieces[which] += [b.pairs[f][which].detach().to(dev, torch.float32).reshape(-1, C),
                                  zeros[: -b.rows[f] % bitstream.ENCODE_ROW_ALIGN]]
        return d_host, torch.cat(pieces[0] + pieces[1]).view(2, plan.n_rows, C)

    def _batch_solve(self, b, lat):
        """Per distinct lambda one vbq_prep_planes_f32 and one solve of its files' rows into its planes of the one index array
        -> (idx u16 [C * R], canon u16 [C, T] or None: the map a batch coder applies when the table has repeated code points)."""
        plan, C = b.plan, self.num_channels
        idx = torch.empty(C * plan.n_rows, dtype=torch.uint16, device=lat.device)
        for t, key in enumerate(b.tables):
            r0, B = int(plan.group_row_base[t]), int(plan.group_rows[t])
            mu_cb, sg_cb = self._prep(lat[0, r0:r0 + B], lat[1, r0:r0 + B], spread="logvar")
            self._solve_idx(mu_cb, sg_cb, [key], self._level_len_dev([key]), out_idx=idx[C * r0:C * (r0 + B)].view(1, C, B))
        canon = None if self._strict else self._dev("canon_u16", lambda: torch.from_numpy(self._canon.astype(np.uint16)))
        return idx, canon

    def _encode_batch_run(self, b, d_host, lat):
        """The device side: per distinct lambda one vbq_prep_planes_f32 and one solve of its files' rows into its planes of the
        one index array, ONE vbq_rans_encode_files_u16, ONE vbq_rans_pack_u16 -> the payload u16 (its first `total` words are
        valid); total, sizes and status land in d_host[:b.back].  Nothing is read back."""
        from . import _lib
        plan, C, N, dev, segment = b.plan, self.num_channels, self.max_bits_per_coord, d_host.device, b.segment
        F, M, cut = len(b.keys), plan.M, b.cut
        d_total, d_sizes = d_host[:8].view(torch.uint64), d_host[8:8 + 4 * M].view(torch.uint32)
        d_status = d_host[8 + 4 * M:b.back].view(torch.uint32)
        d_files = d_host[cut[0]:cut[1]].view(torch.int64).view(F, 6)
        d_items = d_host[cut[1]:cut[2]].view(torch.int32).view(-1, 2)
        idx, canon = self._batch_solve(b, lat)
        freq = self._coder_stack(b.tables, segment)._freq(dev).view(len(b.tables), C, -1)
        words = torch.empty((M, segment + 2), dtype=torch.uint16, device=dev)      # pack reads valid words only
        payload = torch.empty(M * (segment + 2), dtype=torch.uint16, device=dev)
        offsets = torch.empty(M, dtype=torch.int64, device=dev)
        ops.rans_encode_files(idx, d_files, d_items, freq, M, seg=segment, N=N, canon=canon, words=words, sizes=d_sizes,
                              status=d_status)
        _lib.check(_lib.lib().vbq_rans_pack_u16(ops._ptr(words), ops._ptr(d_sizes), 1, M * segment, segment, ops._ptr(payload),
                                                ops._ptr(offsets), ops._ptr(d_total), ops._stream(words)), "vbq_rans_pack_u16")
        return payload

    def compress_to_bytes_batch(self, Xs, vae, lambs, segment=1024):
        """`vae.encode(X)` for every X of `Xs`, then compress_latents_to_bytes_batch."""
        return self.compress_latents_to_bytes_batch([vae.encode(X) for X in Xs], lambs, segment=segment)

    # ------------------------------------------------------------------ batches of compact files (include/vbq.h, "Compact batch")
    # The one-file calls give the interleaved coder one wave per part: a Kodak-shaped latent is three parts, so three waves run
    # and the call takes the time of one wave's steps.  Here the parts of all files of a batch run side by side, one launch
    # per step.  Nothing routes here implicitly: one file stays with compress_latents_to_bytes / decompress_latents.
    def compress_latents_to_compact_batch(self, latents, lambs, part=1 << 17):
        """[compress_latents_to_bytes(means_f, logvars_f, lambs[f], layout="interleaved", part=part) for f], byte for byte, with
        ONE sizes launch and ONE encode launch for all files.  `latents`, `lambs`, the errors and their order are those of
        compress_latents_to_bytes_batch, with `part` checked by bitstream.check_part; the table may have repeated code points.
        F == 0 returns [].
        Work per call, L the number of DISTINCT lambdas: the one staging buffer and upload of the batch encoder (the plan of
        bitstream.compact_plan, zeroed sizes and status words, the latents unless all are device tensors); per distinct
        lambda one vbq_prep_planes_f32 and one solve; ONE vbq_rans_il_sizes_files_u16 over every part of every file; the
        offsets by a device cumsum; ONE vbq_rans_il_encode_files_u16 into a payload buffer of the known upper bound,
        sum(C * B_f) + 128 * P_all words.  Two device-to-host copies: the part sizes and the status words, then the valid
        words.  The F files are assembled on the host (bitstream.CompactHeader / bitstream.write_compact)."""
        pairs, shapes, keys, part = self._batch_file_inputs(latents, lambs, part, "interleaved")
        return self._compact_batch(pairs, shapes, keys, part)

    def _compact_batch(self, pairs, shapes, keys, part, part_sizes=None):
        """The device side and the assembly of compress_latents_to_compact_batch, its inputs checked.  part_sizes: u32 [P_all]
        on the host, the words of every part of every file, file-major as bitstream.compact_plan lays them, from a caller
        that has sized the parts already (the budget calls: a row per file of the rate kernel's table).  Given, they ride in
        the front region of the staging buffer in the place of the zeros, and there is no vbq_rans_il_sizes_files_u16 launch:
        the encode kernel takes sizes and offsets as the caller's own and checks them for memory safety only."""
        from . import _lib
        F, C, N = len(pairs), self.num_channels, self.max_bits_per_coord
        if F == 0:
            return []
        tables = sorted(set(keys), key=float)                     # (a stable tag for the codec cache of _coder_stack)
        digests = {k: self._coder_tables(k)[1] for k in tables}
        rows = [int(np.prod(sh[:-1], dtype=np.int64)) for sh in shapes]
        plan = bitstream.compact_plan(rows, [tables.index(k) for k in keys], part, C, len(tables))
        P = plan.P_all
        b = self._batch_stage(plan, shapes, keys, tables, digests, part, rows, pairs, 4 * P + 4 * F)
        if part_sizes is not None:
            b.host.numpy()[:4 * P] = np.ascontiguousarray(part_sizes, dtype=np.uint32).reshape(P).view(np.uint8)
        d_host, lat = self._encode_batch_upload(b)
        d_sizes, d_status = d_host[:4 * P].view(torch.uint32), d_host[4 * P:b.back].view(torch.uint32)
        d_files = d_host[b.cut[0]:b.cut[1]].view(torch.int64).view(F, bitstream.COMPACT_FIELDS)
        d_items = d_host[b.cut[1]:b.cut[2]].view(torch.int32).view(-1, 2)
        idx, canon = self._batch_solve(b, lat)
        freq = self._coder_stack(tables, None)._freq(idx.device).view(len(tables), C, -1)
        if part_sizes is None:
            ops.rans_il_sizes_files(idx, d_files, d_items, freq, P, N=N, canon=canon, sizes=d_sizes, status=d_status)
        s64 = d_sizes.view(torch.int32).to(torch.int64)                                   # (a size is at most 2^24 + 128)
        payload = torch.empty(C * sum(rows) + bitstream.PART_STATE_WORDS * P, dtype=torch.uint16, device=idx.device)
        ops.rans_il_encode_files(idx, d_files, d_items, freq, d_sizes, torch.cumsum(s64, 0) - s64, payload, N=N, canon=canon,
                                 status=d_status)
        h = d_host[:b.back].cpu().numpy()
        sizes, status = h[:4 * P].view(np.uint32), h[4 * P:].view(np.uint32)
        for f in np.flatnonzero(status):
            raise _lib.VBQError(f"file {int(f)}: the batch encoder refused its descriptor (status {int(status[f])})")
        ends = np.cumsum(sizes, dtype=np.int64)
        pay = payload[:int(ends[-1])].cpu().numpy()
        out = []
        for f in range(F):
            p0, p1 = int(plan.part_base[f]), int(plan.part_base[f] + plan.n_parts[f])
            w0, w1 = int(ends[p0 - 1]) if p0 else 0, int(ends[p1 - 1])
            hd = bitstream.CompactHeader(N=N, C=C, shape=shapes[f], lamb=float(keys[f]), digest=digests[keys[f]],
                                         n_words=w1 - w0, part=part)
            out.append(bitstream.write_compact(hd, sizes[p0:p1], pay[w0:w1]))
        return out

    def compress_to_compact_batch(self, Xs, vae, lambs, part=1 << 17):
        """`vae.encode(X)` for every X of `Xs`, then compress_latents_to_compact_batch."""
        return self.compress_latents_to_compact_batch([vae.encode(X) for X in Xs], lambs, part=part)

    def _compact_headers(self, files):
        """The parsed headers of `files` with the checks of decompress_latents on each, (headers, sizes, payload offsets, keys);
        ValueError naming the index of a file that is no b"VBQc" file of this quantizer."""
        heads, sizes, starts, keys = [], [], [], []
        for i, data in enumerate(files):
            magic = bytes(memoryview(data).cast("B")[:4])
            foreign = {bitstream.MAGIC: "a file in segments (magic b'VBQb')",
                       bitstream.MAPPED_MAGIC: "a lambda-map file (magic b'VBQm')"}.get(magic)
            if foreign:
                raise ValueError(f"file {i} is {foreign}; compact batches read compact files (magic b'VBQc')")
            h, sz, start, key = self._batch_file_header(i, data, bitstream.parse_compact)
            heads.append(h), sizes.append(sz), starts.append(start), keys.append(key)
        return heads, sizes, starts, keys

    def decompress_latents_compact_batch(self, files, stack=True, return_np=False):
        """Many compact latent files decoded in full in ONE launch, every value bit-identical to decompress_latents(files[f]).
        `files`: b"VBQc" byte strings of this quantizer -- any built lambdas, any latent shapes, any `part` per file; each
        gets the checks of decompress_latents (ValueError naming the file's index, also for a b"VBQb" or b"VBQm" file;
        KeyError for a lambda without a model).  stack=True: one f32 [F, *shape]; ValueError naming the first file whose shape
        differs from file 0's.  stack=False: a list of F tensors, each shaped like its latents, all views of one allocation.
        F == 0 returns an empty tensor or list with no launch.
        Work per call: one staging buffer and ONE upload (descriptors, part offsets -- the exclusive sum of the part sizes,
        which the parser has validated, taken on the host --, items, all part sizes, all payloads), ONE
        vbq_rans_il_decode_files_u16 into the columns of one [C, sum B_f] index matrix, ONE gather of it into channel-last
        values, one read of the status words.  A damaged file raises VBQError naming the index of the first one."""
        from . import _lib, coder
        self._check_coder_bits()
        files = list(files)
        F, C, N = len(files), self.num_channels, self.max_bits_per_coord
        heads, sizes, starts, keys = self._compact_headers(files)
        if stack:
            for i, h in enumerate(heads):
                if h.shape != heads[0].shape:
                    raise ValueError(f"file {i} has latent shape {h.shape}, file 0 has {heads[0].shape}: stack=False returns "
                                     "a list")
        if F == 0:
            if not stack:
                return []
            out = torch.empty((0,), dtype=torch.float32, device=self.device)
            return out.cpu().numpy() if return_np else out
        dev = self.device
        tables = sorted(set(keys), key=float)                      # (a stable tag for the codec cache of _coder_stack)
        rows = [h.n_rows for h in heads]
        plan = bitstream.compact_plan(rows, [tables.index(k) for k in keys], [h.part for h in heads], C, len(tables))
        P, B = plan.P_all, int(sum(rows))
        desc = plan.files.copy()
        n_words_f = np.array([h.n_words for h in heads], np.int64)
        # the files side by side as columns of ONE [C, B] index matrix, so that one gather serves them all
        desc[:, 0], desc[:, 1] = np.cumsum(rows) - rows, B
        desc[:, 6], desc[:, 7] = np.cumsum(n_words_f) - n_words_f, n_words_f
        all_sizes = np.concatenate(sizes).astype(np.uint32)
        offsets = np.cumsum(all_sizes, dtype=np.int64) - all_sizes
        n_words = int(n_words_f.sum())
        raws = [np.frombuffer(memoryview(d).cast("B"), dtype=np.uint8) for d in files]
        head = [desc.view(np.uint8).reshape(-1), offsets.view(np.uint8), plan.items.view(np.uint8).reshape(-1),
                all_sizes.view(np.uint8), np.zeros(4 * (P & 1), np.uint8)]
        host = np.concatenate(head + [r[s: s + 2 * h.n_words] for r, h, s in zip(raws, heads, starts)])
        cut = [int(c) for c in np.cumsum([0] + [a.size for a in head])]
        d = torch.from_numpy(host).to(dev)
        d_files = d[cut[0]:cut[1]].view(torch.int64).view(F, bitstream.COMPACT_FIELDS)
        d_offsets = d[cut[1]:cut[2]].view(torch.int64)
        d_items = d[cut[2]:cut[3]].view(torch.int32).view(P, 2)
        d_sizes = d[cut[3]:cut[4]].view(torch.uint32)
        d_payload = d[cut[5]:cut[5] + 2 * n_words].view(torch.uint16)
        freq = self._coder_stack(tables, None)._freq(dev).view(len(tables), C, -1)
        idx = torch.empty((C, B), dtype=torch.uint16, device=dev)                       # every position lies in a listed part
        _, status = ops.rans_il_decode_files(d_payload, d_sizes, d_offsets, d_files, d_items, freq, idx, N=N)
        zhat = ops.gather(idx[None], self._sorted_dev(), C, N=N, layout="cb", out_layout="bc").view(B, C)
        st = status.cpu().numpy()
        for f in np.flatnonzero(st):
            try:
                coder._raise_status(int(st[f]))
            except _lib.VBQError as e:
                raise _lib.VBQError(f"file {int(f)}: {e}") from None
        if stack:
            out = zhat.view((F,) + heads[0].shape)
            return out.cpu().numpy() if return_np else out
        col = desc[:, 0]
        out = [zhat[int(col[f]): int(col[f]) + rows[f]].view(heads[f].shape) for f in range(F)]
        return [o.cpu().numpy() for o in out] if return_np else out

    # ------------------------------------------------------------------ lambda maps (vbq_amd.bitstream, magic b"VBQm")
    # A palette `lambs` of 1..4 distinct built lambdas and `classes`, integers in [0, P) shaped like the latents without the
    # channel axis: position b of every channel is quantized and coded at lambs[classes[b]].  The solve is independent per
    # latent and the decoder never needs lambda, so the result at (b, c) is exactly what compress_latents gives there for that
    # lambda; the coder switches the frequency table from symbol to symbol (coder.MappedRansCodec).
    def _map_inputs(self, posterior_means, lambs, classes):
        """(palette keys, classes as a NumPy u8 array [B]); ValueError for P outside 1..4, a repeated lambda, classes of the
        wrong shape or dtype or outside [0, P); KeyError for a lambda without a model."""
        lambs = list(lambs)
        if not 1 <= len(lambs) <= bitstream.MAX_CLASSES:
            raise ValueError(f"a palette of {len(lambs)} lambdas: need 1..{bitstream.MAX_CLASSES}")
        keys = [self._lambda_key(l) for l in lambs]
        if len(set(float(k) for k in keys)) != len(keys):
            raise ValueError(f"repeated lambda in the palette {lambs}")
        shape = tuple(int(d) for d in np.shape(posterior_means))
        cls = _to_numpy(classes)
        if cls.dtype.kind not in "iu":
            raise ValueError(f"classes must be integers, got {cls.dtype}")
        if tuple(cls.shape) != shape[:-1]:
            raise ValueError(f"classes of shape {tuple(cls.shape)}: the latents {shape} need {shape[:-1]}")
        if cls.size and (int(cls.min()) < 0 or int(cls.max()) >= len(keys)):
            raise ValueError(f"class outside [0, {len(keys)}): the palette has {len(keys)} lambdas")
        return keys, np.ascontiguousarray(cls.reshape(-1).astype(np.uint8))

    def _mapped_codec(self, keys, segment):
        """(MappedRansCodec over the tables of `keys`, their digests), cached as _coder_stack caches its codecs."""
        from .coder import MappedRansCodec
        digests = tuple(self._coder_tables(k, segment)[1] for k in keys)                       # refreshes the per-lambda cache
        per = self._dev_cache["_coder_tables"][2]
        hit = self._dev_cache.get("_coder_maps")
        if hit is None or hit[0] is not self._code_counts or hit[1] != self._add_n_smoothing:
            hit = self._dev_cache["_coder_maps"] = (self._code_counts, self._add_n_smoothing, {})
        codecs = hit[2]
        tag = (tuple(float(k) for k in keys), segment)
        codec = codecs.get(tag)
        if codec is None:
            if len(codecs) >= 8:
                codecs.clear()
            codec = codecs[tag] = MappedRansCodec(np.stack([per[k]["freq"] for k in keys]), N=self.max_bits_per_coord,
                                                  segment=segment)
        return codec, digests

    def compress_latents_mapped(self, posterior_means, posterior_logvars, lambs, classes, return_np=True):
        """{"Z_hat", "num_bits"} shaped like the latents: at position b, channel c exactly compress_latents(posterior_means,
        posterior_logvars, lambs)[...][lambs[classes[b]]] there -- one solve of the palette, then a per-position selection."""
        keys, cls = self._map_inputs(posterior_means, lambs, classes)
        shape = tuple(int(d) for d in np.shape(posterior_means))
        out = self.compress_latents(posterior_means, posterior_logvars, keys, return_np=False)
        pick = torch.from_numpy(cls).to(self.device, torch.int64).reshape((1,) + shape[:-1] + (1,)).expand((1,) + shape)
        res = {name: torch.gather(torch.stack([out[name][k] for k in keys]), 0, pick)[0] for name in ("Z_hat", "num_bits")}
        return {name: t.cpu().numpy() for name, t in res.items()} if return_np else res

    def _mapped_file_inputs(self, posterior_means, posterior_logvars, lambs, classes, segment):
        self._check_coder_bits()
        keys, cls = self._map_inputs(posterior_means, lambs, classes)
        shape, _, segment = self._file_layout(posterior_means, posterior_logvars, "segments", segment, None)
        codec, digests = self._mapped_codec(keys, segment)
        idx = self._file_indices(posterior_means, posterior_logvars, keys)                     # [P, C, B]
        return keys, cls, shape, segment, codec, digests, idx

    def compress_latents_to_bytes_mapped(self, posterior_means, posterior_logvars, lambs, classes, segment=1024) -> bytes:
        """compress_latents_mapped, entropy-coded into a self-describing byte string (vbq_amd.bitstream, magic b"VBQm").  One
        solve of the palette (the indices of compress_latents_to_bytes at each lambda); the mapped encoder reads symbol b of
        channel c straight out of plane classes[b] of that result with the table of (lambs[classes[b]], c); pack; two
        device-to-host copies.  decompress_latents reads the file.  ValueError for a palette outside 1..4 lambdas or with a
        repeat and for classes of the wrong shape or outside [0, P); KeyError for a lambda without a model."""
        keys, cls, shape, segment, codec, digests, idx = self._mapped_file_inputs(posterior_means, posterior_logvars, lambs,
                                                                                  classes, segment)
        sizes, payload = codec.encode_packed(idx, cls)
        h = bitstream.MappedHeader(N=self.max_bits_per_coord, C=self.num_channels, shape=shape, segment=segment,
                                   lambs=tuple(float(k) for k in keys), digests=digests, n_words=int(payload.size))
        return bitstream.write_mapped(h, cls, sizes, payload)

    def coded_nbytes_mapped(self, posterior_means, posterior_logvars, lambs, classes, segment=1024) -> int:
        """len(compress_latents_to_bytes_mapped(...)) for the same arguments, exact, without building the file: the solve,
        one vbq_rans_map_sizes_u16 launch (segment sizes only, no words), one copy of their total."""
        keys, cls, shape, segment, codec, _, idx = self._mapped_file_inputs(posterior_means, posterior_logvars, lambs, classes,
                                                                            segment)
        n_words = int(codec.sizes(idx, cls).view(torch.int32).sum(dtype=torch.int64).item())
        return bitstream.mapped_nbytes(shape, self.num_channels, segment, n_words, len(keys))

    def compress_to_bytes_mapped(self, X, vae, lambs, classes, segment=1024) -> bytes:
        """`vae.encode(X)`, then compress_latents_to_bytes_mapped; `classes` is at latent resolution."""
        posterior_means, posterior_logvars = vae.encode(X)
        return self.compress_latents_to_bytes_mapped(posterior_means, posterior_logvars, lambs, classes, segment=segment)

    # ------------------------------------------------------------------ batches of lambda maps, written (include/vbq.h, "Mapped
    # batch encode").  The one-file call gives a workgroup the 64 consecutive segments of one stream and up to four tables to
    # stage for them; here the segments of all files of a batch share workgroups, palette by palette.  Nothing routes here
    # implicitly: one file stays with compress_latents_to_bytes_mapped.
    _MappedBatch = namedtuple("_MappedBatch", "b groups palette_of cls max_classes")

    def _mapped_batch_plan(self, latents, lambs, classes, segment):
        """The host side of the mapped batch calls: every check of the one-file call per file (the file's index in the
        message), the plan of bitstream.mapped_encode_plan and the ONE staging buffer of _batch_stage with the palettes int32
        [G, 4] and the class bytes u8 [n_cls] after the items.  b.tables: the distinct lambdas of all palettes; groups: the
        distinct palettes as tuples of keys, in order of first use.  None when there is no file."""
        self._check_coder_bits()
        bitstream.check_segment(segment)
        segment = int(segment)
        pairs, classes, lambs = list(latents), list(classes), list(lambs)
        F, C = len(pairs), self.num_channels
        if len(classes) != F:
            raise ValueError(f"{len(classes)} class maps for {F} files")
        scalar = [np.ndim(l) == 0 for l in lambs]
        if all(scalar):
            palettes = [lambs] * F                                # one palette for all files
        elif any(scalar) or len(lambs) != F:
            raise ValueError(f"`lambs` must be one palette (a sequence of numbers) or a sequence of {F} palettes, one per file")
        else:
            palettes = lambs
        shapes = self._batch_file_shapes(pairs, segment)
        if F == 0:
            return None
        groups, palette_of, cls = [], [], []
        for f in range(F):
            try:
                keys, cl = self._map_inputs(pairs[f][0], palettes[f], classes[f])
            except ValueError as e:
                raise ValueError(f"file {f}: {e}") from None
            except KeyError as e:
                raise KeyError(f"file {f}: no entropy model for lambda {e.args[0]!r}") from None
            keys = tuple(keys)
            if keys not in groups:
                groups.append(keys)
            palette_of.append(groups.index(keys))
            cls.append(cl)
        tables = sorted({k for g in groups for k in g}, key=float)    # (a stable tag for the codec cache of _coder_stack)
        digests = {k: self._coder_tables(k, segment)[1] for k in tables}
        rows = [int(np.prod(sh[:-1], dtype=np.int64)) for sh in shapes]
        plan = bitstream.mapped_encode_plan(rows, palette_of, [len(g) for g in groups], segment, C)
        rows4 = plan.palettes.copy()
        for g, keys in enumerate(groups):
            rows4[g, :len(keys)] = [tables.index(k) for k in keys]
        cls_bytes = np.zeros(plan.n_cls, np.uint8)
        for f in range(F):
            cls_bytes[int(plan.cls_base[f]): int(plan.cls_base[f]) + rows[f]] = cls[f]
        b = self._batch_stage(plan, shapes, [groups[g] for g in palette_of], tables, digests, segment, rows, pairs,
                              8 + 4 * plan.M + 4 * F, group=np.asarray(palette_of, np.int64),
                              extra=(rows4.view(np.uint8).reshape(-1), cls_bytes))
        return self._MappedBatch(b, groups, palette_of, cls, max(len(g) for g in groups))

    def _mapped_batch_run(self, mb, d_host, lat, words: bool):
        """The device side, after the one upload (_encode_batch_upload(mb.b) -> d_host, lat): per distinct palette one
        vbq_prep_planes_f32 and one solve of its files' rows at its P lambdas into its [P, C, B_g] planes of the one index
        array, then ONE vbq_rans_map_encode_files_u16 and ONE vbq_rans_pack_u16 (words=True) or ONE
        vbq_rans_map_sizes_files_u16 -> the payload u16 or None; total, sizes and status land in d_host[:b.back].  Nothing is
        read back."""
        from . import _lib
        b = mb.b
        plan, C, N, segment, cut = b.plan, self.num_channels, self.max_bits_per_coord, b.segment, b.cut
        dev, F, M = d_host.device, len(b.keys), plan.M
        d_total, d_sizes = d_host[:8].view(torch.uint64), d_host[8:8 + 4 * M].view(torch.uint32)
        d_status = d_host[8 + 4 * M:b.back].view(torch.uint32)
        d_files = d_host[cut[0]:cut[1]].view(torch.int64).view(F, bitstream.MAPPED_ENCODE_FIELDS)
        d_items = d_host[cut[1]:cut[2]].view(torch.int32).view(-1, 2)
        d_palettes = d_host[cut[2]:cut[3]].view(torch.int32).view(-1, bitstream.MAX_CLASSES)
        d_cls = d_host[cut[3]:cut[4]]
        idx = torch.empty(plan.n_idx, dtype=torch.uint16, device=dev)
        for g, keys in enumerate(mb.groups):
            r0, B, P, i0 = int(plan.group_row_base[g]), int(plan.group_rows[g]), len(keys), int(plan.group_idx_base[g])
            mu_cb, sg_cb = self._prep(lat[0, r0:r0 + B], lat[1, r0:r0 + B], spread="logvar")
            self._solve_idx(mu_cb, sg_cb, list(keys), self._level_len_dev(list(keys)),
                            out_idx=idx[i0:i0 + P * C * B].view(P, C, B))
        canon = None if self._strict else self._dev("canon_u16", lambda: torch.from_numpy(self._canon.astype(np.uint16)))
        freq = self._coder_stack(b.tables, segment)._freq(dev).view(len(b.tables), C, -1)
        if not words:
            ops.rans_map_sizes_files(idx, d_cls, d_files, d_palettes, d_items, freq, M, seg=segment, max_classes=mb.max_classes,
                                     N=N, canon=canon, sizes=d_sizes, status=d_status)
            return None
        buf = torch.empty((M, segment + 2), dtype=torch.uint16, device=dev)           # pack reads valid words only
        payload = torch.empty(M * (segment + 2), dtype=torch.uint16, device=dev)
        offsets = torch.empty(M, dtype=torch.int64, device=dev)
        ops.rans_map_encode_files(idx, d_cls, d_files, d_palettes, d_items, freq, M, seg=segment, max_classes=mb.max_classes,
                                  N=N, canon=canon, words=buf, sizes=d_sizes, status=d_status)
        _lib.check(_lib.lib().vbq_rans_pack_u16(ops._ptr(buf), ops._ptr(d_sizes), 1, M * segment, segment, ops._ptr(payload),
                                                ops._ptr(offsets), ops._ptr(d_total), ops._stream(buf)), "vbq_rans_pack_u16")
        return payload

    def _mapped_batch_back(self, mb, d_host):
        """The first copy back -> (total, sizes u32 [M], the end of every file's words among all words int64 [F]); VBQError
        naming the file whose descriptor the kernel refused."""
        from . import _lib
        plan, M = mb.b.plan, mb.b.plan.M
        h = d_host[:mb.b.back].cpu().numpy()
        total, sizes, status = int(h[:8].view(np.uint64)[0]), h[8:8 + 4 * M].view(np.uint32), h[8 + 4 * M:].view(np.uint32)
        for f in np.flatnonzero(status):
            raise _lib.VBQError(f"file {int(f)}: the mapped batch encoder refused its descriptor (status {int(status[f])})")
        return total, sizes, np.cumsum(sizes, dtype=np.int64)[plan.seg_base + self.num_channels * plan.nseg - 1]

    def compress_latents_to_bytes_mapped_batch(self, latents, lambs, classes, segment=1024):
        """[compress_latents_to_bytes_mapped(means_f, logvars_f, lambs_f, classes[f], segment=segment) for f], byte for byte,
        with ONE encode launch for all files.  `latents`: F pairs as compress_latents_to_bytes_batch takes them (any shapes,
        NumPy or tensors, host or device).  `lambs`: one palette for all files (a sequence of 1..4 distinct built lambdas) or a
        sequence of F palettes; palettes are grouped as ordered tuples, so (a, b) and (b, a) are two groups.  `classes`: a
        sequence of F integer arrays, classes[f] shaped like file f's latents without the channel axis.  The table may have
        repeated code points (the canonical map is applied to the staged tables: no int64 gather).  F == 0 returns [].
        Errors are those of the one-file call, raised before any device work with the file's index in the message; also
        ValueError for len(classes) != F, for a wrong number of palettes and for more than 65535 files.
        Work per call, G the number of DISTINCT palettes: one staging buffer and one upload (the plan of
        bitstream.mapped_encode_plan, zeroed sizes and status words, descriptors, items, palettes, class bytes and -- for
        inputs that are not all device tensors -- the latents); per palette one vbq_prep_planes_f32 and one solve of its
        files' rows at its P lambdas; ONE vbq_rans_map_encode_files_u16; ONE vbq_rans_pack_u16 (two launches): 2 G + 3
        launches.  Two device-to-host copies: the total, all segment sizes and the status words, then the first `total`
        payload words.  The files are assembled on the host (bitstream.MappedHeader / bitstream.write_mapped)."""
        mb = self._mapped_batch_plan(latents, lambs, classes, segment)
        if mb is None:
            return []
        b, plan, C = mb.b, mb.b.plan, self.num_channels
        d_host, lat = self._encode_batch_upload(b)
        payload = self._mapped_batch_run(mb, d_host, lat, words=True)
        total, sizes, ends = self._mapped_batch_back(mb, d_host)
        pay = payload[:total].cpu().numpy()
        out = []
        for f, keys in enumerate(b.keys):
            n_words = int(ends[f] - (ends[f - 1] if f else 0))
            hd = bitstream.MappedHeader(N=self.max_bits_per_coord, C=C, shape=b.shapes[f], segment=b.segment,
                                        lambs=tuple(float(k) for k in keys), digests=tuple(b.digests[k] for k in keys),
                                        n_words=n_words)
            sz = sizes[int(plan.seg_base[f]): int(plan.seg_base[f] + C * plan.nseg[f])]
            out.append(bitstream.write_mapped(hd, mb.cls[f], sz, pay[int(ends[f]) - n_words: int(ends[f])]))
        return out

    def compress_to_bytes_mapped_batch(self, Xs, vae, lambs, classes, segment=1024):
        """`vae.encode(X)` for every X of `Xs`, then compress_latents_to_bytes_mapped_batch; `classes` at latent resolution."""
        return self.compress_latents_to_bytes_mapped_batch([vae.encode(X) for X in Xs], lambs, classes, segment=segment)

    def coded_nbytes_mapped_batch(self, latents, lambs, classes, segment=1024) -> list:
        """[coded_nbytes_mapped(means_f, logvars_f, lambs_f, classes[f], segment=segment) for f], exact, without building a
        file: the plan, the upload and the solves of compress_latents_to_bytes_mapped_batch, ONE
        vbq_rans_map_sizes_files_u16 (segment sizes only, no words) and one copy of the sizes and the status words back; the
        lengths come from bitstream.mapped_nbytes.  Arguments and errors as compress_latents_to_bytes_mapped_batch."""
        mb = self._mapped_batch_plan(latents, lambs, classes, segment)
        if mb is None:
            return []
        d_host, lat = self._encode_batch_upload(mb.b)
        self._mapped_batch_run(mb, d_host, lat, words=False)
        _, _, ends = self._mapped_batch_back(mb, d_host)
        n_words = np.diff(ends, prepend=0)
        return [bitstream.mapped_nbytes(mb.b.shapes[f], self.num_channels, mb.b.segment, int(n_words[f]), len(keys))
                for f, keys in enumerate(mb.b.keys)]

    # ------------------------------------------------------------------ byte budgets over lambda maps (include/vbq.h, "Mapped
    # batch rates").  The caller gives an ORDERED list of K candidate palettes, each of the same P distinct built lambdas
    # (bitstream.palette_ladder builds the usual one), and one class map per file; a budget call keeps the FIRST candidate of
    # the list whose exact file length fits -- palettes have no natural order, and no monotonicity is assumed.  Every distinct
    # lambda of the candidates is solved once and ONE launch sizes every file under every candidate.  Nothing routes here
    # implicitly.
    def _mapped_palettes_inputs(self, latents, palettes, classes, segment):
        """Every check of the calls below, before any device work -> (pairs, shapes, candidates as K tuples of P keys, the
        class maps as F u8 arrays, the class maps as given, segment)."""
        self._check_coder_bits()
        bitstream.check_segment(segment)
        pairs, classes = list(latents), list(classes)
        F, C = len(pairs), self.num_channels
        if len(classes) != F:
            raise ValueError(f"{len(classes)} class maps for {F} files")
        given = list(palettes)
        if not given:
            raise ValueError("no candidate palette to choose from")
        if any(np.ndim(p) != 1 for p in given):
            raise ValueError("`palettes` must be a sequence of candidate palettes, each a sequence of lambdas")
        nothing = (np.zeros((0, C), np.float32), np.zeros(0, np.int64))
        cands = []
        for k, pal in enumerate(given):
            if len(pal) != len(given[0]):
                raise ValueError(f"palette {k}: {len(pal)} lambdas, palette 0 has {len(given[0])}: the candidates of one call "
                                 "have one size")
            try:
                cands.append(tuple(self._map_inputs(nothing[0], pal, nothing[1])[0]))      # (the palette's own checks)
            except ValueError as e:
                raise ValueError(f"palette {k}: {e}") from None
            except KeyError as e:
                raise KeyError(f"palette {k}: no entropy model for lambda {e.args[0]!r}") from None
        shapes = self._batch_file_shapes(pairs, segment)
        cls = []
        for f in range(F):
            try:
                cls.append(self._map_inputs(pairs[f][0], cands[0], classes[f])[1])           # (the classes: P alone matters)
            except ValueError as e:
                raise ValueError(f"file {f}: {e}") from None
        return pairs, shapes, cands, cls, classes, int(segment)

    def _coded_nbytes_mapped_palettes(self, pairs, shapes, cands, cls, segment):
        """(nbytes int64 [F, K] with nbytes[f, k] = the exact lambda-map file length of latent f under cands[k], the F latents
        as pairs of device tensors shaped like the inputs): ONE plan with every file in one palette group
        (bitstream.mapped_encode_plan), ONE upload as the batch encoder's (zeroed totals u64 [K, F] and status u32 [F],
        descriptors, items, candidate rows, class bytes and -- unless every input is a device tensor -- the latents), one
        vbq_prep_planes_f32 of all R rows, then per chunk of candidates (bitstream.candidate_chunks with max(1,
        RATE_SCRATCH_BYTES // (2 C R)) tables) one solve of the chunk's distinct lambdas into [L_chunk, C, R] and ONE
        vbq_rans_map_rates_files_u16, and one copy of the totals and the status words back."""
        from . import _lib
        F, K, P, C, N, dev = len(pairs), len(cands), len(cands[0]), self.num_channels, self.max_bits_per_coord, self.device
        rows = [int(np.prod(sh[:-1], dtype=np.int64)) for sh in shapes]
        plan = bitstream.mapped_encode_plan(rows, [0] * F, [P], segment, C)
        R = plan.n_rows
        lambs = sorted({k for cand in cands for k in cand}, key=float)                         # the L distinct lambdas
        chunks = list(bitstream.candidate_chunks([[lambs.index(k) for k in cand] for cand in cands],
                                                 max(1, RATE_SCRATCH_BYTES // (2 * C * R))))
        rows4 = np.full((K, bitstream.MAX_CLASSES), -1, np.int32)                              # planes of the candidate's own chunk
        for k0, k1, tables in chunks:
            rows4[k0:k1, :P] = [[tables.index(lambs.index(k)) for k in cand] for cand in cands[k0:k1]]
        cls_bytes = np.zeros(plan.n_cls, np.uint8)
        for f in range(F):
            cls_bytes[int(plan.cls_base[f]): int(plan.cls_base[f]) + rows[f]] = cls[f]
        b = self._batch_stage(plan, shapes, cands, None, None, segment, rows, pairs, 8 * K * F + 4 * F,
                              group=np.zeros(F, np.int64), extra=(rows4.view(np.uint8).reshape(-1), cls_bytes))
        d_host, lat = self._encode_batch_upload(b)
        cut = b.cut
        d_totals = d_host[:8 * K * F].view(torch.uint64).view(K, F)
        d_status = d_host[8 * K * F:b.back].view(torch.uint32)
        d_files = d_host[cut[0]:cut[1]].view(torch.int64).view(F, bitstream.MAPPED_ENCODE_FIELDS)
        d_items = d_host[cut[1]:cut[2]].view(torch.int32).view(-1, 2)
        d_rows4 = d_host[cut[2]:cut[3]].view(torch.int32).view(K, bitstream.MAX_CLASSES)
        d_cls = d_host[cut[3]:cut[4]]
        canon = None if self._strict else self._dev("canon_u16", lambda: torch.from_numpy(self._canon.astype(np.uint16)))
        mu_cb, sg_cb = self._prep(lat[0], lat[1], spread="logvar")
        for k0, k1, tables in chunks:
            ks = [lambs[t] for t in tables]
            idx = self._solve_idx(mu_cb, sg_cb, ks, self._level_len_dev(ks))                   # [L_chunk, C, R]
            freq = self._coder_stack(ks, segment)._freq(dev).view(len(ks), C, -1)
            ops.rans_map_rates_files(idx.view(-1), d_cls, d_files, d_rows4[k0:k1], d_items, freq, lambda_stride=C * R,
                                     seg=segment, max_classes=P, N=N, canon=canon, totals=d_totals[k0:k1], status=d_status)
        h = d_host[:b.back].cpu().numpy()
        totals, status = h[:8 * K * F].view(np.uint64).reshape(K, F), h[8 * K * F:].view(np.uint32)
        for f in np.flatnonzero(status):
            raise _lib.VBQError(f"file {int(f)}: the mapped rates kernel refused its descriptor (status {int(status[f])})")
        nbytes = np.array([[bitstream.mapped_nbytes(shapes[f], C, segment, int(totals[k, f]), P) for k in range(K)]
                           for f in range(F)], dtype=np.int64).reshape(F, K)
        on_dev = [tuple(lat[w, int(plan.row0[f]):int(plan.row0[f]) + rows[f]].view(shapes[f]) for w in (0, 1)) for f in range(F)]
        return nbytes, on_dev

    def coded_nbytes_mapped_palettes_batch(self, latents, palettes, classes, segment=1024) -> np.ndarray:
        """int64 [F, K]: entry [f, k] == coded_nbytes_mapped(means_f, logvars_f, palettes[k], classes[f], segment=segment),
        exact, with every distinct lambda of the candidates solved ONCE and ONE vbq_rans_map_rates_files_u16 launch for all
        files and candidates (per chunk of candidates: see _coded_nbytes_mapped_palettes).  `latents`: F pairs as
        compress_latents_to_bytes_mapped_batch takes them; `palettes`: K >= 1 candidates, each a sequence of the same P
        (1..4) distinct built lambdas, in the caller's order -- (a, b) and (b, a) are two candidates; `classes`: F integer
        arrays in [0, P), classes[f] shaped like file f's latents without the channel axis.  F == 0 returns an empty [0, K]
        array.  Errors before any device work: those of compress_latents_to_bytes_mapped per candidate ("palette k: ...":
        a size outside 1..4, a repeated lambda; KeyError for a lambda without a model) and per file ("file f: ...": a bad
        shape pair, classes of the wrong shape or dtype or outside [0, P)); ValueError for candidates of unequal length, for no
        candidate, for len(classes) != F, for a bad `segment` and for more than 65535 files."""
        pairs, shapes, cands, cls, _, segment = self._mapped_palettes_inputs(latents, palettes, classes, segment)
        if not pairs:
            return np.zeros((0, len(cands)), np.int64)
        return self._coded_nbytes_mapped_palettes(pairs, shapes, cands, cls, segment)[0]

    def compress_latents_to_budget_mapped_batch(self, latents, max_bytes, palettes, classes, segment=1024) -> list:
        """F lambda-map files: file f is, byte for byte, compress_latents_to_bytes_mapped(means_f, logvars_f, palettes[k_f],
        classes[f], segment=segment) with k_f the FIRST candidate of `palettes` whose exact length is within the file's
        budget.  `max_bytes`: one integer >= 1 for all files or a sequence of F.  The lengths come from
        coded_nbytes_mapped_palettes_batch's one rates launch, the files from compress_latents_to_bytes_mapped_batch on the
        latents already on the device with every file's chosen palette (its solves cover only the chosen palettes).
        ValueError (bitstream.smallest_rates_within) naming the first file that no candidate fits, before anything is
        encoded.  F == 0 returns []."""
        budgets = bitstream.check_budgets(max_bytes)
        pairs, shapes, cands, cls, classes, segment = self._mapped_palettes_inputs(latents, palettes, classes, segment)
        if budgets is not None and len(budgets) != len(pairs):
            raise ValueError(f"{len(budgets)} budgets for {len(pairs)} files")
        if not pairs:
            return []
        nbytes, on_dev = self._coded_nbytes_mapped_palettes(pairs, shapes, cands, cls, segment)
        cols = bitstream.smallest_rates_within(nbytes, max_bytes if budgets is None else budgets, name="palette")
        return self.compress_latents_to_bytes_mapped_batch(on_dev, [list(cands[c]) for c in cols], classes, segment=segment)

    def compress_latents_to_total_budget_mapped(self, latents, max_total_bytes, palettes, classes, segment=1024):
        """(k, files): ONE candidate for all files -- the first of `palettes` under which the F files together take at most
        max_total_bytes -- and files == compress_latents_to_bytes_mapped_batch(latents, palettes[k], classes, segment).
        ValueError for no files, or naming the smallest achievable total and its candidate when nothing fits."""
        budget = bitstream.check_budget(max_total_bytes)
        pairs, shapes, cands, cls, classes, segment = self._mapped_palettes_inputs(latents, palettes, classes, segment)
        if not pairs:
            raise ValueError("no files: a total budget needs at least one")
        nbytes, on_dev = self._coded_nbytes_mapped_palettes(pairs, shapes, cands, cls, segment)
        sums = nbytes.sum(axis=0)
        fits = np.flatnonzero(sums <= budget)
        if not fits.size:
            raise ValueError(f"no palette fits in {budget} bytes in total: the smallest total is {int(sums.min())} bytes, at "
                             f"palette {int(np.argmin(sums))}")
        k = int(fits[0])
        return k, self.compress_latents_to_bytes_mapped_batch(on_dev, list(cands[k]), classes, segment=segment)

    def coded_nbytes_mapped_palettes(self, posterior_means, posterior_logvars, palettes, classes, segment=1024) -> list:
        """[coded_nbytes_mapped(posterior_means, posterior_logvars, p, classes, segment=segment) for p in palettes], K ints:
        coded_nbytes_mapped_palettes_batch for one file."""
        return [int(v) for v in self.coded_nbytes_mapped_palettes_batch([(posterior_means, posterior_logvars)], palettes,
                                                                        [classes], segment=segment)[0]]

    def compress_latents_to_budget_mapped(self, posterior_means, posterior_logvars, max_bytes, palettes, classes,
                                          segment=1024) -> bytes:
        """The lambda-map file of the first candidate of `palettes` whose exact length is <= max_bytes:
        compress_latents_to_budget_mapped_batch for one file."""
        bitstream.check_budget(max_bytes)
        return self.compress_latents_to_budget_mapped_batch([(posterior_means, posterior_logvars)], max_bytes, palettes,
                                                            [classes], segment=segment)[0]

    def compress_to_budget_mapped(self, X, vae, max_bytes, palettes, classes, segment=1024) -> bytes:
        """`vae.encode(X)`, then compress_latents_to_budget_mapped; `classes` is at latent resolution."""
        posterior_means, posterior_logvars = vae.encode(X)
        return self.compress_latents_to_budget_mapped(posterior_means, posterior_logvars, max_bytes, palettes, classes,
                                                      segment=segment)

    def compress_to_budget_mapped_batch(self, Xs, vae, max_bytes, palettes, classes, segment=1024) -> list:
        """`vae.encode(X)` for every X of `Xs`, then compress_latents_to_budget_mapped_batch; `classes` at latent resolution."""
        return self.compress_latents_to_budget_mapped_batch([vae.encode(X) for X in Xs], max_bytes, palettes, classes,
                                                            segment=segment)

    def _decompress_latents_mapped(self, data, return_np):
        """decompress_latents of a lambda-map file: the digest of every class, the mapped decoder, the gather."""
        h, classes, _, _ = bitstream.parse_mapped(data)
        if h.N != self.max_bits_per_coord or h.C != self.num_channels:
            raise ValueError(f"stream is for N = {h.N}, C = {h.C}; this quantizer has N = {self.max_bits_per_coord}, "
                             f"C = {self.num_channels}")
        keys = [self._lambda_key(l) for l in h.lambs]
        codec, digests = self._mapped_codec(keys, h.segment)
        if digests != h.digests:
            raise ValueError("stream was compressed with a different quantizer or entropy model (digest mismatch)")
        tail = np.frombuffer(memoryview(data).cast("B"), dtype="<u2", count=h.n_sizes + h.n_words, offset=h.sizes_offset)
        buf = torch.from_numpy(tail.copy()).to(self.device)                                 # sizes, then payload: one upload
        idx = codec.decode_packed(buf[h.n_sizes:], buf[: h.n_sizes], classes, h.n_rows)
        zhat = ops.gather(idx[None], self._sorted_dev(), self.num_channels, N=self.max_bits_per_coord, layout="cb",
                          out_layout="bc").reshape(h.shape)
        return zhat.cpu().numpy() if return_np else zhat

    # ------------------------------------------------------------------ rate control: exact lengths, byte budgets
    def _rate_keys(self, lambs):
        """The entropy-model keys of `lambs` (all of self.lambs when None), in order, each once; KeyError for an unknown one."""
        self._need_entropy_models()
        return list(dict.fromkeys(self.lambs if lambs is None else [self._lambda_key(l) for l in lambs]))

    def _coder_stack(self, keys, segment):
        """One codec over the L x C streams of `keys` (the per-lambda tables of _coder_tables, stacked).  Cached in a slot of its
        own, invalidated as _coder_tables is (a rebuild of the models) and holding the last few (lambdas, segment) asked for."""
        from .coder import RansCodec
        for k in keys:
            self._coder_tables(k, segment)                                                    # refreshes the per-lambda cache
        per = self._dev_cache["_coder_tables"][2]
        hit = self._dev_cache.get("_coder_stacks")
        if hit is None or hit[0] is not self._code_counts or hit[1] != self._add_n_smoothing:
            hit = self._dev_cache["_coder_stacks"] = (self._code_counts, self._add_n_smoothing, {})
        stacks = hit[2]
        tag = (tuple(float(k) for k in keys), segment)
        codec = stacks.get(tag)
        if codec is None:
            if len(stacks) >= 8:
                stacks.clear()
            codec = stacks[tag] = RansCodec(np.concatenate([per[k]["freq"] for k in keys]), N=self.max_bits_per_coord,
                                            segment=segment)
        return codec

    def coded_nbytes(self, posterior_means, posterior_logvars, lambs=None, segment=1024, layout="segments", part=1 << 17) -> dict:
        """{lambda: len(compress_latents_to_bytes(posterior_means, posterior_logvars, lambda, segment))} for every key of
        entropy_models in `lambs` (default: all of self.lambs), exact, without building a file: ONE solve of every lambda, one
        vbq_rans_sizes_u16 launch over the L x C streams (segment sizes only, no words), one copy of the L totals.  Inputs and
        errors as compress_latents_to_bytes (KeyError for a lambda without a model).  layout="interleaved": the lengths of the
        compact files -- one vbq_rans_il_sizes_u16 launch per lambda (a part never holds symbols of two lambdas)."""
        self._check_coder_bits()
        keys = self._rate_keys(lambs)
        shape, lay, unit = self._file_layout(posterior_means, posterior_logvars, layout, segment, part)
        idx = self._file_indices(posterior_means, posterior_logvars, keys)                     # [L, C, B]
        words = lay.words(self, keys, idx, unit).cpu().numpy()
        return {k: lay.nbytes(shape, self.num_channels, unit, int(w)) for k, w in zip(keys, words)}

    def compress_latents_to_budget(self, posterior_means, posterior_logvars, max_bytes, lambs=None, segment=1024,
                                   layout="segments", part=1 << 17) -> bytes:
        """The file of the numerically SMALLEST lambda of `lambs` (default: all of self.lambs) whose exact length is <= max_bytes
        (an integer >= 1), byte for byte compress_latents_to_bytes at that lambda; the header says which lambda it is.  A larger
        lambda usually, but not always, gives a smaller file: the rule takes no monotonicity for granted.  ValueError naming
        the smallest achievable length and its lambda when nothing fits."""
        bitstream.check_budget(max_bytes)
        nbytes = self.coded_nbytes(posterior_means, posterior_logvars, lambs, segment=segment, layout=layout, part=part)
        lamb = bitstream.smallest_rate_within(nbytes, max_bytes, "lambda")
        return self.compress_latents_to_bytes(posterior_means, posterior_logvars, lamb, segment=segment, layout=layout, part=part)

    def compress_to_budget(self, X, vae, max_bytes, lambs=None, segment=1024, layout="segments", part=1 << 17) -> bytes:
        """`vae.encode(X)`, then compress_latents_to_budget."""
        posterior_means, posterior_logvars = vae.encode(X)
        return self.compress_latents_to_budget(posterior_means, posterior_logvars, max_bytes, lambs=lambs, segment=segment,
                                               layout=layout, part=part)

    # ------------------------------------------------------------------ rate control for batches (include/vbq.h, "Batch sizes")
    def _rate_batch_inputs(self, latents, lambs, segment, layout="segments"):
        """Every check of the batch rate calls, before any device work: those of _batch_file_inputs for the files and of
        _rate_keys for the candidate lambdas -> (pairs, shapes, keys, segment); no lambda is looked up when there is no file.
        With layout "interleaved" `segment` is the part of the compact rate calls."""
        self._check_coder_bits()
        _LAYOUTS[layout].check(segment)
        pairs = list(latents)
        shapes = self._batch_file_shapes(pairs, segment, layout)
        keys = self._rate_keys(lambs) if pairs else []
        return pairs, shapes, keys, int(segment)

    def _coded_nbytes_batch(self, pairs, shapes, keys, segment):
        """(nbytes int64 [F, L] with nbytes[f, l] = the exact file length of latent f at keys[l], the F latents as pairs of
        device tensors shaped like the inputs): ONE plan with every file in table 0 (bitstream.encode_plan), ONE upload as the
        batch encoder's (zeroed totals u64 [L, F] and status u32 [F], descriptors, items and -- unless every input is a device
        tensor -- the latents), one vbq_prep_planes_f32 of all R rows, then per chunk of max(1, RATE_SCRATCH_BYTES // (2 C R))
        lambdas one solve into [L_chunk, C, R] and ONE vbq_rans_sizes_files_u16 with that chunk's tables, and one copy of the
        totals and the status words back."""
        from . import _lib
        F, L, C, N, dev = len(pairs), len(keys), self.num_channels, self.max_bits_per_coord, self.device
        rows = [int(np.prod(sh[:-1], dtype=np.int64)) for sh in shapes]
        plan = bitstream.encode_plan(rows, [0] * F, segment, C, 1)
        R = plan.n_rows
        b = self._batch_stage(plan, shapes, keys, None, None, segment, rows, pairs, 8 * L * F + 4 * F)
        d_host, lat = self._encode_batch_upload(b)
        d_status = d_host[8 * L * F:b.back].view(torch.uint32)
        d_files = d_host[b.cut[0]:b.cut[1]].view(torch.int64).view(F, 6)
        d_items = d_host[b.cut[1]:b.cut[2]].view(torch.int32).view(-1, 2)
        canon = None if self._strict else self._dev("canon_u16", lambda: torch.from_numpy(self._canon.astype(np.uint16)))
        mu_cb, sg_cb = self._prep(lat[0], lat[1], spread="logvar")
        chunk = max(1, RATE_SCRATCH_BYTES // (2 * C * R))
        for l0 in range(0, L, chunk):
            ks = keys[l0:l0 + chunk]
            idx = self._solve_idx(mu_cb, sg_cb, ks, self._level_len_dev(ks))                   # [L_chunk, C, R]
            freq = self._coder_stack(ks, segment)._freq(dev).view(len(ks), C, -1)
            ops.rans_sizes_files(idx.view(-1), d_files, d_items, freq, lambda_stride=C * R, seg=segment, N=N, canon=canon,
                                 totals=d_host[8 * l0 * F:8 * (l0 + len(ks)) * F].view(torch.uint64).view(len(ks), F),
                                 status=d_status)
        h = d_host[:b.back].cpu().numpy()
        totals, status = h[:8 * L * F].view(np.uint64).reshape(L, F), h[8 * L * F:].view(np.uint32)
        for f in np.flatnonzero(status):
            raise _lib.VBQError(f"file {int(f)}: the batch sizes kernel refused its descriptor (status {int(status[f])})")
        nbytes = np.array([[bitstream.latent_nbytes(shapes[f], C, segment, int(totals[l, f])) for l in range(L)]
                           for f in range(F)], dtype=np.int64).reshape(F, L)
        row_base = plan.row0                                      # (one table: its group starts at row 0)
        on_dev = [tuple(lat[w, int(row_base[f]):int(row_base[f]) + rows[f]].view(shapes[f]) for w in (0, 1)) for f in range(F)]
        return nbytes, on_dev

    def coded_nbytes_batch(self, latents, lambs=None, segment=1024) -> list:
        """[coded_nbytes(means_f, logvars_f, lambs, segment=segment) for f]: a list of F dicts {lambda: exact file length}, the
        same keys in the same order, with ONE solve and ONE vbq_rans_sizes_files_u16 launch for all files and lambdas (per
        chunk of lambdas: see _coded_nbytes_batch).  `latents` as compress_latents_to_bytes_batch takes them; files in
        segments only.  F == 0 returns [].  Errors before any device work: those of compress_latents_to_bytes_batch for the
        files (ValueError naming the file's index), KeyError for a lambda without a model."""
        pairs, shapes, keys, segment = self._rate_batch_inputs(latents, lambs, segment)
        if not pairs:
            return []
        nbytes, _ = self._coded_nbytes_batch(pairs, shapes, keys, segment)
        return [{k: int(b) for k, b in zip(keys, row)} for row in nbytes]

    def compress_latents_to_budget_batch(self, latents, max_bytes, lambs=None, segment=1024) -> list:
        """[compress_latents_to_budget(means_f, logvars_f, max_bytes[f], lambs, segment=segment) for f], byte for byte:
        every file at the numerically smallest lambda of `lambs` whose exact length is within the file's budget.  `max_bytes`:
        one integer >= 1 for all files or a sequence of F.  The lengths come from coded_nbytes_batch's one sizes launch, the
        files from compress_latents_to_bytes_batch at the chosen lambdas on the latents already on the device (its solve
        covers only the chosen lambdas).  ValueError (bitstream.smallest_rates_within) naming the first file that no lambda
        fits, before anything is encoded.  F == 0 returns []."""
        budgets = bitstream.check_budgets(max_bytes)
        pairs, shapes, keys, segment = self._rate_batch_inputs(latents, lambs, segment)
        if budgets is not None and len(budgets) != len(pairs):
            raise ValueError(f"{len(budgets)} budgets for {len(pairs)} files")
        if not pairs:
            return []
        nbytes, on_dev = self._coded_nbytes_batch(pairs, shapes, keys, segment)
        order = sorted(range(len(keys)), key=lambda j: float(keys[j]))          # columns in ascending order of lambda
        cols = bitstream.smallest_rates_within(nbytes[:, order], max_bytes if budgets is None else budgets,
                                               rates=[float(keys[j]) for j in order])
        return self.compress_latents_to_bytes_batch(on_dev, [keys[order[c]] for c in cols], segment=segment)

    def compress_latents_to_total_budget(self, latents, max_total_bytes, lambs=None, segment=1024):
        """(lamb, files): ONE lambda for all files -- the numerically smallest of `lambs` at which the F files together take
        at most max_total_bytes (bitstream.smallest_rate_within on the column sums of the length table) -- and
        files == compress_latents_to_bytes_batch(latents, lamb, segment).  ValueError for no files, or naming the smallest
        achievable total and its lambda when nothing fits."""
        bitstream.check_budget(max_total_bytes)
        pairs, shapes, keys, segment = self._rate_batch_inputs(latents, lambs, segment)
        if not pairs:
            raise ValueError("no files: a total budget needs at least one")
        nbytes, on_dev = self._coded_nbytes_batch(pairs, shapes, keys, segment)
        lamb = bitstream.smallest_rate_within(dict(zip(keys, nbytes.sum(axis=0))), max_total_bytes, "lambda")
        return lamb, self.compress_latents_to_bytes_batch(on_dev, lamb, segment=segment)

    def compress_to_budget_batch(self, Xs, vae, max_bytes, lambs=None, segment=1024) -> list:
        """`vae.encode(X)` for every X of `Xs`, then compress_latents_to_budget_batch."""
        return self.compress_latents_to_budget_batch([vae.encode(X) for X in Xs], max_bytes, lambs=lambs, segment=segment)

    # ------------------------------------------------------------------ rate control for batches of compact files (include/vbq.h,
    # "Compact batch", vbq_rans_il_rates_files_u16).  The four calls above, for the compact file: `part` in the place of
    # `segment`.  A sizes pass of the interleaved coder costs about what the encode costs, so the writers hand the part sizes
    # the rate kernel computed to _compact_batch and nothing is sized twice.  Nothing routes here implicitly.
    def _coded_nbytes_compact_batch(self, pairs, shapes, keys, part):
        """(nbytes int64 [F, L] with nbytes[f, l] = the exact compact file length of latent f at keys[l], the F latents as
        pairs of device tensors shaped like the inputs, the part sizes u32 [L, P_all] on the host, the plan): ONE plan with
        every file in table 0 (bitstream.compact_plan), ONE upload as the batch encoder's (zeroed sizes u32 [L, P_all] and
        status u32 [F], descriptors, items and -- unless every input is a device tensor -- the latents), one
        vbq_prep_planes_f32 of all R rows, then per chunk of max(1, RATE_SCRATCH_BYTES // (2 C R)) lambdas one solve into
        [L_chunk, C, R] and ONE vbq_rans_il_rates_files_u16 with that chunk's tables, and one copy of the sizes and the
        status words back."""
        from . import _lib
        F, L, C, N, dev = len(pairs), len(keys), self.num_channels, self.max_bits_per_coord, self.device
        rows = [int(np.prod(sh[:-1], dtype=np.int64)) for sh in shapes]
        plan = bitstream.compact_plan(rows, [0] * F, part, C, 1)
        R, P = plan.n_rows, plan.P_all
        b = self._batch_stage(plan, shapes, keys, None, None, part, rows, pairs, 4 * L * P + 4 * F)
        d_host, lat = self._encode_batch_upload(b)
        d_status = d_host[4 * L * P:b.back].view(torch.uint32)
        d_files = d_host[b.cut[0]:b.cut[1]].view(torch.int64).view(F, bitstream.COMPACT_FIELDS)
        d_items = d_host[b.cut[1]:b.cut[2]].view(torch.int32).view(-1, 2)
        canon = None if self._strict else self._dev("canon_u16", lambda: torch.from_numpy(self._canon.astype(np.uint16)))
        mu_cb, sg_cb = self._prep(lat[0], lat[1], spread="logvar")
        chunk = max(1, RATE_SCRATCH_BYTES // (2 * C * R))
        for l0 in range(0, L, chunk):
            ks = keys[l0:l0 + chunk]
            idx = self._solve_idx(mu_cb, sg_cb, ks, self._level_len_dev(ks))                   # [L_chunk, C, R]
            freq = self._coder_stack(ks, None)._freq(dev).view(len(ks), C, -1)
            ops.rans_il_rates_files(idx.view(-1), d_files, d_items, freq, P, lambda_stride=C * R, N=N, canon=canon,
                                    sizes=d_host[4 * l0 * P:4 * (l0 + len(ks)) * P].view(torch.uint32).view(len(ks), P),
                                    status=d_status)
        h = d_host[:b.back].cpu().numpy()
        sizes, status = h[:4 * L * P].view(np.uint32).reshape(L, P), h[4 * L * P:].view(np.uint32)
        for f in np.flatnonzero(status):
            raise _lib.VBQError(f"file {int(f)}: the compact rate kernel refused its descriptor (status {int(status[f])})")
        words = bitstream.compact_file_words(sizes, plan)                                      # [L, F]
        nbytes = np.array([[bitstream.compact_nbytes(shapes[f], C, part, int(words[l, f])) for l in range(L)]
                           for f in range(F)], dtype=np.int64).reshape(F, L)
        row_base = plan.row0                                      # (one table: its group starts at row 0)
        on_dev = [tuple(lat[w, int(row_base[f]):int(row_base[f]) + rows[f]].view(shapes[f]) for w in (0, 1)) for f in range(F)]
        return nbytes, on_dev, sizes, plan

    @staticmethod
    def _chosen_part_sizes(sizes, plan, cols):
        """The part sizes u32 [P_all] of every file at its own lambda: file f's block from row cols[f] of sizes [L, P_all]."""
        return sizes[np.repeat(np.asarray(cols, np.int64), plan.n_parts), np.arange(plan.P_all)]

    def coded_nbytes_compact_batch(self, latents, lambs=None, part=1 << 17) -> list:
        """[coded_nbytes(means_f, logvars_f, lambs, layout="interleaved", part=part) for f]: a list of F dicts {lambda: exact
        compact file length}, the same keys in the same order, with ONE solve and ONE vbq_rans_il_rates_files_u16 launch for
        all files and lambdas (per chunk of lambdas: see _coded_nbytes_compact_batch).  `latents` as
        compress_latents_to_compact_batch takes them.  F == 0 returns [].  Errors before any device work: those of
        compress_latents_to_compact_batch for the files (ValueError naming the file's index; `part` by bitstream.check_part),
        KeyError for a lambda without a model."""
        pairs, shapes, keys, part = self._rate_batch_inputs(latents, lambs, part, "interleaved")
        if not pairs:
            return []
        nbytes = self._coded_nbytes_compact_batch(pairs, shapes, keys, part)[0]
        return [{k: int(b) for k, b in zip(keys, row)} for row in nbytes]

    def compress_latents_to_compact_budget_batch(self, latents, max_bytes, lambs=None, part=1 << 17) -> list:
        """[compress_latents_to_budget(means_f, logvars_f, max_bytes[f], lambs, layout="interleaved", part=part) for f], byte
        for byte: every file at the numerically smallest lambda of `lambs` whose exact length is within the file's budget.
        `max_bytes`: one integer >= 1 for all files or a sequence of F.  The lengths come from
        coded_nbytes_compact_batch's one rate launch; the files from the compact batch writer at the chosen lambdas on the
        latents already on the device, with the part sizes the rate launch computed at those lambdas: its solve covers only
        the chosen lambdas and it runs no sizes launch.  ValueError (bitstream.smallest_rates_within) naming the first file
        that no lambda fits, before anything is encoded.  F == 0 returns []."""
        budgets = bitstream.check_budgets(max_bytes)
        pairs, shapes, keys, part = self._rate_batch_inputs(latents, lambs, part, "interleaved")
        if budgets is not None and len(budgets) != len(pairs):
            raise ValueError(f"{len(budgets)} budgets for {len(pairs)} files")
        if not pairs:
            return []
        nbytes, on_dev, sizes, plan = self._coded_nbytes_compact_batch(pairs, shapes, keys, part)
        order = sorted(range(len(keys)), key=lambda j: float(keys[j]))          # columns in ascending order of lambda
        cols = bitstream.smallest_rates_within(nbytes[:, order], max_bytes if budgets is None else budgets,
                                               rates=[float(keys[j]) for j in order])
        chosen = [order[c] for c in cols]
        return self._compact_batch(on_dev, shapes, [keys[j] for j in chosen], part, self._chosen_part_sizes(sizes, plan, chosen))

    def compress_latents_to_compact_total_budget(self, latents, max_total_bytes, lambs=None, part=1 << 17):
        """(lamb, files): ONE lambda for all files -- the numerically smallest of `lambs` at which the F files together take
        at most max_total_bytes (bitstream.smallest_rate_within on the column sums of the length table) -- and
        files == compress_latents_to_compact_batch(latents, lamb, part), written without a second sizes launch.  ValueError
        for no files, or naming the smallest achievable total and its lambda when nothing fits."""
        bitstream.check_budget(max_total_bytes)
        pairs, shapes, keys, part = self._rate_batch_inputs(latents, lambs, part, "interleaved")
        if not pairs:
            raise ValueError("no files: a total budget needs at least one")
        nbytes, on_dev, sizes, plan = self._coded_nbytes_compact_batch(pairs, shapes, keys, part)
        lamb = bitstream.smallest_rate_within(dict(zip(keys, nbytes.sum(axis=0))), max_total_bytes, "lambda")
        return lamb, self._compact_batch(on_dev, shapes, [lamb] * len(pairs), part, sizes[keys.index(lamb)])

    def compress_to_compact_budget_batch(self, Xs, vae, max_bytes, lambs=None, part=1 << 17) -> list:
        """`vae.encode(X)` for every X of `Xs`, then compress_latents_to_compact_budget_batch."""
        return self.compress_latents_to_compact_budget_batch([vae.encode(X) for X in Xs], max_bytes, lambs=lambs, part=part)

    def decompress(self, data, vae, clip=True, return_np=True):
        """decompress_latents, then `vae.decode` and the clip to [0, 1] of compress (quantizer.py:251-253).  The decoder
        receives the latents as a device tensor; the image comes back as NumPy unless return_np=False."""
        Z = self.decompress_latents(data, return_np=False)
        X_hat = vae.decode(Z)
        if isinstance(X_hat, torch.Tensor):
            X_hat = X_hat.detach()
            if clip:
                X_hat = X_hat.clamp(0, 1)
            return X_hat.cpu().numpy() if return_np else X_hat
        X_hat = _to_numpy(X_hat)
        return np.clip(X_hat, 0, 1) if clip else X_hat

    def compress(self, X, vae, lambs, clip=True):
        """quantizer.py:242-256.  With a torch VAE on the device nothing crosses PCIe here: the decoder gets the Z_hat tensor the
        kernels wrote (the reference -- and this method before round 5 -- went through NumPy: a device-to-host copy of L latent
        tensors and the same bytes back for `vae.decode`), and 'X_hat' comes back as lazy views like the other quantities."""
        from .lazy import DeviceStack, LazyArray, common_stack, join
        lambs = list(lambs)
        L = len(lambs)
        posterior_means, posterior_logvars = vae.encode(X)
        output = self.compress_latents(posterior_means, posterior_logvars, lambs)
        Z_hat_dict = output["Z_hat"]
        latent_shape = tuple(np.shape(posterior_means))
        z_dev = common_stack([Z_hat_dict[lamb] for lamb in lambs]) if isinstance(posterior_means, torch.Tensor) else None
        if z_dev is not None:
            Z_flat = z_dev.reshape((-1,) + latent_shape[1:])                          # len(lambs) * batch x latent shape[1:]
            if Z_flat.device != posterior_means.device:
                Z_flat = Z_flat.to(posterior_means.device)
        else:
            Z_hat_batch = np.stack([Z_hat_dict[lamb] for lamb in lambs])             # len(lambs) x latent shape
            Z_flat = Z_hat_batch.reshape((-1,) + latent_shape[1:])
            if isinstance(posterior_means, torch.Tensor):
                Z_flat = torch.from_numpy(Z_flat).to(posterior_means.device)
        X_hat = vae.decode(Z_flat)
        if isinstance(X_hat, torch.Tensor) and X_hat.is_cuda:
            X_hat_batch = X_hat.detach().reshape((L,) + tuple(np.shape(X)))
            if clip:
                X_hat_batch = X_hat_batch.clamp(0, 1)                                  # np.clip(X_hat_batch, 0, 1), :253
            xs = DeviceStack("X_hat", X_hat_batch.contiguous(), self._stager())
            if isinstance(Z_hat_dict[lambs[0]], LazyArray):
                join(Z_hat_dict[lambs[0]], xs)                                     # a quantity of THIS call (the prefetch rule)
            output["X_hat"] = dict(zip(lambs, xs.rows()))
            return output
        X_hat_batch = _to_numpy(X_hat).reshape((L,) + tuple(np.shape(X)))
        if clip:
            X_hat_batch = np.clip(X_hat_batch, 0, 1)
        output["X_hat"] = {lamb: X_hat_batch[i] for i, lamb in enumerate(lambs)}
        return output
