"""Element-axis sharding across the GPUs of one node (one process per GPU, RCCL over xGMI).

Every (mu, sigma) element is solved independently (utils.py:401 is a per-element argmax), so
the rows are split contiguously across ranks and the only exchange of the whole pipeline is the
sum of the per-rank histograms (quantizer.py:104-105,138-140) and moment accumulators
(ipynb:374): integer / f64 all-reduces of a few hundred KB to a few tens of MB.  Integer sums
make the resulting entropy models independent of the number of ranks.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist


def init_from_env(backend: Optional[str] = None):
    """Initialise torch.distributed from RANK / WORLD_SIZE / LOCAL_RANK / MASTER_*; returns
    (rank, world, device).  backend "nccl" is RCCL on ROCm; "gloo" is used on CPU-only hosts."""
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC only on this driver (RCCL across processes)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    use_gpu = torch.cuda.is_available()
    device = torch.device("cuda", local) if use_gpu else torch.device("cpu")
    if use_gpu:
        torch.cuda.set_device(local)
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        dist.init_process_group(backend or ("nccl" if use_gpu else "gloo"), rank=rank, world_size=world)
    return rank, world, device


def shard_rows(n_rows: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous [start, stop) of this rank's rows; sizes differ by at most one."""
    base, rem = divmod(n_rows, world)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)


def allreduce_sum_(t: torch.Tensor, group=None) -> torch.Tensor:
    """In-place SUM over ranks (no-op without an initialised process group)."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t


def global_counts(local_counts: torch.Tensor, group=None) -> torch.Tensor:
    """int64 [L, C, T] rank histograms -> global histogram on every rank."""
    assert local_counts.dtype == torch.int64
    return allreduce_sum_(local_counts, group)


def global_empirical_std(local_moments: torch.Tensor, n_local: int, group=None) -> np.ndarray:
    """f64 [C, 2] = (sum x, sum x^2) of this shard -> sqrt(mean x^2) per channel over all shards
    (ipynb:374 computed globally)."""
    buf = torch.cat([local_moments.reshape(-1), torch.tensor([float(n_local)], dtype=torch.float64,
                                                             device=local_moments.device)])
    allreduce_sum_(buf, group)
    m = buf[:-1].reshape(local_moments.shape).cpu().numpy()
    return np.sqrt(m[:, 1] / float(buf[-1].item()))


def entropy_models_from_local_counts(local_counts: torch.Tensor, N: int, add_n_smoothing=1, group=None):
    """The collective + finish of build_entropy_models for one pass: returns
    (raw_length_models f32 [L, C, N+1], code_point_models f32 [L, C, T]) computed from the
    GLOBAL histogram; identical on every rank and for every world size."""
    from . import entropy
    g = global_counts(local_counts.clone(), group)
    raw = entropy.neg_log2_freq(entropy.level_counts_from_counts(g, N), add_n_smoothing)
    full = entropy.neg_log2_freq(g, add_n_smoothing)
    return raw, full


class Communicator:
    """The C-ABI's own RCCL communicator (vbq_comm_* / vbq_allreduce_hist, include/vbq.h): what a binder WITHOUT
    torch.distributed uses for the histogram exchange.  Rank 0 creates the 128-byte id (`Communicator.unique_id()`)
    and hands it to the other ranks by any means (a file, MPI, a socket); every rank then constructs the
    communicator with its GPU current.  The torch.distributed path above remains what the Python host uses."""

    def __init__(self, n_ranks: int, rank: int, unique_id: bytes):
        import ctypes as C
        from . import _lib
        if len(unique_id) != _lib.COMM_ID_BYTES:
            raise ValueError(f"unique_id must be {_lib.COMM_ID_BYTES} bytes")
        self._h = _lib.lib()
        self._comm = C.c_void_p()
        buf = C.create_string_buffer(unique_id, _lib.COMM_ID_BYTES)
        _lib.check(self._h.vbq_comm_init(C.byref(self._comm), int(n_ranks), buf, int(rank)), "vbq_comm_init")
        self.n_ranks, self.rank = int(n_ranks), int(rank)

    @staticmethod
    def unique_id() -> bytes:
        import ctypes as C
        from . import _lib
        buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
        _lib.check(_lib.lib().vbq_comm_unique_id(buf), "vbq_comm_unique_id")
        return buf.raw

    def all_reduce_(self, counts: torch.Tensor) -> torch.Tensor:
        """In-place SUM of an int32 / int64 device tensor over the ranks, asynchronous on the current stream."""
        from . import _lib, ops
        if counts.dtype not in (torch.int32, torch.int64) or not counts.is_cuda or not counts.is_contiguous():
            raise ValueError("counts must be a contiguous int32 / int64 device tensor")
        _lib.check(self._h.vbq_allreduce_hist(self._comm, ops._ptr(counts), counts.numel(), int(counts.dtype == torch.int32),
                                              ops._stream(counts)), "vbq_allreduce_hist")
        return counts

    def close(self):
        from . import _lib
        if self._comm:
            _lib.check(self._h.vbq_comm_destroy(self._comm), "vbq_comm_destroy")
            self._comm = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


PACKED_FIELD_LIMIT = 1 << 21


class CountsAllReduce:
    """SUM all-reduce of an int32 histogram [L, C, T] with fewer bytes on the wire.

    While every global count is below 2^21 three counters travel in one int64 word (vbq_pack_counts_3x21): the SUM
    of the words is the field-wise sum, 2.67 instead of 4 bytes per bin -- the difference between a communication-
    bound and a compute-bound step on two GPUs joined by a single xGMI link.  Otherwise the int32 tensor is reduced
    as it is.  `start()` is asynchronous (the collective overlaps later kernels); `wait()` leaves the global counts
    in the tensor given to `start()`.

    The packed path is chosen from the caller's `max_global_count` (an upper bound of any global bin, e.g. the
    global number of rows per channel) and GUARDED on the device: the pack kernel raises a flag when a local count
    reaches 2^21 / world, the flag travels in a spare word of the same all-reduce (so every rank sees the same
    answer), and `check()` -- one device-to-host read, call it outside the timed loop, or `wait(check=True)` --
    raises VBQError when any rank flagged: the sums of that step cannot be trusted then (use packed=False).
    The guard is CONSERVATIVE: a rank that holds more than 1 / world of a bin flags although the global sum may still be
    below 2^21 (unbalanced shards); the error then costs a retry with packed=False, never a wrong count.
    `EntropyModelBuild.check()` calls it after a build.
    """

    def __init__(self, numel: int, device, max_global_count: int, group=None, packed: Optional[bool] = None):
        self.group = group
        fits = max_global_count < PACKED_FIELD_LIMIT and device.type == "cuda"
        self.packed = fits if packed is None else (bool(packed) and device.type == "cuda")
        self.numel = int(numel)
        self.nw = (numel + 2) // 3
        # word nw carries the overflow flags of all ranks (their sum)
        self.words = torch.zeros(self.nw + 1, dtype=torch.int64, device=device) if self.packed else None
        self._work = None
        self._counts = None

    @staticmethod
    def _require_group(group):
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("CountsAllReduce needs an initialised torch.distributed process group "
                               "(vbq_amd.dist.init_from_env())")
        return dist.get_world_size(group)

    def payload_bytes(self, counts: torch.Tensor) -> int:
        return self.words.numel() * 8 if self.packed else counts.numel() * counts.element_size()

    def start(self, counts: torch.Tensor):
        from . import _lib, ops
        world = self._require_group(self.group)
        if self.packed:                   # wait() unpacks the sums into this tensor: it is checked as any tensor the library writes
            counts = ops._out(counts, "any", torch.int32, self.words.device, "counts", False, (("words", self.words),))
            if counts is None or counts.numel() != self.numel:
                raise ValueError(f"counts: expected a contiguous {torch.int32} device tensor of {self.numel} elements")
        else:
            assert counts.dtype == torch.int32 and counts.is_contiguous()
        self._counts = counts
        if self.packed:
            self.words[self.nw:].zero_()
            _lib.check(_lib.lib().vbq_pack_counts_3x21(ops._ptr(counts), counts.numel(), ops._ptr(self.words), world,
                                                       ops._ptr(self.words[self.nw:]), ops._stream(counts)), "vbq_pack_counts_3x21")
            self._work = dist.all_reduce(self.words, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        else:
            self._work = dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        return self

    def wait(self, check: bool = False):
        from . import _lib, ops
        if self._work is None:
            return
        self._work.wait()                 # the compute stream now waits for the collective
        if self.packed:
            c = self._counts
            _lib.check(_lib.lib().vbq_unpack_counts_3x21(ops._ptr(self.words), c.numel(), ops._ptr(c), ops._stream(c)),
                       "vbq_unpack_counts_3x21")
        self._work = None
        if check:
            self.check()

    def check(self):
        """Raise if, in the most recent packed reduce, any rank held a count that could have carried into the
        neighbouring field (synchronises: one 8-byte read)."""
        from ._lib import VBQError
        if self.packed and int(self.words[self.nw].item()) != 0:
            raise VBQError("packed 3x21-bit histogram all-reduce overflowed: a local count reached 2^21 / world_size; "
                           "the reduced counts of that step are invalid -- use CountsAllReduce(..., packed=False)")
