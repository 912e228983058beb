"""Write footprints: buffers whose surroundings show a store that left the output it was given.

The oracle tests compare an output tensor and nothing else.  A fresh torch.empty sits in a caching allocator's block, rounded
up and packed next to other tensors, so a stray store lands in slack nobody reads; one element past plane c is the first
element of plane c + 1, which its own workgroup overwrites.  Here every output lives in ONE allocation laid out as

    guard | offset | payload | guard

filled end to end with a bit pattern no kernel of this library produces (CANARY).  After the call the guards -- and, with
assert_only, the part of the payload the call had no business in -- must still hold it.  Guards are ordinary memory of the same
allocation: nothing here is placed against the end of a mapping and nothing is meant to fault; the check is the comparison
after the call.  Patterns are compared through integer views only (the float ones are NaNs).

COVERED / EXEMPT say, for every function of include/vbq.h, which tests of tests/test_gpu_write_footprint.py guard its outputs or
why none does; tests/test_write_footprint_host.py holds them against the header.  Importable without a GPU."""
import numpy as np
import torch

# ------------------------------------------------------------------------------------------------------------------ canaries
U8_CANARIES = (0xA5, 0x5A)          # one byte value can be a legitimate output: every u8 case runs with each
_NP = {torch.uint8: np.uint8, torch.uint16: np.uint16, torch.int16: np.int16, torch.uint32: np.uint32, torch.int32: np.int32,
       torch.uint64: np.uint64, torch.int64: np.int64, torch.float32: np.float32, torch.float64: np.float64}
_PATTERN = {1: 0xA5, 2: 0xABCD, 4: 0xA5C3E1D2, 8: 0xA5C3E1D2A5C3E1D2}      # u16: above every rank index (T <= 8191)
_FLOAT_PATTERN = {torch.float32: 0x7FA5C3E1, torch.float64: 0x7FF4A5C3E1D2B697}      # NaN payloads


def canary(dtype, u8=U8_CANARIES[0]):
    """The canary of `dtype` as an unsigned integer (its bit pattern)."""
    if dtype in _FLOAT_PATTERN:
        return _FLOAT_PATTERN[dtype]
    size = np.dtype(_NP[dtype]).itemsize
    return int(u8) if size == 1 else _PATTERN[size]


def _uint(itemsize):
    return {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[itemsize]


class Guarded:
    """guard | offset | payload | guard in one flat allocation, all canary.

    view            the contiguous payload of `shape` and `dtype` (what vbq_amd.ops._out accepts)
    offset_elems    elements between the aligned base and the payload: 1 gives a base with element alignment only
    align           alignment of the base the offset counts from (256: what the caller workspaces of include/vbq.h ask for)
    guard_bytes     canary bytes on either side (rounded up to 8)
    fill(a)         the payload := a (accumulating outputs start from a known pattern that is not the canary)
    host()          the payload as a NumPy array
    """

    def __init__(self, shape, dtype, device="cpu", offset_elems=0, guard_bytes=1024, u8_canary=U8_CANARIES[0], align=256):
        self.shape = tuple(int(s) for s in (shape if hasattr(shape, "__len__") else (shape,)))
        self.dtype = dtype
        self.np_dtype = np.dtype(_NP[dtype])
        self.itemsize = self.np_dtype.itemsize
        self.pattern = canary(dtype, u8_canary)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.itemsize
        guard = -(-int(guard_bytes) // 8) * 8
        total = guard + align + offset_elems * self.itemsize + self.nbytes + guard + 8
        total = -(-total // 8) * 8
        self.raw = torch.empty(total, dtype=torch.uint8, device=device)
        base = self.raw.data_ptr()
        assert base % 8 == 0
        pad = (-(base + guard)) % align
        self.start = guard + pad + offset_elems * self.itemsize          # byte offset of the payload inside raw
        self.lead = guard + offset_elems * self.itemsize                  # canary bytes checked before the payload
        self.trail = guard
        self.end = self.start + self.nbytes
        assert self.end + self.trail <= total and self.start % self.itemsize == 0
        one = np.array([self.pattern], _uint(self.itemsize)).view(np.uint8)
        self.raw.copy_(torch.from_numpy(np.tile(one, total // self.itemsize)))
        self.view = self.raw[self.start:self.end].view(dtype).view(self.shape)
        self.ptr = base + self.start                                      # (an empty view has no data pointer of its own)
        assert self.view.is_contiguous() and (self.nbytes == 0 or self.view.data_ptr() == self.ptr)
        assert (self.ptr - offset_elems * self.itemsize) % align == 0

    # ---- the payload
    def fill(self, a):
        a = np.ascontiguousarray(a, self.np_dtype)
        assert a.shape == self.shape
        self.raw[self.start:self.end].copy_(torch.from_numpy(a.reshape(-1).view(np.uint8).copy()))
        return self

    def host(self):
        return self.raw[self.start:self.end].cpu().numpy().view(self.np_dtype).reshape(self.shape)

    def bits(self):
        """The payload as unsigned integers of its element size."""
        return self.raw[self.start:self.end].cpu().numpy().view(_uint(self.itemsize)).reshape(self.shape)

    # ---- the checks
    def _expect(self, nbytes, phase):
        one = np.array([self.pattern], _uint(self.itemsize)).view(np.uint8)
        return np.tile(one, nbytes // self.itemsize + 2)[phase:phase + nbytes]

    def assert_outside_intact(self, what=""):
        """Both guards (the offset gap included) still hold the canary; otherwise AssertionError naming the byte offset of the
        first damaged guard byte relative to the payload (negative: before it; >= its byte count: after it) and its value."""
        a = self.start - self.lead
        before = self.raw[a:self.start].cpu().numpy()
        after = self.raw[self.end:self.end + self.trail].cpu().numpy()
        for got, first in ((before, a), (after, self.end)):
            bad = np.flatnonzero(got != self._expect(got.size, first % self.itemsize))
            if bad.size:
                at = first + int(bad[0]) - self.start
                raise AssertionError(f"{what}: write outside the output: byte offset {at} relative to the payload "
                                     f"({self.nbytes} bytes of {self.np_dtype.name} {self.shape}) holds 0x{int(got[bad[0]]):02x}; "
                                     f"{bad.size} guard bytes damaged")

    def assert_only(self, mask, what=""):
        """Payload elements outside the boolean `mask` (broadcast to the shape) still hold the canary."""
        mask = np.broadcast_to(np.asarray(mask, bool), self.shape)
        bits = self.bits()
        bad = np.argwhere(~mask & (bits != _uint(self.itemsize)(self.pattern)))
        if bad.size:
            at = tuple(int(i) for i in bad[0])
            raise AssertionError(f"{what}: write outside the documented region of the output: element {at} of "
                                 f"{self.np_dtype.name} {self.shape} holds 0x{int(bits[at]):x}; {len(bad)} elements damaged")

    def assert_untouched(self, what=""):
        self.assert_outside_intact(what)
        self.assert_only(np.zeros(self.shape, bool), what)


def guarded_workspace(nbytes, device="cpu", align=256, u8_canary=U8_CANARIES[0]):
    """A caller workspace of EXACTLY `nbytes` bytes (what a vbq_*_workspace_bytes function returned) at the alignment the header
    states, canary before and after: .view is the u8 tensor to pass, .assert_outside_intact() the check."""
    return Guarded((int(nbytes),), torch.uint8, device, 0, 1024, u8_canary, align)


def shifted(a, offset_elems, device="cpu"):
    """A device copy of the array whose base lies `offset_elems` elements past a 256-byte boundary (an input with element
    alignment only)."""
    a = np.ascontiguousarray(a)
    dtype = {np.dtype(v): k for k, v in _NP.items()}[a.dtype]
    return Guarded(a.shape, dtype, device, offset_elems, 64).fill(a).view          # the view's storage is the allocation


# ------------------------------------------------------------------------------------------------------------------ coverage
NO_WRITE, HOST, COMM = "writes no device memory", "host function", "communicator / multi-GPU"
UNTOUCHED, TOO_LARGE = "untouched-region test exists: ", "smallest reaching shape exceeds memory"
EXEMPT_REASONS = (NO_WRITE, HOST, COMM, UNTOUCHED, TOO_LARGE)
"""The closed set of reasons.  UNTOUCHED is followed by `<module>::<test>` and is open to the *_files_u16 and *_window_f32
batch entry points only; TOO_LARGE is for an instance no test can afford, not for an entry point (EXEMPT_INSTANCES)."""

_SOLVE = ["test_fast_kernel_indices_only", "test_fast_kernel_with_zhat_and_lengths", "test_pruned_kernel",
          "test_hull_index_kernel", "test_fast_kernel_other_depths", "test_literal_flat_kernel", "test_literal_tiled_kernel",
          "test_solve_workspace_is_exactly_what_was_asked_for"]
_REDUCE = ["test_small_outputs_of_the_reductions"]
_SEGMENT, _IL, _MAPPED = ["test_segment_coder"], ["test_interleaved_coder"], ["test_mapped_coder"]
_HIST = ["test_histogram_adds_into_its_rows_of_bins"]

COVERED = {
    "vbq_quantize_f32": _SOLVE,
    "vbq_quantize_rows_f32": ["test_row_ranges_leave_the_other_rows_alone", "test_row_ranges_channel_last",
                              "test_solve_workspace_is_exactly_what_was_asked_for"],
    "vbq_level_counts_f32": ["test_level_counts", "test_solve_workspace_is_exactly_what_was_asked_for"],
    "vbq_n_bit_intervals_f32": ["test_n_bit_intervals"],
    "vbq_check_inputs_f32": _REDUCE, "vbq_index_max_u16": _REDUCE, "vbq_moments_f32": _REDUCE, "vbq_rd_sums_u16": _REDUCE,
    "vbq_numpy_sum_sq_f32": _REDUCE, "vbq_numpy_row_sums_f32": _REDUCE,
    "vbq_code_lengths_from_counts": ["test_code_lengths_from_counts"],
    "vbq_histogram_u16": _HIST, "vbq_histogram_u16_i32": _HIST, "vbq_histogram_rows_u16": _HIST,
    "vbq_histogram_models_u16": ["test_histogram_models_assigns"],
    "vbq_transpose_f32": ["test_transpose", "test_control_an_overrun_into_the_guard_is_caught"],
    "vbq_transpose_planes": ["test_transpose"],
    "vbq_prep_planes_f32": ["test_prep_planes"],
    "vbq_gather_f32": ["test_gather"],
    "vbq_gather_latents_u16": ["test_gather_latents", "test_lookup_from_the_lds"],
    "vbq_compress_latents_f32": ["test_compress_latents_in_an_exact_workspace"],
    "vbq_build_entropy_models_f32": ["test_build_entropy_models_in_an_exact_workspace"],
    "vbq_quantize_notebook_f64": ["test_notebook_kernels"],
    "vbq_argmax_candidates_f32": ["test_argmax_candidates"],
    "vbq_xi_intervals_f64": ["test_xi_intervals_and_select"], "vbq_xi_select_f64": ["test_xi_intervals_and_select"],
    "vbq_uniform_quantize_f32": ["test_comparison_quantizers"], "vbq_nearest_code_f64": ["test_comparison_quantizers"],
    "vbq_bmshj_cdf_pdf_f32": ["test_bmshj_kernels"], "vbq_bmshj_icdf_step_f32": ["test_bmshj_kernels"],
    "vbq_bmshj_icdf_chain_f32": ["test_bmshj_kernels"], "vbq_bmshj_nll_grad_f32": ["test_bmshj_kernels"],
    "vbq_analogy_ranks_f32": ["test_image_metrics"], "vbq_image_sqerr_u8": ["test_image_metrics"],
    "vbq_ssim_scale_f64": ["test_image_metrics"], "vbq_downsample2_f64": ["test_image_metrics"],
    "vbq_u8_to_f64": ["test_pixel_conversions"], "vbq_unit_to_u8_f32": ["test_pixel_conversions"],
    "vbq_pack_counts_3x21": ["test_packed_counters"], "vbq_unpack_counts_3x21": ["test_packed_counters"],
    "vbq_rans_encode_u16": _SEGMENT, "vbq_rans_sizes_u16": _SEGMENT, "vbq_rans_decode_u16": _SEGMENT,
    "vbq_rans_pack_u16": _SEGMENT, "vbq_rans_unpack_u16": _SEGMENT, "vbq_rans_segment_offsets_u16": _SEGMENT,
    "vbq_rans_decode_values_f32": _SEGMENT,
    "vbq_rans_il_sizes_u16": _IL, "vbq_rans_il_encode_u16": _IL, "vbq_rans_il_decode_u16": _IL,
    "vbq_rans_map_encode_u16": _MAPPED, "vbq_rans_map_sizes_u16": _MAPPED, "vbq_rans_map_decode_u16": _MAPPED,
    "vbq_budget_dp_f64": ["test_budget_dp"], "vbq_budget_patience_f64": ["test_budget_patience"],
    "vbq_records_pack_u16": ["test_records_pack_and_unpack"], "vbq_records_unpack_f32": ["test_records_pack_and_unpack"],
    "vbq_records_topk_f32": ["test_topk"], "vbq_topk_f32": ["test_topk"],
    "vbq_records_bag_f32": ["test_bags"], "vbq_bag_f32": ["test_bags"],
    "vbq_rans_decode_window_f32": ["test_window_decodes"], "vbq_rans_map_decode_window_f32": ["test_window_decodes"],
    "vbq_rans_encode_files_u16": ["test_batch_encode_of_segment_files"],
    "vbq_rans_sizes_files_u16": ["test_batch_encode_of_segment_files"],
    "vbq_rans_map_encode_files_u16": ["test_batch_encode_of_mapped_files"],
    "vbq_rans_map_sizes_files_u16": ["test_batch_encode_of_mapped_files"],
    "vbq_rans_map_rates_files_u16": ["test_batch_encode_of_mapped_files"],
    "vbq_rans_il_sizes_files_u16": ["test_batch_of_compact_files"], "vbq_rans_il_encode_files_u16": ["test_batch_of_compact_files"],
    "vbq_rans_il_decode_files_u16": ["test_batch_of_compact_files"], "vbq_rans_il_rates_files_u16": ["test_batch_of_compact_files"],
}
"""C entry point -> the tests of tests/test_gpu_write_footprint.py that put its outputs (and workspace) behind guards."""

EXEMPT = {
    "vbq_abi_version": NO_WRITE, "vbq_last_error": NO_WRITE, "vbq_solve_grid": NO_WRITE, "vbq_device_count": NO_WRITE,
    "vbq_device_name": NO_WRITE, "vbq_records_words": NO_WRITE,
    "vbq_quantize_workspace_bytes": NO_WRITE, "vbq_numpy_sum_sq_workspace_bytes": NO_WRITE,
    "vbq_numpy_row_sums_workspace_bytes": NO_WRITE, "vbq_compress_latents_workspace_bytes": NO_WRITE,
    "vbq_build_entropy_models_workspace_bytes": NO_WRITE, "vbq_analogy_ranks_workspace_bytes": NO_WRITE,
    "vbq_ssim_scale_workspace_bytes": NO_WRITE, "vbq_budget_dp_workspace_bytes": NO_WRITE, "vbq_topk_workspace_bytes": NO_WRITE,
    "vbq_host_neg_log2_freq_f32": HOST, "vbq_host_stage_run": HOST,
    "vbq_comm_unique_id": COMM, "vbq_comm_init": COMM, "vbq_allreduce_hist": COMM, "vbq_comm_destroy": COMM,
}
"""C entry point -> why no test guards it (one of EXEMPT_REASONS)."""

EXEMPT_INSTANCES = {"k_quant_hull_idx<BUF = false>": TOO_LARGE}
"""Kernel instances (not entry points) left out: K1e without the buffer descriptor serves planes of more than 4 GB."""
