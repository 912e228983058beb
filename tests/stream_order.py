"""Every call is ordered on the caller's stream: the late-input harness and the tables of what runs in it.

Every entry point of include/vbq.h takes a stream and every wrapper passes torch's current stream of the tensor's device; the
Python host keeps state of its own across calls (lazy results, captured graphs, a side stream of the model build, cached
tables and workspaces).  A test that runs a call on a side stream and compares passes when a launch is misrouted: the misrouted
kernel still finds finished inputs.  Here THE INPUTS ARRIVE LATE.  `run_late(call, fresh, stale, blocking=...)`:

1. the reference, on the default stream: call(fresh) and call(stale), each after one warm-up call (lazy initialisation, table
   uploads and graph captures stay out of the timing); t_ref is the host wall time of the fresh one.  The two answers must differ (bit patterns / quantizer_histories.same) -- a case on which they agree
   cannot tell the orders apart and FAILS;
2. device buffers filled with `stale`; one warm-up call on them under the side stream (its allocator pool, the uploads and
   captures of the object under test); the device is synchronized;
3. on a side stream s: a spin kernel of delay_ms(t_ref) (torch.cuda._sleep, calibrated once per module by `calibrate`), an
   event `armed` behind it, device-to-device copies of `fresh` into the same buffers, then call(buffers) while s is current;
4. blocking=False (calls that return device tensors or lazy views): `armed` must not have completed when the call returns --
   the call did not synchronize, and the delay was still running while all of its work was enqueued.  A case that is not armed
   fails;
5. still under s the results are read; s is synchronized; the answer must equal the fresh reference exactly.

Whatever part of the call runs on another stream -- the null stream, a private stream without a wait, a graph launched
elsewhere -- does not wait for the delay, reads `stale`, and the answer differs.  Stale inputs are another seeded draw of the
same shapes, dtypes and valid ranges (never garbage, canaries or NaN): a wrong order shows as a wrong value, never as a fault.

BLOCKING CALLS (bytes, NumPy arrays, Python integers) have to read the device.  They get the same late inputs and the same
comparison but no arming assertion: such a call may synchronize before its first launch (an input scan), and from then on
the delay is over and THE HARNESS IS BLIND for the rest of the call.  What covers the C side of those calls is the static
stream discipline of the sources (tests/test_stream_order_host.py): every launch, memset and copy of vbq_amd/csrc names the
caller's stream, and every Python call site passes ops._stream(...) at the header's stream position.

The harness never waits on a flag the host releases later, never sets a delay above CAP_MS, opens at most three streams of its
own, and starts no threads or processes.

LATE / HOST class every probe of quantizer_histories.PROBES; BY_SOURCE gives, for every vbq_amd/csrc/*.hip, the cases of
tests/test_gpu_stream_order.py that go through an entry point defined in it (and which), or why none does.  A NEW PROBE GOES
INTO LATE OR HOST, A NEW .hip FILE GETS A ROW IN BY_SOURCE.  Importable without a GPU."""
import time

import numpy as np

import quantizer_histories as QH

CAP_MS = 400.0
FLOOR_MS = 20.0
"""At least 4 x the largest t_ref an asynchronous case showed on an MI355X: 0.80 ms (tests/test_gpu_stream_order.py records
the figures); 20 ms also outlasts a host thread that loses its time slice on a shared machine."""
SLACK = 4.0
STALE_SEED = 1907


# ------------------------------------------------------------------------------------------------------------------ the delay
def delay_ms(t_ref_ms):
    """max(FLOOR, 4 x t_ref), capped.  The 4 x is slack for host jitter, measured against the reference on the default stream."""
    return min(CAP_MS, max(FLOOR_MS, SLACK * float(t_ref_ms)))


def fits_cap(t_ref_ms):
    """An asynchronous case whose 4 x t_ref exceeds the cap has inputs that are too large."""
    return SLACK * float(t_ref_ms) <= CAP_MS


def cycles_per_ms(c1, ms1, c2, ms2):
    """The slope of two timed spins (the intercept is launch overhead); ValueError when the two do not order as their cycle
    counts do -- the spin is then no clock."""
    if not (c2 > c1 > 0 and ms2 > ms1 > 0):
        raise ValueError(f"spins of {c1} and {c2} cycles took {ms1:.3f} and {ms2:.3f} ms")
    return (c2 - c1) / (ms2 - ms1)


class Spin:
    """A bounded delay on a stream: torch.cuda._sleep scaled by a calibration, or -- where that is no stable clock -- a chain of
    large device copies sized by the same calibration."""

    def __init__(self, kind, per_ms, buf=None):
        self.kind, self.per_ms, self.buf = kind, per_ms, buf

    def enqueue(self, ms):
        import torch
        assert 0 < ms <= CAP_MS, ms
        if self.kind == "sleep":
            torch.cuda._sleep(int(ms * self.per_ms))
        else:
            a, b = self.buf
            for _ in range(max(1, int(round(ms * self.per_ms)))):
                b.copy_(a, non_blocking=True)

    def __repr__(self):
        return f"Spin({self.kind}, {self.per_ms:.4g} per ms)"


def _timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def calibrate(target_ms=20.0):
    """-> (Spin, the measurements as text).  Two cycle counts timed with events give cycles per millisecond; a spin of
    target_ms is then timed and must come out within a factor of 2, else the copy chain is calibrated the same way."""
    import torch
    torch.cuda._sleep(1000)
    notes = []
    try:
        c1, c2 = 100_000, 1_000_000
        m1, m2 = (min(_timed(lambda: torch.cuda._sleep(c)) for _ in range(3)) for c in (c1, c2))
        per = cycles_per_ms(c1, m1, c2, m2)
        got = _timed(lambda: torch.cuda._sleep(int(target_ms * per)))
        notes.append(f"_sleep: {c1} cycles {m1:.3f} ms, {c2} cycles {m2:.3f} ms, {per:.0f} cycles/ms; {target_ms} ms asked, {got:.2f} ms")
        if 0.5 * target_ms <= got <= 2.0 * target_ms:
            return Spin("sleep", per * target_ms / got), "; ".join(notes)
    except ValueError as e:
        notes.append(f"_sleep: {e}")
    a = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    chain = lambda n: [b.copy_(a, non_blocking=True) for _ in range(n)]
    chain(4)
    n1, n2 = 8, 64
    m1, m2 = (min(_timed(lambda: chain(n)) for _ in range(3)) for n in (n1, n2))
    per = cycles_per_ms(n1, m1, n2, m2)
    notes.append(f"copy chain of 64 MiB: {n1} copies {m1:.3f} ms, {n2} copies {m2:.3f} ms, {per:.2f} copies/ms")
    return Spin("copies", per, (a, b)), "; ".join(notes)


# ------------------------------------------------------------------------------------------------------------------ input sets
def _map(f, x):
    """An input set is a tensor or a nest of lists, tuples and dicts of them; anything else (None, numbers) is kept."""
    if isinstance(x, (list, tuple)):
        return type(x)(_map(f, v) for v in x)
    if isinstance(x, dict):
        return {k: _map(f, v) for k, v in x.items()}
    return f(x) if hasattr(x, "data_ptr") or isinstance(x, np.ndarray) else x


def _leaves(x):
    out = []
    _map(lambda t: out.append(t) or t, x)
    return out


def to_device(x):
    """A nest of NumPy arrays as the same nest of device tensors."""
    import torch
    if isinstance(x, (list, tuple)):
        return type(x)(to_device(v) for v in x)
    if isinstance(x, dict):
        return {k: to_device(v) for k, v in x.items()}
    return torch.from_numpy(np.ascontiguousarray(x)).cuda() if isinstance(x, np.ndarray) else x


def bits(a):
    """An outcome with every float array replaced by its bit pattern: -0.0 and 0.0 differ, a NaN equals itself."""
    if isinstance(a, tuple):
        return tuple(bits(x) for x in a)
    if isinstance(a, np.ndarray) and a.dtype.kind in "fc":
        return np.ascontiguousarray(a).view({2: np.uint16, 4: np.uint32, 8: np.uint64, 16: np.uint64}[a.dtype.itemsize])
    return a


def plain(v):
    """What a call returned as nested tuples of bytes, ints and NumPy arrays (device tensors and lazy views are read here)."""
    return bits(QH._plain(v))


def check_recipe(fresh, stale):
    """The two input sets have the same structure, shapes and dtypes, differ in value, and the floating ones are finite."""
    f, s = _leaves(fresh), _leaves(stale)
    assert len(f) == len(s) and len(f) > 0, (len(f), len(s))
    differ = False
    for a, b in zip(f, s):
        assert tuple(a.shape) == tuple(b.shape) and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
        an, bn = (QH._plain(t) if hasattr(t, "cpu") else np.asarray(t) for t in (a, b))
        if an.dtype.kind == "f":
            assert np.isfinite(an).all() and np.isfinite(bn).all()
        differ = differ or an.tobytes() != bn.tobytes()
    assert differ, "the stale inputs equal the fresh ones"


# ------------------------------------------------------------------------------------------------------------------ the harness
class Late:
    """What run_late measured: the fresh and stale references, the late answer, what the call returned, t_ref and the delay in ms."""

    def __init__(self, want_fresh, want_stale, got, out, t_ref_ms, delay, armed):
        self.want_fresh, self.want_stale, self.got, self.out = want_fresh, want_stale, got, out
        self.t_ref_ms, self.delay, self.armed = t_ref_ms, delay, armed


T_REF = {}
"""case -> (t_ref in ms, blocking): what the module's report prints."""


def reference(call, inputs, read=plain, reset=None):
    """The answer on the default stream after one warm-up call, and the host wall time of the second call in ms."""
    import torch
    if reset is not None:
        reset()
    read(call(inputs))
    if reset is not None:
        reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = read(call(inputs))
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def run_late(call, fresh, stale, *, blocking, spin, name=None, reference_call=None, read=plain, warm=True, stream=None,
             compare=True, reset=None):
    """See the module docstring.  call(inputs) -> results; `fresh` / `stale`: input sets of device tensors.
    reference_call: what computes the references (default: `call` itself); warm: one call(buffers) under the side stream while
    the buffers hold `stale`, before the delay, so that the late call uploads, allocates and captures nothing; stream: the
    side stream to use (default: a new one); reset: puts accumulating outputs the call was given back to their start (before
    every call that is compared).  -> Late; with compare=False the comparison with want_fresh is left to the caller (the control)."""
    import torch
    ref = call if reference_call is None else reference_call
    check_recipe(fresh, stale)
    want_fresh, t_ref = reference(ref, fresh, read, reset)
    want_stale, _ = reference(ref, stale, read, reset)
    assert not QH.same(want_fresh, want_stale), f"{name}: fresh and stale inputs give the same answer: change the recipe"
    if name is not None:
        T_REF[name] = (t_ref, blocking)
    if not blocking:
        assert fits_cap(t_ref), f"{name}: t_ref {t_ref:.2f} ms: 4 x t_ref exceeds the cap of {CAP_MS} ms, shrink the inputs"
    delay = delay_ms(t_ref)
    buffers = _map(lambda t: t.clone(), stale)
    s = torch.cuda.Stream() if stream is None else stream
    if warm:
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            read(call(buffers))
    if reset is not None:
        reset()
    torch.cuda.synchronize()
    armed = torch.cuda.Event()
    with torch.cuda.stream(s):
        spin.enqueue(delay)
        armed.record(s)
        for b, f in zip(_leaves(buffers), _leaves(fresh)):
            b.copy_(f, non_blocking=True)
        out = call(buffers)
        was_armed = not armed.query()
        if not blocking:
            assert was_armed, (f"{name}: not armed -- the call synchronized with the device, or took longer to enqueue than the "
                               f"delay of {delay:.1f} ms (t_ref {t_ref:.2f} ms)")
        got = read(out)
    s.synchronize()
    if compare:
        assert QH.same(got, want_fresh), f"{name}: the answer under the delayed stream is not the fresh one" + \
            (" (it is the stale one)" if QH.same(got, want_stale) else "")
    return Late(want_fresh, want_stale, got, out, t_ref, delay, was_armed)


def run_delayed(call, want, *, spin, name=None, read=plain, ms=None):
    """A call whose inputs pass through host memory, on a stream that is still busy with the delay: equality with `want` only."""
    import torch
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        spin.enqueue(FLOOR_MS if ms is None else ms)
        got = read(call())
    s.synchronize()
    assert QH.same(got, want), f"{name}: the answer under a delayed stream differs from the one on the default stream"
    return got


# ------------------------------------------------------------------------------------------------------------------ the tables
LATE = {
    # probe -> how its late inputs reach it
    **{name: "files[0] of Inputs.on_device() is the late buffer" for name in ("latents", "latents_mapped", *QH.ONE_FILE)},
    **{name: "every file of Inputs.on_device() is a late buffer" for name in QH.BATCHES},
    **{name: "the image and vae.means are late buffers" for name in QH.WITH_VAE},
}
HOST = {
    **{name: "takes NumPy rows: the inputs pass through host memory" for name in ("batch_channel", "intervals", "codec")},
    **{name: "reads files given as bytes" for name in QH.READERS},
}
"""Probe -> why its inputs cannot arrive late on the device: run under the delayed stream, equality only."""

SEVERAL_RANKS, NO_DEVICE_WORK = "needs several ranks", "no device work"
EXEMPT_REASONS = {"vbq_comm.hip": SEVERAL_RANKS, "vbq_api.hip": NO_DEVICE_WORK, "vbq_host.hip": NO_DEVICE_WORK}
"""The closed set: which file may carry which reason."""

BY_SOURCE = {
    # file -> {case of tests/test_gpu_stream_order.py: the vbq_* entry points of that file it goes through} | a reason
    "vbq_api.hip": NO_DEVICE_WORK,
    "vbq_host.hip": NO_DEVICE_WORK,
    "vbq_comm.hip": SEVERAL_RANKS,
    "vbq_quantize.hip": {"quantize_f64_rows": ["vbq_quantize_rows_f32"], "quantize_f64_planes": ["vbq_quantize_f32"],
                         "level_counts": ["vbq_level_counts_f32"], "rows_to_budget": ["vbq_n_bit_intervals_f32"]},
    "vbq_quantize_fast.hip": {"quantize_planes": ["vbq_quantize_f32 > launch_quant_fast"],
                              "quantize_channel_last_indices": ["vbq_quantize_f32 > launch_quant_pruned"],
                              "quantize_f32_level_len_rows": ["vbq_quantize_rows_f32 > launch_quant_fast"],
                              "level_counts": ["vbq_level_counts_f32 > launch_level_counts_hull10"]},
    "vbq_hist.hip": {"histogram": ["vbq_histogram_u16", "vbq_histogram_u16_i32"], "histogram_models": ["vbq_histogram_models_u16"],
                     "code_lengths_from_counts": ["vbq_code_lengths_from_counts"]},
    "vbq_transpose.hip": {"transpose": ["vbq_transpose_f32"], "transpose_planes": ["vbq_transpose_planes"],
                          "prep_planes": ["vbq_prep_planes_f32"]},
    "vbq_latents.hip": {"gather_latents": ["vbq_gather_latents_u16", "vbq_gather_f32"], "probe:latents": ["vbq_compress_latents_f32"],
                        "build_entropy_models": ["vbq_build_entropy_models_f32"]},
    "vbq_reduce.hip": {"moments": ["vbq_moments_f32"], "rd_sums": ["vbq_rd_sums_u16"],
                       "numpy_sums": ["vbq_numpy_sum_sq_f32", "vbq_numpy_row_sums_f32"]},
    "vbq_notebook.hip": {"notebook_one_beta": ["vbq_quantize_notebook_f64"], "notebook_sweep": ["vbq_quantize_notebook_f64"]},
    "vbq_candidates.hip": {"candidates": ["vbq_argmax_candidates_f32"]},
    "vbq_budget.hip": {"rows_to_budget": ["vbq_budget_dp_f64"],
                       "budget_patience": ["vbq_budget_patience_f64"]},
    "vbq_records.hip": {"records_pack_rows": ["vbq_records_pack_u16", "vbq_records_unpack_f32"]},
    "vbq_topk.hip": {"records_most_similar": ["vbq_records_topk_f32"], "dense_most_similar": ["vbq_topk_f32"]},
    "vbq_bag.hip": {"records_bag": ["vbq_records_bag_f32"], "dense_bag": ["vbq_bag_f32"]},
    "vbq_ranks.hip": {"prediction_ranks": ["vbq_analogy_ranks_f32"]},
    "vbq_metrics.hip": {"mse": ["vbq_image_sqerr_u8"], "numpy_sums": ["vbq_unit_to_u8_f32"], "ms_ssim": ["vbq_ssim_scale_f64", "vbq_downsample2_f64"]},
    "vbq_bmshj.hip": {"bmshj_cdf_pdf": ["vbq_bmshj_cdf_pdf_f32"], "bmshj_loss_and_grads": ["vbq_bmshj_nll_grad_f32"]},
    "vbq_baselines.hip": {"uniform_quantizer": ["vbq_uniform_quantize_f32"], "nearest_code_quantizer": ["vbq_nearest_code_f64"]},
    "vbq_xi.hip": {"xi_encoder_on_a_delayed_stream": ["vbq_xi_intervals_f64", "vbq_xi_select_f64"]},
    "vbq_rans.hip": {"rans_encode": ["vbq_rans_encode_u16", "vbq_rans_sizes_u16"],
                     "rans_codec": ["vbq_rans_encode_u16", "vbq_rans_decode_u16", "vbq_rans_pack_u16", "vbq_rans_unpack_u16"],
                     "probe:to_bytes": ["vbq_rans_pack_u16"]},
    "vbq_rans_il.hip": {"interleaved_codec": ["vbq_rans_il_sizes_u16", "vbq_rans_il_encode_u16", "vbq_rans_il_decode_u16"]},
    "vbq_rans_map.hip": {"mapped_codec": ["vbq_rans_map_encode_u16", "vbq_rans_map_sizes_u16", "vbq_rans_map_decode_u16"]},
    "vbq_rans_files.hip": {"probe:b_to_bytes": ["vbq_rans_encode_files_u16"]},
    "vbq_rans_sizes_files.hip": {"probe:b_coded_nbytes": ["vbq_rans_sizes_files_u16"]},
    "vbq_rans_il_files.hip": {"probe:b_compact": ["vbq_rans_il_sizes_files_u16", "vbq_rans_il_encode_files_u16"],
                              "probe:b_coded_nbytes_compact": ["vbq_rans_il_rates_files_u16"],
                              "probe:r_compact_batch": ["vbq_rans_il_decode_files_u16"]},
    "vbq_rans_map_files.hip": {"probe:b_mapped": ["vbq_rans_map_encode_files_u16"],
                               "probe:b_coded_nbytes_mapped": ["vbq_rans_map_sizes_files_u16"]},
    "vbq_rans_map_rates_files.hip": {"probe:b_nbytes_palettes": ["vbq_rans_map_rates_files_u16"]},
    "vbq_rans_window.hip": {"probe:r_batch": ["vbq_rans_decode_window_f32"]},
    "vbq_rans_map_window.hip": {"probe:r_mapped_batch": ["vbq_rans_map_decode_window_f32"]},
}
"""`probe:<name>` is the case of that probe of quantizer_histories.PROBES (section a of the GPU module); every other name is a
key of its CASES (section b) or the name of a test of section c."""
