"""Every call is ordered on the caller's stream: what runs in the late-input harness of tests/stream_order.py (which says how
the harness works, why the inputs arrive late, and what it cannot see in a blocking call).

a. every probe of quantizer_histories.PROBES on a quantizer in state A: the probes of stream_order.LATE with the latents of
   their files (the image and the VAE's means for the image probes) arriving late, the probes of stream_order.HOST on the
   delayed stream with equality only; compress_latents also in its device-returning form, as an asynchronous (armed) case;
b. the calls outside the quantizer (CASES), at the small shapes their own test modules use, each asynchronous where it
   returns device tensors without reading them; stream_order.BY_SOURCE names them per source file;
c. state that crosses streams: lazy results read under another stream than the one that produced them (the wait_stream
   branch of HostStager.start), one quantizer used under three streams in turn, compress_replay captured and replayed under
   a side stream and replayed under the default one, EntropyModelBuild with its own side stream and its host stages;
d. the control: with ops._stream redirected to a third stream, the three one-launch calls answer with the STALE result.

The image of compress_replay passes through host memory (np.asarray in the method, a page-locked staging array in the
replay): it cannot arrive late on the device, the VAE's means -- which the captured graph reads -- do.  The xi-space encoder
takes and returns NumPy arrays only: it runs on the delayed stream with equality, as the probes of HOST do.

MEASURED on an MI355X (two runs of this module, 102 tests): t_ref of the 38 asynchronous cases 0.05 .. 0.80 ms (the largest:
compress with a device image), of the 39 blocking cases 0.12 .. 1.40 ms (the largest: the lambda-map batch budget), so every
delay is the FLOOR of 20 ms, 25 x the largest asynchronous t_ref (the rule asks for 4 x: 3.2 ms); no case comes near the cap.
torch.cuda._sleep is a stable clock there: 100 000 cycles 0.045 ms, 1 000 000 cycles 0.420 ms, 2.40e6 cycles per ms, and a
spin asked for 20 ms took 20.01 ms (the copy-chain fall-back was not needed).  The module takes 5.3 .. 6.4 s after 8 s of set-up (the
library load and the first quantizer); the fixture below prints these figures again on every run.

What the module found when it was written: HostStager.start waited on torch.cuda.ExternalStream(0) for results produced on
the default stream, which orders nothing -- a copy behind that wait read Z_hat before the default stream had written it
(test_lazy_results_read_under_another_stream[compress-default->side]).  vbq_amd/lazy.py now names the default stream itself."""
import contextlib
import ctypes
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import launch_plans as LP  # noqa: E402
import quantizer_histories as QH  # noqa: E402
import stream_order as SO  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
STALE = SO.STALE_SEED


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")
    t0 = time.perf_counter()
    yield
    rows = sorted(SO.T_REF.items(), key=lambda kv: kv[1][0])
    asyn = [v[0] for _, v in rows if not v[1]]
    block = [v[0] for _, v in rows if v[1]]
    print(f"\n[test_gpu_stream_order] {time.perf_counter() - t0:.1f} s; FLOOR {SO.FLOOR_MS} ms, cap {SO.CAP_MS} ms")
    if asyn:
        print(f"[test_gpu_stream_order] t_ref of {len(asyn)} asynchronous cases: {min(asyn):.3f} .. {max(asyn):.3f} ms "
              f"(largest: {[k for k, v in rows if not v[1]][-1]})")
    if block:
        print(f"[test_gpu_stream_order] t_ref of {len(block)} blocking cases: {min(block):.3f} .. {max(block):.3f} ms "
              f"(largest: {[k for k, v in rows if v[1]][-1]})")


@pytest.fixture(scope="module")
def spin():
    """The delay, calibrated once for the module."""
    sp, notes = SO.calibrate()
    print(f"\n[test_gpu_stream_order] {sp}: {notes}")
    return sp


@pytest.fixture(autouse=True)
def _stop_on_a_device_error():
    """A device error is not a wrong answer: after one, nothing more of this module is launched."""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"device error, the rest of the module is not run: {e}", returncode=3)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ====================================================================================================== a. the probes
_CACHE = {}


def inputs_A():
    """The inputs of state A (budgets from a fresh quantizer of the state), NumPy and device form."""
    if "inp" not in _CACHE:
        inp = QH.make_inputs(QH.fresh(QH.STATES["A"]), QH.STATES["A"].lambs, QH.FILE_SHAPES, "A/main")
        _CACHE["inp"] = (inp, inp.on_device())
    return _CACHE["inp"]


def oracle(name, probe, inp):
    """What a quantizer built once, in state A, and asked only this answers on the default stream."""
    key = (name, inp.tag)
    if key not in _CACHE:
        _CACHE[key] = SO.bits(QH.outcome(probe, QH.fresh(QH.STATES["A"]), inp))
    return _CACHE[key]


def with_files(inp, files):
    """`inp` with other latents in its files; the budgets, class maps and palettes stay those of the fresh inputs."""
    new = inp._copy()
    new.files = [tuple(pair) for pair in files]
    return new


def stale_files(seed=STALE):
    return SO.to_device([list(p) for p in QH.latents(QH.FILE_SHAPES, seed=seed)])


FILE_PROBES = {**{k: QH.PROBES[k] for k in ("latents", "latents_mapped")}, **QH.ONE_FILE, **QH.BATCHES}


@pytest.mark.parametrize("name", list(FILE_PROBES))
def test_probe_with_late_latents(name, spin):
    """The files of Inputs.on_device() are the late buffers; the reference is fresh(A) on the default stream.  These probes
    return bytes, integers and NumPy arrays: blocking, no arming assertion."""
    assert name in SO.LATE
    probe = FILE_PROBES[name]
    _, dinp = inputs_A()
    q, qr = QH.fresh(QH.STATES["A"]), QH.fresh(QH.STATES["A"])
    fresh = [list(p) for p in dinp.files]
    late = SO.run_late(lambda files: QH.outcome(probe, q, with_files(dinp, files)), fresh, stale_files(), blocking=True, spin=spin,
                       name=f"probe:{name}", reference_call=lambda files: QH.outcome(probe, qr, with_files(dinp, files)), read=SO.bits)
    assert late.want_fresh[0] == "ok", late.want_fresh[:3]
    assert QH.same(late.want_fresh, oracle(name + "[device]", probe, dinp))


def _latents_device(q, i):
    """compress_latents in its device-returning form: nothing is read."""
    m, lv = i.files[0]
    out = q.compress_latents(m[None], lv[None], i.lambs, return_np=False)
    return tuple(out[k][l] for k in ("Z_hat", "raw_num_bits", "num_bits_cl", "num_bits") for l in out[k])


def _latents_lazy(q, i):
    """compress_latents as it returns by default: lazy views, nothing is read until somebody looks."""
    m, lv = i.files[0]
    out = q.compress_latents(m[None], lv[None], i.lambs)
    return tuple(out[k][l] for k in ("Z_hat", "raw_num_bits", "num_bits_cl", "num_bits") for l in out[k])


def _latents_mapped_device(q, i):
    m, lv = i.files[0]
    out = q.compress_latents_mapped(m, lv, i.palette3, i.cls3[0], return_np=False)
    return out["Z_hat"], out["num_bits"]


@pytest.mark.parametrize("name,probe,blocking", [
    ("latents[return_np=False]", _latents_device, False), ("latents[lazy]", _latents_lazy, False),
    # (the class map is a NumPy array: its upload after the solve's launches waits for the stream)
    ("latents_mapped[return_np=False]", _latents_mapped_device, True)])
def test_device_returning_forms_are_asynchronous(name, probe, blocking, spin):
    _, dinp = inputs_A()
    q, qr = QH.fresh(QH.STATES["A"]), QH.fresh(QH.STATES["A"])
    fresh = [list(p) for p in dinp.files]
    late = SO.run_late(lambda files: probe(q, with_files(dinp, files)), fresh, stale_files(), blocking=blocking, spin=spin,
                       name=f"probe:{name}", reference_call=lambda files: probe(qr, with_files(dinp, files)))
    base = "latents" if name.startswith("latents[") else "latents_mapped"
    assert QH.same(late.want_fresh, oracle(base + "[device]", QH.PROBES[base], dinp)[1])


@pytest.mark.parametrize("name", list(SO.HOST))
def test_probe_through_host_memory_on_a_delayed_stream(name, spin):
    """NumPy rows and files given as bytes cannot arrive late on the device: the probe runs while the stream is still busy
    with the delay and must answer as fresh(A) does on the default stream."""
    probe = QH.PROBES[name]
    inp, _ = inputs_A()
    want = oracle(name, probe, inp)
    assert want[0] == "ok"
    q = QH.fresh(QH.STATES["A"])
    SO.run_delayed(lambda: QH.outcome(probe, q, inp), want, spin=spin, name=f"probe:{name}", read=SO.bits)


class LateVAE(QH.StubVAE):
    """The stub VAE with its means in a buffer the test fills late."""

    def __init__(self, shape, means):
        super().__init__(shape)
        self.means = means


def late_vae(cache, who, shape, means):
    """One LateVAE per (caller, means buffer): making one uploads its log-variances, which a late call must not do."""
    key = (who, means.data_ptr())
    if key not in cache:
        cache[key] = LateVAE(shape, means)
    return cache[key]


def vae_means(shape, seed):
    rng = np.random.default_rng(seed + int(np.prod(shape)))
    return dev((rng.normal(0, 1.2, tuple(shape[:-1]) + (QH.C,)) * QH.SCALES).astype(F32))


def image_dev(shape, seed):
    return dev(QH.image(shape, seed))


def _v_compress(q, i, X, vae):
    out = q.compress(X, vae, i.lambs)
    return tuple(out[k][l] for k in ("Z_hat", "raw_num_bits", "num_bits_cl", "num_bits", "X_hat") for l in out[k])


def _v_bytes(q, i, X, vae):
    data = q.compress_to_bytes(X, vae, i.lamb, segment=QH.SEGMENT)
    return data, q.decompress(data, vae)


def _replay_answer(q, vae, X, lambs):
    out, (sums, sums_cl, u8) = q.compress_replay(X, vae, lambs)
    return (tuple(np.array(out[k][l]) for k in ("Z_hat", "raw_num_bits", "num_bits_cl", "num_bits", "X_hat") for l in out[k]),
            sums, sums_cl, u8)


@pytest.mark.parametrize("name,run,blocking", [("v_compress", _v_compress, False), ("v_bytes", _v_bytes, True)])
def test_image_probe_with_a_late_image_and_late_means(name, run, blocking, spin):
    """compress returns lazy views without reading them (asynchronous, armed); compress_to_bytes + decompress return bytes and
    an array.  The image is a device tensor (StubVAE.encode takes one); it and the VAE's means arrive late."""
    assert name in SO.LATE
    shape = QH.IMAGE_SHAPES[0]
    inp, _ = inputs_A()
    q, qr = QH.fresh(QH.STATES["A"]), QH.fresh(QH.STATES["A"])
    fresh, stale = [image_dev(shape, 3), vae_means(shape, 5)], [image_dev(shape, STALE), vae_means(shape, STALE)]
    vaes = {}

    def call(who):
        def go(b):
            return run(q if who == "late" else qr, inp, b[0], late_vae(vaes, who, shape, b[1]))
        return go
    SO.run_late(call("late"), fresh, stale, blocking=blocking, spin=spin, name=f"probe:{name}", reference_call=call("ref"))


def test_image_probe_replay_with_late_means(spin):
    """v_replay: the capture, then a replay of it with another image.  Both images pass through host memory; what the captured
    graph reads on the device besides them, the VAE's means, arrives late before the capture and again, with other values,
    before the replay."""
    assert "v_replay" in SO.LATE
    shape = QH.IMAGE_SHAPES[0]
    inp, _ = inputs_A()
    X = QH.image(shape)
    images = [X, (0.5 * X).astype(F32)]
    means = [vae_means(shape, 5), vae_means(shape, 6)]
    stale = vae_means(shape, STALE)
    qr, ref_vae = QH.fresh(QH.STATES["A"]), LateVAE(shape, stale.clone())
    want, want_stale = [], []
    for x, m in zip(images, means):
        ref_vae.means.copy_(stale)
        want_stale.append(SO.plain(_replay_answer(qr, ref_vae, x, inp.lambs)))
        ref_vae.means.copy_(m)
        want.append(SO.plain(_replay_answer(qr, ref_vae, x, inp.lambs)))
    assert not any(QH.same(a, b) for a, b in zip(want, want_stale)) and not QH.same(want[0], want[1])
    q, vae = QH.fresh(QH.STATES["A"]), LateVAE(shape, stale.clone())
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for step, (x, m) in enumerate(zip(images, means)):
            spin.enqueue(SO.FLOOR_MS)
            vae.means.copy_(m, non_blocking=True)
            got = SO.plain(_replay_answer(q, vae, x, inp.lambs))
            assert QH.same(got, want[step]), f"step {step}: " + ("the stale answer" if QH.same(got, want_stale[step]) else "neither answer")
    s.synchronize()
    replays = list(q._dev_cache["_replays"].values())
    assert [r.mode for r in replays] == ["full"] and replays[0].replays == 2


# ====================================================================================================== b. outside the quantizer
CASES = {}


def case(name, blocking):
    """Register `fn() -> (call, make)`: call(inputs) -> results, make(seed) -> the input set on the device."""
    def deco(fn):
        assert name not in CASES
        CASES[name] = (fn, blocking)
        return fn
    return deco


N10, N4 = 10, 4
T10, T4 = 2 ** (N10 + 1) - 1, 2 ** (N4 + 1) - 1
CH = 3
ROWS = 515                                     # one element past two 256-thread workgroups of a plane, odd plane strides
SCALE = np.array([0.5, 1.0, 2.0])
LAM32 = [float(v) for v in 2.0 ** np.linspace(-8, 7.5, 32)]
FAST3 = [LAM32[3], LAM32[11], LAM32[20]]


def tables(N):
    """(level-major, sorted) f32 [CH, T] Gaussian code books on the device."""
    from vbq_amd import gaussian_table
    from vbq_amd import tables as TB
    tab = gaussian_table(SCALE, N)
    return dev(tab), dev(TB.level_major_to_sorted(tab))


def pair(seed, rows=ROWS, planes=False):
    """[mu, sigma] f32 [rows, CH] (or planes [CH, rows]) on the device."""
    rng = np.random.default_rng(seed)
    mu = (SCALE * rng.normal(0, 1, (rows, CH))).astype(F32)
    sg = np.clip(np.exp(rng.normal(-2, 0.7, (rows, CH))), 1e-4, 10).astype(F32)
    return [dev(mu.T), dev(sg.T)] if planes else [dev(mu), dev(sg)]


def indices(seed, shape, T):
    return dev(np.random.default_rng(seed).integers(0, T, shape).astype(np.uint16))


def level_len(seed, L, N):
    rng = np.random.default_rng(seed + 17)
    return dev((np.arange(N + 1, dtype=F32)[None, None] + rng.uniform(0, 3, (L, CH, N + 1))).astype(F32))


@case("quantize_planes", blocking=False)
def _():
    import vbq_amd
    tab, _ = tables(N10)
    assert LP.solve_kernel(N10, FAST3, "cb", CH, want_idx=True, elements=ROWS * CH) == "K1<0>"
    return (lambda b: vbq_amd.quantize(b[0], b[1], FAST3, table=tab, N=N10, out_layout="planes", return_values=True, validate=False),
            pair)


@case("quantize_channel_last", blocking=False)
def _():
    import vbq_amd
    tab, _ = tables(N10)
    ll = level_len(0, 3, N10)
    return (lambda b: vbq_amd.quantize(b[0], b[1], FAST3, table=tab, N=N10, lengths=ll, return_values=True, return_bits=True,
                                       validate=False), pair)


@case("quantize_channel_last_indices", blocking=False)
def _():
    import vbq_amd
    tab, _ = tables(N10)
    return lambda b: vbq_amd.quantize(b[0], b[1], LAM32[5], table=tab, N=N10, validate=False), pair


def _given_outputs(L, shape):
    from vbq_amd import _lib
    return dict(out_idx=torch.zeros((L,) + shape, dtype=torch.uint16, device="cuda"),
                out_zhat=torch.zeros((L,) + shape, dtype=torch.float32, device="cuda"),
                out_bits=torch.zeros((L,) + shape, dtype=torch.float32, device="cuda"),
                workspace=torch.empty(max(256, _lib.lib().vbq_quantize_workspace_bytes(CH, L, N10)), dtype=torch.uint8, device="cuda"))


@case("quantize_f32_level_len_rows", blocking=False)
def _():
    from vbq_amd import ops
    tab, _ = tables(N10)
    given = _given_outputs(3, (CH, ROWS))
    assert LP.solve_kernel(N10, FAST3, "cb", CH, level_len=True, want_zhat=True, want_bits=True, elements=ROWS * CH) == "K1<1>"
    # the length table is a late input too
    return (lambda b: ops.quantize(b[0], b[1], tab, FAST3, N=N10, level_len=b[2], layout="cb", rows=(3, 513), **given),
            lambda seed: pair(seed, planes=True) + [level_len(seed, 3, N10)])


@case("quantize_f64_rows", blocking=False)
def _():
    from vbq_amd import ops
    tab, _ = tables(N10)
    lam = [0.0, 0.5, 2.0]
    given = _given_outputs(3, (ROWS, CH))
    assert LP.solve_kernel(N10, lam, "bc", CH, mode="f64", want_zhat=True, want_bits=True, elements=ROWS * CH) == "tiled"
    return lambda b: ops.quantize(b[0], b[1], tab, lam, N=N10, layout="bc", mode="f64", rows=(1, ROWS - 1), **given), pair


@case("quantize_f64_planes", blocking=False)
def _():
    from vbq_amd import ops
    tab, _ = tables(N10)
    lam = [0.0, 0.5, 2.0]
    assert LP.solve_kernel(N10, lam, "cb", CH, mode="f64", want_zhat=True, elements=ROWS * CH) == "flat"
    return (lambda b: ops.quantize(b[0], b[1], tab, lam, N=N10, layout="cb", mode="f64", want_zhat=True),
            lambda seed: pair(seed, planes=True))


@case("level_counts", blocking=False)
def _():
    from vbq_amd import ops
    tab, _ = tables(N10)
    assert LP.solve_kernel(N10, FAST3, "cb", CH, counting=True, elements=ROWS * CH) == "K1t"
    assert LP.solve_kernel(N10, FAST3, "cb", CH, counting=True, level_len=True, elements=ROWS * CH) == "K1<2>"
    ll = level_len(1, 3, N10)
    return (lambda b: (ops.level_counts(b[0], b[1], tab, FAST3, N=N10, layout="cb"),
                       ops.level_counts(b[0], b[1], tab, FAST3, N=N10, layout="cb", level_len=ll)),
            lambda seed: pair(seed, planes=True))


@case("histogram", blocking=False)
def _():
    from vbq_amd import ops
    return (lambda b: (ops.histogram(b[0], CH, N=N4, layout="bc"), ops.histogram(b[0].reshape(2, -1), 1, N=N4, dtype=torch.int32)),
            lambda seed: [indices(seed, (2, ROWS, CH), T4)])


@case("histogram_models", blocking=False)
def _():
    from vbq_amd import ops
    lut = dev((-np.log2((np.arange(ROWS + 1) + 1.0) / (ROWS + T4))).astype(F32))
    counts = torch.empty((2, CH, T4), dtype=torch.int32, device="cuda")
    models = torch.empty((2, CH, T4), dtype=torch.float32, device="cuda")
    return lambda b: ops.histogram_models(b[0], CH, counts, N=N4, lut=lut, models=models), lambda seed: [indices(seed, (2, CH, ROWS), T4)]


@case("code_lengths_from_counts", blocking=False)
def _():
    from vbq_amd import ops
    lut = dev((-np.log2((np.arange(ROWS + 1) + 1.0) / (ROWS + N4 + 1))).astype(F32))
    return (lambda b: ops.code_lengths_from_counts(b[0], lut, level_period=N4 + 1, want_model=True),
            lambda seed: [dev(np.random.default_rng(seed).integers(0, ROWS + 1, (2, CH, N4 + 1)))])


@case("transpose", blocking=False)
def _():
    from vbq_amd import ops
    return lambda b: ops.transpose(b[0]), lambda seed: pair(seed)[:1]


@case("transpose_planes", blocking=False)
def _():
    from vbq_amd import ops
    return (lambda b: (ops.transpose_planes(b[0]), ops.transpose_planes(b[1])),
            lambda seed: [indices(seed, (2, CH, ROWS), T4), dev(np.random.default_rng(seed).normal(0, 1, (2, ROWS, CH)).astype(F32))])


@case("prep_planes", blocking=False)
def _():
    from vbq_amd import ops
    return lambda b: ops.prep_planes(b[0], b[1], spread="variance"), pair


@case("gather_latents", blocking=False)
def _():
    from vbq_amd import ops
    _, srt = tables(N4)
    ll = level_len(2, 2, N4)
    models = dev(np.random.default_rng(3).uniform(1, 12, (2, CH, T4)).astype(F32))
    return (lambda b: tuple(ops.gather_latents(b[0], N=N4, table_sorted=srt, level_len=ll, models=models, want_num_bits=True, want_idx=True))
            + (ops.gather(b[0], srt, CH, N=N4, layout="cb", out_layout="bc"),),
            lambda seed: [indices(seed, (2, CH, ROWS), T4)])


def quarters(seed, shape, lo=-8, hi=8):
    """Multiples of 1/4: the two reductions below add f64 terms with atomics, in whatever order the workgroups arrive, and are
    compared bit for bit here -- so every term and every partial sum has to be exact.  Multiples of 1/4 (of 1/8 for the code
    points) below 8 in magnitude and standard deviations that are powers of two make them so."""
    return dev((np.random.default_rng(seed).integers(4 * lo, 4 * hi + 1, shape) / 4.0).astype(F32))


@case("moments", blocking=False)
def _():
    from vbq_amd import ops
    return (lambda b: (ops.moments(b[0]), ops.moments(b[1], layout="cb")),
            lambda seed: [quarters(seed, (ROWS, CH)), quarters(seed + 1, (CH, ROWS))])


@case("rd_sums", blocking=False)
def _():
    from vbq_amd import ops
    srt = dev(((np.arange(T4)[None, :] - 15 + np.arange(CH)[:, None]) / 8.0).astype(F32))          # sorted, exact (see quarters)
    rate = quarters(4, (2, CH, T4), 0, 12)

    def make(seed):
        sigma = dev(np.random.default_rng(seed).choice(np.array([0.5, 1.0, 2.0], F32), (ROWS, CH)))
        return [quarters(seed, (ROWS, CH), -2, 2), sigma, indices(seed, (2, ROWS, CH), T4)]
    return lambda b: ops.rd_sums(b[0], b[1], b[2], srt, CH, N=N4, layout="bc", rate=rate), make


@case("numpy_sums", blocking=False)
def _():
    from vbq_amd import ops
    return (lambda b: (ops.numpy_sum_sq(b[0]), ops.numpy_row_sums(b[0]), ops.unit_to_u8(b[0])),
            lambda seed: [dev(np.random.default_rng(seed).uniform(0, 1, (5, 1031)).astype(F32))])


def _notebook(betas):
    from scipy.stats import norm
    from vbq_amd import ops
    from vbq_amd import tables as TB
    book = dev(norm.ppf(TB.dyadic_xi(N4)))

    def make(seed):
        rng = np.random.default_rng(seed)
        return [dev(rng.normal(0, 1, (ROWS, 5)).astype(F32)), dev(rng.uniform(0.05, 1.0, (ROWS, 5)).astype(F32))]
    return lambda b: ops.quantize_notebook(b[0], b[1], book, betas, N=N4), make


@case("notebook_one_beta", blocking=False)
def _():
    return _notebook([0.7])


@case("notebook_sweep", blocking=False)
def _():
    return _notebook([0.01, 0.3, 2.0, 40.0])


@case("candidates", blocking=False)
def _():
    from vbq_amd import ops

    def make(seed):
        rng = np.random.default_rng(seed)
        P = np.sort(rng.normal(0, 1.5, (6, ROWS, CH)), axis=0).astype(F32)
        lens = rng.uniform(0, 9, (2, 6, ROWS, CH)).astype(F32)
        return [dev(P), dev(lens)] + pair(seed)
    return (lambda b: (ops.argmax_candidates(b[0], b[1], b[2], b[3], [0.05, 3.0], want_j=True),
                       ops.argmax_candidates(b[0], b[1][0], b[2], b[3], [0.05, 3.0], mode="f64")), make)


K_ROW, R_ROWS, BITS = 5, 9, 11


def _book4():
    from scipy.stats import norm
    from vbq_amd import tables as TB
    book = norm.ppf(TB.dyadic_xi(N4)).astype(F32)
    book.setflags(write=False)
    return book


def _rows(seed, rows=R_ROWS):
    rng = np.random.default_rng(seed)
    return [dev(rng.normal(0, 1, (rows, K_ROW)).astype(F32)), dev(rng.uniform(0.05, 1.0, (rows, K_ROW)).astype(F32))]


@case("rows_to_budget", blocking=True)
def _():
    """Reads one status word after its last launch: every launch is enqueued while the delay runs."""
    import vbq_amd
    book = _book4()
    budgets = np.array([BITS, 0, 3, K_ROW * N4, 7, BITS, 1, 12, 5])
    return (lambda b: (vbq_amd.quantize_rows_to_budget(b[0], b[1], BITS, table=book, N=N4),
                       vbq_amd.quantize_rows_to_budget(b[0], b[1], budgets, table=book, N=N4)), _rows)


@case("budget_patience", blocking=False)
def _():
    from vbq_amd import ops
    return (lambda b: ops.budget_patience(b[0], 0.3, 3),
            lambda seed: [dev(np.sort(np.random.default_rng(seed).normal(0, 2, (N4 + 1, 777)), axis=0))])


def _record_indices(seed, rows):
    import vbq_amd
    idx, _, _ = vbq_amd.quantize_rows_to_budget(*_rows(seed, rows), BITS, table=_book4(), N=N4)
    return idx


@case("records_pack_rows", blocking=False)
def _():
    """ops.records_pack, then the rows of the records just packed: the second launch reads what the first wrote."""
    from vbq_amd import ops
    from vbq_amd import tables as TB
    srt = dev(TB.level_major_to_sorted(_book4()[None]))
    ids = dev(np.array([3, 0, 300, 3, 299]))

    def call(b):
        status = torch.zeros(2, dtype=torch.int32, device="cuda").view(torch.uint32)
        words = ops.records_pack(b[0], BITS, N4, status=status[:1])
        return (words, status) + tuple(ops.records_unpack(words, K_ROW, N4, BITS, srt, ids, want_idx=True, status=status[1:]))
    return call, lambda seed: [_record_indices(seed, 301)]


def _record_file(seed, rows=40):
    from vbq_amd import embeddings as E
    m, s = _rows(seed, rows)
    return E.compress_to_records(m, s, BITS, _book4(), N4)


@case("records_rows_most_similar_bag", blocking=True)
def _():
    """RecordEmbeddings.rows, .most_similar and .bag upload their ids and read a status word.  The file is bytes; what arrives
    late is the record words the object keeps on the device."""
    from vbq_amd import embeddings as E
    re = E.RecordEmbeddings(_record_file(1))
    q = np.random.default_rng(9).normal(0, 1, (2, K_ROW)).astype(F32)

    def call(b):
        re._words = b[0]
        return (re.rows([3, 1, 39, 3]), re.tensor()) + tuple(re.most_similar(q, k=3)) + tuple(re.most_similar(ids=[2, 0], k=3, metric="dot")) + \
            (re.bag([[0, 1, 5], [2, -1, 39]]), re.bag([4, 4, 7, 1], [0, 1], mode="mean"))
    return call, lambda seed: [E.RecordEmbeddings(_record_file(seed))._words.clone()]


def _emb(seed, V=301, K=7):
    return dev(np.random.default_rng(seed).normal(0, 1, (V, K)).astype(F32))


@case("records_most_similar", blocking=False)
def _():
    from vbq_amd import ops
    from vbq_amd import tables as TB
    srt = dev(TB.level_major_to_sorted(_book4()[None]))
    excl = dev(np.array([[1, -1], [7, 8]]))

    def call(b):
        status = torch.zeros(1, dtype=torch.int32, device="cuda").view(torch.uint32)
        words = ops.records_pack(b[0], BITS, N4)
        return ops.records_topk(words, K_ROW, N4, BITS, srt, b[1], 4, "cosine", excl, status=status) + (status,)
    return call, lambda seed: [_record_indices(seed, 301), dev(np.random.default_rng(seed).normal(0, 1, (2, K_ROW)).astype(F32))]


@case("records_bag", blocking=False)
def _():
    from vbq_amd import ops
    from vbq_amd import tables as TB
    srt = dev(TB.level_major_to_sorted(_book4()[None]))
    offsets = dev(np.array([0, 3, 3, 8]))

    def call(b):
        words = ops.records_pack(b[0], BITS, N4)
        return ops.records_bag(words, K_ROW, N4, BITS, srt, b[1], offsets, weights=b[2]), ops.records_bag(words, K_ROW, N4, BITS, srt, b[1], offsets, mode="max")

    def make(seed):
        rng = np.random.default_rng(seed)
        return [_record_indices(seed, 301), dev(rng.integers(-1, 301, 8)), dev(rng.uniform(0.5, 2, 8).astype(F32))]
    return call, make


@case("dense_most_similar", blocking=False)
def _():
    from vbq_amd import ops
    return (lambda b: ops.topk(b[0], b[1], 5, "cosine") + ops.topk(b[0], b[1], 2, "dot"),
            lambda seed: [_emb(seed), dev(np.random.default_rng(seed + 1).normal(0, 1, (3, 7)).astype(F32))])


@case("dense_most_similar_checked", blocking=True)
def _():
    """embeddings.most_similar looks at its queries (isfinite) before the launch."""
    from vbq_amd import embeddings as E
    return (lambda b: E.most_similar(b[0], b[1], k=5),
            lambda seed: [_emb(seed), dev(np.random.default_rng(seed + 1).normal(0, 1, (3, 7)).astype(F32))])


@case("dense_bag", blocking=False)
def _():
    from vbq_amd import ops
    offsets = dev(np.array([0, 3, 3, 8]))
    return (lambda b: (ops.bag(b[0], b[1], offsets, mode="mean"), ops.bag(b[0], b[1], offsets, weights=b[2])),
            lambda seed: [_emb(seed), dev(np.random.default_rng(seed).integers(-1, 301, 8)),
                          dev(np.random.default_rng(seed).uniform(0.5, 2, 8).astype(F32))])


@case("dense_bag_checked", blocking=True)
def _():
    """embeddings.bag checks and uploads its ids on the host, and reads a status word."""
    from vbq_amd import embeddings as E
    return lambda b: E.bag(b[0], [[0, 1, 5], [2, -1, 300]], mode="sum"), lambda seed: [_emb(seed)]


@case("prediction_ranks", blocking=True)
def _():
    """Uploads the analogy ids before its launches; the ranks come back as a device tensor."""
    from vbq_amd import embeddings as E
    an = np.random.default_rng(5).integers(0, 301, (37, 4))
    return lambda b: E.prediction_ranks(b[0], an), lambda seed: [_emb(seed, 301, 50)]


def _images(seed, shape=(2, 24, 20, 3)):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, shape).astype(np.uint8)
    return [dev(a), dev(np.clip(a.astype(np.int64) + rng.integers(-9, 10, shape), 0, 255).astype(np.uint8))]


@case("mse", blocking=True)
def _():
    from vbq_amd import metrics
    return lambda b: (metrics.mse(b[0], b[1]), metrics.mse(b[0].to(torch.float32), b[1].to(torch.float32))), _images


@case("ms_ssim", blocking=True)
def _():
    from vbq_amd import metrics
    return lambda b: metrics.ms_ssim(b[0], b[1], weights=[0.3, 0.7]), _images


def _bmshj():
    from vbq_amd import priors
    p = priors.BMSHJ2018Prior(CH, init_scale=10.0, seed=0)
    rng = np.random.default_rng(1000)
    p.set_weights([w + rng.normal(0, 0.3, w.shape).astype(F32) for w in p.get_weights()])
    return p


@case("bmshj_cdf_pdf", blocking=False)
def _():
    p = _bmshj()
    return (lambda b: p.cdf_pdf(b[0]) + (p.logpdf(b[0]),),
            lambda seed: [dev(np.random.default_rng(seed).normal(0, 3, (ROWS, CH)).astype(F32))])


@case("bmshj_loss_and_grads", blocking=True)
def _():
    p = _bmshj()
    return lambda b: p.loss_and_grads(b[0]), lambda seed: [dev(np.random.default_rng(seed).normal(0, 3, (CH, ROWS)).astype(F32))]


@case("uniform_quantizer", blocking=False)
def _():
    """The launch of UniformQuantizer.fit / .quantize (which look at their samples on the host first)."""
    from vbq_amd import baselines
    u = baselines.UniformQuantizer(16)
    u.min, u.max, u.delta = F32(-3.0), F32(3.0), F32(6.0 / 16)
    return lambda b: u._run(b[0], True), lambda seed: [dev(np.random.default_rng(seed).normal(0, 1, 1031).astype(F32))]


@case("nearest_code_quantizer", blocking=True)
def _():
    """The launch of KmeansQuantizer.fit / .quantize; the code points are uploaded per call."""
    from vbq_amd import baselines
    km = baselines.KmeansQuantizer(16)
    km.code_points = np.random.default_rng(2).normal(0, 1, 16)
    return lambda b: km._vq(b[0], True), lambda seed: [dev(np.random.default_rng(seed).normal(0, 1, 1031).astype(F32))]


SEG, STREAMS, SYMS = 32, 3, 75


def _freq(seed, shape):
    from vbq_amd import coder
    return coder.quantize_frequencies(np.random.default_rng(seed).integers(0, 50, shape + (T4,)))


@case("rans_encode", blocking=False)
def _():
    from vbq_amd.coder import RansCodec
    codec = RansCodec(_freq(1, (STREAMS,)), N=N4, segment=SEG)
    return (lambda b: codec.encode(b[0]) + (codec.sizes(b[0]),),
            lambda seed: [indices(seed, (STREAMS, SYMS), T4)])


@case("rans_codec", blocking=True)
def _():
    """encode -> decode as one chained call: the decoder reads its status word."""
    from vbq_amd.coder import RansCodec
    codec = RansCodec(_freq(1, (STREAMS,)), N=N4, segment=SEG)

    def call(b):
        words, sizes = codec.encode(b[0])
        sz, payload = codec.encode_packed(b[0])
        return words, sizes, codec.decode(words, sizes, SYMS), sz, payload, codec.decode_packed(dev(payload), dev(sz.astype(np.uint16)), SYMS)
    return call, lambda seed: [indices(seed, (STREAMS, SYMS), T4)]


@case("interleaved_sizes", blocking=False)
def _():
    from vbq_amd.coder import RansCodec
    codec = RansCodec(_freq(1, (STREAMS,)), N=N4, segment=None)
    return lambda b: codec.sizes_interleaved(b[0], 64), lambda seed: [indices(seed, (STREAMS, SYMS), T4)]


@case("interleaved_codec", blocking=True)
def _():
    from vbq_amd.coder import RansCodec
    codec = RansCodec(_freq(1, (STREAMS,)), N=N4, segment=None)

    def call(b):
        sizes, payload = codec.encode_interleaved(b[0], 64)
        return sizes, payload, codec.decode_interleaved(dev(payload), dev(sizes), SYMS, 64)
    return call, lambda seed: [indices(seed, (STREAMS, SYMS), T4)]


@case("mapped_codec", blocking=True)
def _():
    """The class map is checked (and uploaded) before the encoder's launch."""
    from vbq_amd.coder import MappedRansCodec
    codec = MappedRansCodec(_freq(1, (2, STREAMS)), N=N4, segment=SEG)
    cls = np.random.default_rng(3).integers(0, 2, SYMS)

    def call(b):
        words, sizes = codec.encode(b[0], cls)
        return words, sizes, codec.sizes(b[0], cls), codec.decode(words, sizes, cls, SYMS)
    return call, lambda seed: [indices(seed, (2, STREAMS, SYMS), T4)]


@pytest.mark.parametrize("name", list(CASES))
def test_call_with_late_inputs(name, spin):
    fn, blocking = CASES[name]
    call, make = fn()
    SO.run_late(call, make(7), make(STALE), blocking=blocking, spin=spin, name=name)


def test_xi_encoder_on_a_delayed_stream(spin):
    """utils.encode_vectorized takes and returns NumPy arrays, and evaluates the caller's functions on the host between its
    two launches: nothing of it can arrive late on the device."""
    from vbq_amd import utils
    z = np.random.default_rng(7).normal(0, 1.5, 301)
    sq, unsq = (lambda v: 1.0 / (1.0 + np.exp(-v))), (lambda e: np.log(e / (1 - e)))
    call = lambda: tuple(utils.encode_vectorized(lambda zs: -0.5 * (zs - z) ** 2, z, 0.05, sq, unsq, max_bits_per_coord=9).items())
    want = SO.plain(call())
    SO.run_delayed(call, want, spin=spin, name="xi_encoder")


def test_by_source_names_cases_that_exist():
    tests = {k for k in globals() if k.startswith("test_")}
    for name, row in SO.BY_SOURCE.items():
        if isinstance(row, dict):
            for c in row:
                assert (c[6:] in QH.PROBES) if c.startswith("probe:") else (c in CASES or "test_" + c in tests), (name, c)


# ====================================================================================================== c. state across streams
def _stream(s):
    return contextlib.nullcontext() if s is None else torch.cuda.stream(s)


def _lazy_round(make_call, fresh, stale, produce, read_on, spin, q, want):
    """call(buffers) under `produce` (None: the default stream) with late inputs, the lazy results read under `read_on`."""
    buffers = SO._map(lambda t: t.clone(), stale)
    with _stream(produce):
        SO.plain(make_call(buffers))                                  # warm: tables, workspaces, staging blocks
    torch.cuda.synchronize()
    armed = torch.cuda.Event()
    with _stream(produce):
        spin.enqueue(SO.FLOOR_MS)
        armed.record()
        for b, f in zip(SO._leaves(buffers), SO._leaves(fresh)):
            b.copy_(f, non_blocking=True)
        out = make_call(buffers)
        assert not armed.query(), "not armed: producing the lazy results synchronized"
    before = q._stager().transfers
    with _stream(read_on):
        got = SO.plain(out)
    torch.cuda.synchronize()
    assert q._stager().transfers > before, "no transfer was issued: the results were not lazy"
    assert QH.same(got, want), "lazy results read under another stream than the one that produced them are not the fresh ones"


@pytest.mark.parametrize("order", ["side->default", "default->side", "side->second"])
@pytest.mark.parametrize("method", ["compress_latents", "compress"])
def test_lazy_results_read_under_another_stream(method, order, spin):
    """The `stack.stream != st` branch of HostStager.start: the reading stream waits for the producing one."""
    inp, dinp = inputs_A()
    q, qr = QH.fresh(QH.STATES["A"]), QH.fresh(QH.STATES["A"])
    shape = QH.IMAGE_SHAPES[0]
    if method == "compress_latents":
        fresh, stale = [list(dinp.files[0])], [stale_files()[0]]
        call = lambda who: lambda b: _latents_lazy(who, with_files(dinp, b))
    else:
        fresh, stale = [image_dev(shape, 3), vae_means(shape, 5)], [image_dev(shape, STALE), vae_means(shape, STALE)]
        vaes = {}
        call = lambda who: lambda b: _v_compress(who, inp, b[0], late_vae(vaes, id(who), shape, b[1]))
    want = SO.plain(call(qr)(fresh))
    s, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    produce, read_on = {"side->default": (s, None), "default->side": (None, s), "side->second": (s, s2)}[order]
    _lazy_round(call(q), fresh, stale, produce, read_on, spin, q, want)


def test_one_quantizer_moved_between_streams():
    """Built on the default stream, a round of every probe under s, the same round on the default stream, then under s2: the
    cached tables, workspaces, the staging block and the codec caches made under one stream serve the next."""
    inp, _ = inputs_A()
    q = QH.fresh(QH.STATES["A"])
    s, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    main = torch.cuda.current_stream()

    def round_(where):
        bad = []
        with _stream(where):
            for name, probe, i in QH.runs(inp):
                got, want = SO.bits(QH.outcome(probe, q, i)), oracle(name, probe, i)
                if not QH.same(got, want):
                    bad.append(name)
        return bad
    s.wait_stream(main)
    assert not round_(s), "under s"
    main.wait_stream(s)
    assert not round_(None), "back on the default stream"
    s2.wait_stream(main)
    assert not round_(s2), "under s2"
    main.wait_stream(s2)


def test_compress_replay_captured_and_replayed_across_streams(spin):
    """Captured while s is current, replayed under s and under the default stream, for two image shapes (two captures).  Before
    every call the VAE's means -- what the graph reads on the device besides the image it stages itself -- arrive late on the
    stream the call is made under."""
    inp, _ = inputs_A()
    shapes = QH.IMAGE_SHAPES[:2]
    q, qr = QH.fresh(QH.STATES["A"]), QH.fresh(QH.STATES["A"])
    s = torch.cuda.Stream()
    steps = [(s, 0), (s, 1), (None, 2)]                                          # the capture, a replay under s, one under the default stream
    want, stale_want = {}, {}
    vaes = {sh: (LateVAE(sh, vae_means(sh, STALE)), LateVAE(sh, vae_means(sh, STALE))) for sh in shapes}
    for sh in shapes:                                                            # the reference: default stream, its own quantizer and VAE
        for _, k in steps:
            x = (QH.image(sh) * (1.0 - 0.25 * k)).astype(F32)
            vaes[sh][1].means.copy_(vae_means(sh, STALE))
            stale_want[sh, k] = SO.plain(_replay_answer(qr, vaes[sh][1], x, inp.lambs))
            vaes[sh][1].means.copy_(vae_means(sh, 20 + k))
            want[sh, k] = SO.plain(_replay_answer(qr, vaes[sh][1], x, inp.lambs))
            assert not QH.same(want[sh, k], stale_want[sh, k])
    torch.cuda.synchronize()
    for where, k in steps:
        for sh in shapes:
            x = (QH.image(sh) * (1.0 - 0.25 * k)).astype(F32)
            fresh = vae_means(sh, 20 + k)
            torch.cuda.synchronize()
            with _stream(where):
                spin.enqueue(SO.FLOOR_MS)
                vaes[sh][0].means.copy_(fresh, non_blocking=True)
                got = SO.plain(_replay_answer(q, vaes[sh][0], x, inp.lambs))
            torch.cuda.synchronize()
            assert QH.same(got, want[sh, k]), f"step {k}, image {sh}: " + ("the stale answer" if QH.same(got, stale_want[sh, k]) else "neither answer")
    replays = list(q._dev_cache["_replays"].values())
    assert len(replays) == 2 and {r.mode for r in replays} == {"full"} and [r.replays for r in replays] == [3, 3]


BUILD_ROWS, BUILD_LAMBDAS = 4096, [0.5, 2.0]


@pytest.mark.parametrize("n_chunks,smoothing", [(2, 1), (None, 1), (2, 0.5), (None, 0.5)],
                         ids=["chunked", "one-stream", "chunked-host-stages", "one-stream-host-stages"])
def test_entropy_model_build_with_late_latents(n_chunks, smoothing, spin):
    """run() only enqueues: asynchronous and armed.  With n_chunks=2 K2 runs on the build's own side stream behind events
    recorded on the current stream; with a fractional smoothing both -log2 steps are host functions enqueued on the stream
    (hipLaunchHostFunc).  The harness's warm-up is a first run() on the same object: the late run is its second, so the side
    stream of run 1 meets the zero_() of run 2."""
    from vbq_amd.pipeline import EntropyModelBuild
    tab = tables(N4)[0]

    def build():
        b = EntropyModelBuild(BUILD_ROWS, CH, BUILD_LAMBDAS, tab, N=N4, n_chunks=n_chunks, add_n_smoothing=smoothing)
        assert (b.side is not None) == (n_chunks == 2) and b.has_host_stages == (smoothing != 1)
        return b
    late_build, ref_build = build(), build()

    def call(b):
        def go(x):
            b.run(x[0], x[1])
            return b.level_counts, b.counts, b.level_len, b.raw_models, b.models
        return go
    SO.run_late(call(late_build), pair(7, BUILD_ROWS, planes=True), pair(STALE, BUILD_ROWS, planes=True), blocking=False, spin=spin,
                name=f"build_entropy_models[{n_chunks},{smoothing}]", reference_call=call(ref_build))
    late_build.check()


def test_build_entropy_models(spin):
    """vbq_build_entropy_models_f32: the whole alternation in one C call on channel-last latents."""
    from vbq_amd.pipeline import EntropyModelBuild
    tab = tables(N4)[0]
    builds = [EntropyModelBuild(BUILD_ROWS, CH, BUILD_LAMBDAS, tab, N=N4) for _ in range(2)]

    def call(b):
        def go(x):
            b.run_one_call(x[0], x[1])
            return b.level_counts, b.counts, b.level_len, b.raw_models, b.models
        return go
    SO.run_late(call(builds[0]), pair(7, BUILD_ROWS), pair(STALE, BUILD_ROWS), blocking=False, spin=spin, name="build_entropy_models",
                reference_call=call(builds[1]))


# ====================================================================================================== d. the control
def _control_cases():
    from vbq_amd import ops
    tab, _ = tables(N10)
    out_t = torch.empty((CH, ROWS), dtype=torch.float32, device="cuda")
    given = _given_outputs(3, (CH, ROWS))
    counts = torch.zeros((2, CH, T4), dtype=torch.int64, device="cuda")
    return {
        "transpose": (lambda b: ops.transpose(b[0], out=out_t), lambda seed: pair(seed)[:1], None),
        "quantize": (lambda b: ops.quantize(b[0], b[1], tab, FAST3, N=N10, layout="cb", **given), lambda seed: pair(seed, planes=True), None),
        "histogram": (lambda b: ops.histogram(b[0], CH, N=N4, layout="bc", out=counts), lambda seed: [indices(seed, (2, ROWS, CH), T4)],
                      lambda: counts.zero_()),
    }


def runs_beside(s, t, spin):
    """True when work on t does not wait for work enqueued on s before it.  Streams share the runtime's few hardware queues, and
    two that were given the same one run in order by accident: t then only returns once the delay on s is over."""
    torch.cuda.synchronize()
    busy, word = torch.cuda.Event(), torch.zeros(1, device="cuda")
    with torch.cuda.stream(s):
        spin.enqueue(SO.FLOOR_MS)
        busy.record(s)
    with torch.cuda.stream(t):
        word.add_(1)
    t.synchronize()
    beside = not busy.query()
    torch.cuda.synchronize()
    return beside


def two_streams_that_run_side_by_side(spin, candidates=8):
    """The premise of the control, checked instead of assumed: s, and the first of a few streams that runs beside it (which
    hardware queue a stream has depends on every stream the process made before)."""
    s = torch.cuda.Stream()
    for _ in range(candidates):
        t = torch.cuda.Stream()
        if runs_beside(s, t, spin):
            return s, t
    pytest.fail(f"none of {candidates} streams runs beside another one: the control cannot be armed")


@pytest.mark.parametrize("name", ["transpose", "quantize", "histogram"])
def test_control_a_misrouted_launch_is_seen(name, spin, monkeypatch):
    """ops._stream redirected to a third stream t: the one launch of the call does not wait for the delay, reads the stale
    inputs, and the harness sees it -- the answer is not the fresh one, and once everything has run it is exactly the stale
    one.  Only calls that are one launch each, with their outputs (and workspace) given: nothing else is enqueued.  t is a
    stream that does run beside s (two_streams_that_run_side_by_side): on a hardware queue shared with s the misrouted launch
    would wait for the delay like a correct one, and the control would fail for a reason that is none of the library's."""
    from vbq_amd import ops
    call, make, reset = _control_cases()[name]
    s, t = two_streams_that_run_side_by_side(spin)
    handle = t.cuda_stream
    routed = {"on": False, "calls": 0}
    real = ops._stream

    def misrouted(tensor):
        if not routed["on"]:
            return real(tensor)
        routed["calls"] += 1
        return ctypes.c_void_p(handle)
    monkeypatch.setattr(ops, "_stream", misrouted)

    def late_call(b):
        routed["on"] = torch.cuda.current_stream() == s                        # the references and the warm-up stay in order
        try:
            return call(b)
        finally:
            routed["on"] = False
    late = SO.run_late(late_call, make(7), make(STALE), blocking=False, spin=spin, stream=s, compare=False, warm=False, reset=reset)
    assert routed["calls"] == 1, routed
    assert late.armed and not QH.same(late.got, late.want_fresh), "a launch on another stream went unnoticed"
    torch.cuda.synchronize()
    assert QH.same(SO.plain(late.out), late.want_stale), "the misrouted launch did not read the stale inputs"
