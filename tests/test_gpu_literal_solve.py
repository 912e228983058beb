"""The literal 21-candidate R-D solves of vbq_quantize.hip, in both score modes, at their edges.

Every case compares indices, Z_hat and bits bit for bit with the C oracle (oracle.c_oracle.quantize with the same
mode) and checks the winners' scores against oracle/rd_f64.py, which scores every code point of the channel: the score
of the chosen point must equal the exhaustive maximum.

Which kernel a case reaches (launch_quantize in vbq_quantize.hip):
  k_quant_tiled<N, double>   mode "f64", layout "bc", n_ch > 1.  N <= 10.
  k_quant_flat<N, double>    mode "f64", layout "cb" or n_ch == 1.
  k_quant_tiled<N, float>    mode "f32", layout "bc", n_ch > 1.
  k_quant_flat<N, float>     mode "f32", layout "cb" or n_ch == 1, some lambda outside [1.9e-12, 1.8e19] (fast_ok false),
                             and not the pruned descent: L >= 5, Z_hat / bits wanted, or workgroups_per_cu != 0.
                             The cases below put lambda = 0 (or 1e-13, 1e25, 1e30) in every f32 sweep on planes.
  With every lambda inside that range, or indices only with L <= 4 and workgroups_per_cu == 0, f32 planes take the
  fast / pruned kernels instead (the fast-range boundary and the 1-4 lambda cases); the results must be the same.
Lambdas are handled in chunks of 32 (kMaxLambdaChunk): 31, 32, 33 and 70 lambdas cross the chunk loop and its l0
offsets into the outputs.  The tiled kernel walks 128 rows per iteration (kRowsPerIter) and 16-channel tile groups; the
flat one 4 elements per thread, with 16-byte accesses only when rows, views and outputs are 16-byte aligned (vec_ok).
The mode-splitting element set (oracle/mode_split.py) also goes through K1c here; K1c's own edges are in
test_gpu_candidates.py.
"""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import c_oracle as CO
from oracle import rd_f64 as R
from oracle import vbq_oracle as O
from oracle.mode_split import SPLIT_LAMS, mode_splitting_set
from solve_cases import latents            # the edge data: hits, nextafter neighbours, mid-points, both rims, extreme sigmas

pytestmark = pytest.mark.gpu
F32 = np.float32
MODE = {"f32": 0, "f64": 1}
# lambdas f32 cannot represent, and lambda = 0: on planes the f32 sweeps below leave the fast kernels' range
LAM6 = [0.0, 2.0 ** -8 * np.sqrt(2.0), 0.1, 1.0, 37.0, 300.0]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")
    from vbq_amd import ops as _ops
    t0 = time.perf_counter()
    yield _ops
    print(f"\n[test_gpu_literal_solve] {time.perf_counter() - t0:.1f} s")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def tables(rng, C, Nb):
    orc = O.ChannelwiseOracle(C, Nb)
    orc.build_code_points(O.factored_gaussian_icdf(rng.normal(0, 0.2, C), np.exp(rng.uniform(-1, 1, C))))
    return orc.all_code_points


def solve(ops, mu, sg, tab, lam, Nb, layout, mode, want_zhat=True, want_bits=True, level_len=None, view=False, **kw):
    """mu, sg [rows, C] host arrays; layout "bc" (channel-last), "cb" (planes) or "one" (n_ch == 1, 1-D).  view: pass
    device views that start one element past a 16-byte boundary.  Returns (idx, zhat|None, bits|None) as [L, rows, C]."""
    if layout == "one":
        assert mu.shape[1] == 1
        m, s = mu[:, 0], sg[:, 0]
    elif layout == "cb":
        m, s = mu.T, sg.T
    else:
        m, s = mu, sg
    if view:
        m = dev(np.concatenate([[F32(7)], np.ravel(m)]))[1:].view(np.shape(m))
        s = dev(np.concatenate([[F32(1)], np.ravel(s)]))[1:].view(np.shape(s))
        assert m.data_ptr() % 16 == 4
    else:
        m, s = dev(m), dev(s)
    out = ops.quantize(m, s, dev(tab), lam, N=Nb, layout="bc" if layout == "one" else layout, mode=mode, want_zhat=want_zhat,
                       want_bits=want_bits, level_len=None if level_len is None else dev(level_len), **kw)
    out = out if isinstance(out, tuple) else (out,)
    res = []
    for t in out:
        a = host(t)
        res.append(a.transpose(0, 2, 1) if layout == "cb" else (a[:, :, None] if layout == "one" else a))
    idx = res[0]
    zh = res[1] if want_zhat else None
    bt = res[-1] if want_bits else None
    return idx, zh, bt


def check_lambdas(L):
    """The lambdas the exhaustive check covers: all up to 8, else the ends and both sides of each 32-lambda chunk edge."""
    if L <= 8:
        return list(range(L))
    return sorted({0, 1, L - 1} | {i for c in range(32, L, 32) for i in (c - 1, c)})


def check(ops, mu, sg, tab, lam, Nb, layout, mode, want_zhat=True, want_bits=True, level_len=None, view=False, **kw):
    got = solve(ops, mu, sg, tab, lam, Nb, layout, mode, want_zhat, want_bits, level_len, view, **kw)
    want = CO.quantize(mu, sg, tab, lam, N=Nb, level_len=level_len, mode=MODE[mode], want_zhat=True, want_bits=True,
                       threads=8)
    ctx = f"layout={layout} mode={mode} N={Nb} L={len(lam)} shape={mu.shape}"
    assert got[0].shape == want[0].shape, ctx
    assert np.array_equal(got[0], want[0]), ctx
    if want_zhat:
        assert np.array_equal(got[1], want[1]), ctx
    if want_bits:
        assert np.array_equal(got[2], want[2]), ctx
    sel = check_lambdas(len(lam))
    rows = np.arange(mu.shape[0]) if mu.size <= 6000 else np.linspace(0, mu.shape[0] - 1, 6000 // mu.shape[1]).astype(int)
    ll = None if level_len is None else level_len[sel]
    best = R.exhaustive_max(mu[rows], sg[rows], tab, [lam[i] for i in sel], Nb, level_len=ll, mode=mode)
    mine = R.chosen_scores(mu[rows], sg[rows], tab, [lam[i] for i in sel], Nb, got[0][sel][:, rows], level_len=ll, mode=mode)
    assert np.array_equal(mine, best), ctx
    return got


# ------------------------------------------------------------------ both modes through the flat and tiled kernels
@pytest.mark.parametrize("mode", ["f32", "f64"])
@pytest.mark.parametrize("Nb", [4, 5, 6, 7, 8, 9, 10, 11, 12])
def test_bit_depths_both_layouts(ops, mode, Nb):
    rng = np.random.default_rng(100 + Nb + 50 * MODE[mode])
    C, rows = 3, 301
    tab = tables(rng, C, Nb)
    mu, sg = latents(rng, rows, C, tab)
    for layout in (("bc", "cb") if Nb <= 10 else ("cb",)):
        check(ops, mu, sg, tab, LAM6, Nb, layout, mode, want_zhat=layout == "cb", want_bits=True)
    check(ops, mu[:, :1], sg[:, :1], tab[:1], LAM6, Nb, "one", mode)


@pytest.mark.parametrize("mode", ["f32", "f64"])
@pytest.mark.parametrize("Nb", [11, 12])
def test_channel_last_refused_above_ten(ops, mode, Nb):
    from vbq_amd._lib import VBQError
    rng = np.random.default_rng(Nb)
    tab = tables(rng, 2, Nb)
    mu, sg = latents(rng, 10, 2, tab)
    with pytest.raises(VBQError, match=r"failed \(-2\).*planes"):
        ops.quantize(dev(mu), dev(sg), dev(tab), LAM6, N=Nb, mode=mode)


@pytest.mark.parametrize("mode", ["f32", "f64"])
@pytest.mark.parametrize("C,rows", [(1, 1), (1, 4099), (15, 129), (16, 127), (17, 257), (33, 131), (48, 61), (17, 3)])
def test_channel_counts_and_ragged_rows(ops, mode, C, rows):
    rng = np.random.default_rng(7 * C + rows + MODE[mode])
    tab = tables(rng, C, 10)
    mu, sg = latents(rng, rows, C, tab)
    for layout in (("bc", "cb") if C > 1 else ("one",)):
        check(ops, mu, sg, tab, LAM6, 10, layout, mode, want_zhat=rows % 2 == 1, want_bits=rows % 2 == 0)


def lambda_sweep(L):
    lam = list(np.geomspace(1e-3, 1e3, L) * np.sqrt(2.0))         # not f32-representable
    lam[0] = 0.0
    return lam


@pytest.mark.parametrize("mode", ["f32", "f64"])
@pytest.mark.parametrize("L", [1, 31, 32, 33, 70])
def test_lambda_chunks(ops, mode, L):
    rng = np.random.default_rng(L + 10 * MODE[mode])
    C, rows = 17, 203
    tab = tables(rng, C, 10)
    mu, sg = latents(rng, rows, C, tab)
    lam = lambda_sweep(L)
    for layout, wz, wb in (("bc", True, True), ("cb", True, False), ("bc", False, False), ("cb", False, True)):
        check(ops, mu, sg, tab, lam, 10, layout, mode, want_zhat=wz, want_bits=wb)
    check(ops, mu[:, 3:4], sg[:, 3:4], tab[3:4], lam, 10, "one", mode, want_zhat=L % 2 == 0, want_bits=True)


@pytest.mark.parametrize("mode", ["f32", "f64"])
def test_unaligned_views_take_the_scalar_path(ops, mode):
    """Row counts divisible by 4 and 16-byte aligned planes take the 16-byte loads of k_quant_flat; views that start one
    element later take its scalar path.  Same answers."""
    rng = np.random.default_rng(31 + MODE[mode])
    C, rows = 3, 1024
    tab = tables(rng, C, 10)
    mu, sg = latents(rng, rows, C, tab)
    for layout, sl in (("cb", slice(0, 3)), ("one", slice(1, 2))):
        a = check(ops, mu[:, sl], sg[:, sl], tab[sl], LAM6, 10, layout, mode)
        b = check(ops, mu[:, sl], sg[:, sl], tab[sl], LAM6, 10, layout, mode, view=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ inputs that split the score modes
@pytest.fixture(scope="module")
def split_set():
    return mode_splitting_set()


def test_split_set_separates_each_rule(split_set):
    """CPU side: the element set below would catch each of these f64-mode bugs (dozens of elements each)."""
    _, z, _, counts = split_set
    assert all(v >= 40 for v in counts.values()), counts
    assert len(z) < 12000


@pytest.mark.parametrize("mode", ["f32", "f64"])
def test_split_set_through_every_literal_kernel(ops, split_set, mode):
    tab, z, s, _ = split_set
    n = len(z) - len(z) % 3
    check(ops, z[:, None], s[:, None], tab, SPLIT_LAMS, 10, "one", mode)
    tab3 = np.repeat(tab, 3, axis=0)
    mu3, sg3 = z[:n].reshape(-1, 3), s[:n].reshape(-1, 3)
    check(ops, mu3, sg3, tab3, SPLIT_LAMS, 10, "cb", mode, want_bits=False)
    check(ops, mu3, sg3, tab3, SPLIT_LAMS, 10, "bc", mode, want_zhat=False)


@pytest.mark.parametrize("mode", ["f32", "f64"])
def test_split_set_through_the_candidate_solve(ops, split_set, mode):
    """K1c fed the oracle's 21 candidates of the same elements: the same winners as the C oracle."""
    tab, z, s, _ = split_set
    orc = O.ChannelwiseOracle(1, 10)
    orc.build_code_points(O.factored_gaussian_icdf(np.zeros(1), np.ones(1)))
    assert np.array_equal(orc.all_code_points, tab)
    left, right = O.get_all_N_bit_intervals(orc.grids, z[:, None])
    P = O.assemble_candidates(left, right)
    Lraw = O.raw_code_lengths(10, len(z), 1).astype(F32)
    zh, bt = ops.argmax_candidates(dev(P), dev(Lraw), dev(z[:, None]), dev(s[:, None]), SPLIT_LAMS, mode=mode)
    _, wz, wb = CO.quantize(z, s, tab, SPLIT_LAMS, N=10, mode=MODE[mode], want_zhat=True, want_bits=True, threads=8)
    assert np.array_equal(host(zh), wz) and np.array_equal(host(bt), wb)


# ------------------------------------------------------------------ the f32 literal flat kernel
@pytest.mark.parametrize("lam", [[0.0, 1e-13, 0.01, 1.0, 1e25], [1e30, 0.5, 0.0, 7.0, 1e-13, 2.0, 1e25, 0.03],
                                 list(np.geomspace(1e-4, 1e2, 12)) + [1e30]])
def test_f32_flat_sweeps_outside_the_fast_range(ops, lam):
    rng = np.random.default_rng(len(lam))
    C, rows = 5, 777
    tab = tables(rng, C, 10)
    mu, sg = latents(rng, rows, C, tab)
    for wz, wb in ((False, False), (True, True)):
        check(ops, mu, sg, tab, lam, 10, "cb", "f32", want_zhat=wz, want_bits=wb)
        check(ops, mu[:, :1], sg[:, :1], tab[:1], lam, 10, "one", "f32", want_zhat=wz, want_bits=wb)
    ll = (np.arange(11, dtype=F32)[None, None] + rng.uniform(0, 3, (len(lam), C, 11))).astype(F32)
    check(ops, mu, sg, tab, lam, 10, "cb", "f32", level_len=ll)


@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_f32_flat_few_lambdas_with_outputs(ops, L):
    rng = np.random.default_rng(60 + L)
    tab = tables(rng, 2, 10)
    mu, sg = latents(rng, 999, 2, tab)
    lam = [0.0, 1e25, 1e-13, 0.2][:L]
    check(ops, mu, sg, tab, lam, 10, "cb", "f32", want_zhat=True, want_bits=L % 2 == 0)
    check(ops, mu, sg, tab, lam, 10, "cb", "f32", want_zhat=False, want_bits=True)
    check(ops, mu, sg, tab, lam, 10, "cb", "f32", want_zhat=False, want_bits=False)     # the pruned descent
    # the persistent grid (vbq_quantize_rows_f32, workgroups_per_cu = 4): the literal kernel even for indices only
    check(ops, mu, sg, tab, lam, 10, "cb", "f32", want_zhat=False, want_bits=False, workgroups_per_cu=4)
    check(ops, mu[:, :1], sg[:, :1], tab[:1], lam, 10, "one", "f32", want_zhat=False, want_bits=False, workgroups_per_cu=4)


@pytest.mark.parametrize("mode", ["f32", "f64"])
@pytest.mark.parametrize("layout", ["bc", "cb", "one"])
def test_row_chunks_equal_whole(ops, mode, layout):
    """vbq_quantize_rows_f32 chunks (unaligned and empty ones included) reproduce the one-launch result of the literal
    kernels bit for bit; f32 sweeps hold lambda = 0."""
    rng = np.random.default_rng(5 + MODE[mode])
    C = 1 if layout == "one" else 18
    rows = 1031
    tab = tables(rng, C, 10)
    mu, sg = latents(rng, rows, C, tab)
    lam = lambda_sweep(7)
    whole = check(ops, mu, sg, tab, lam, 10, layout, mode)
    m, s = (mu[:, 0], sg[:, 0]) if layout == "one" else ((mu.T, sg.T) if layout == "cb" else (mu, sg))
    m, s = dev(m), dev(s)
    lay = "bc" if layout == "one" else layout
    w = ops.quantize(m, s, dev(tab), lam, N=10, layout=lay, mode=mode, want_zhat=True, want_bits=True)
    for wg in (0, 4):
        idx = torch.full_like(w[0], 0xffff)
        zh, bt = torch.full_like(w[1], -1.0), torch.full_like(w[2], -1.0)
        for a, b in ((0, 0), (0, 1), (1, 130), (130, 130), (130, 517), (517, 1030), (1030, 1031)):
            ops.quantize(m, s, dev(tab), lam, N=10, layout=lay, mode=mode, out_idx=idx, out_zhat=zh, out_bits=bt,
                         rows=(a, b), workgroups_per_cu=wg)
        assert torch.equal(idx.view(torch.int16), w[0].view(torch.int16))
        assert torch.equal(zh, w[1]) and torch.equal(bt, w[2])
    got = host(w[0])
    got = got.transpose(0, 2, 1) if layout == "cb" else (got[:, :, None] if layout == "one" else got)
    assert np.array_equal(got, whole[0])


# ------------------------------------------------------------------ the fast kernels' lambda range, at its edges
LO, HI = 1.9e-12, 1.8e19
EDGES = [LO, np.nextafter(LO, 0.0), np.nextafter(LO, np.inf), HI, np.nextafter(HI, 0.0), np.nextafter(HI, np.inf)]


@pytest.mark.parametrize("size", [3, 16, 32])
@pytest.mark.parametrize("edge", range(len(EDGES)))
def test_fast_range_boundary(ops, size, edge):
    from vbq_amd._lib import VBQError
    lam_e = float(EDGES[edge])
    outside = not (LO <= lam_e <= HI)
    lam = [lam_e] + list(np.geomspace(1e-3, 1e3, size - 1))
    rng = np.random.default_rng(edge * 40 + size)
    C, rows = 2, 513
    tab = tables(rng, C, 10)
    mu, sg = latents(rng, rows, C, tab)
    want = check(ops, mu, sg, tab, lam, 10, "cb", "f32", want_zhat=False, want_bits=False)
    check(ops, mu[:, :1], sg[:, :1], tab[:1], lam, 10, "one", "f32", want_zhat=False, want_bits=False)
    check(ops, mu, sg, tab, lam, 10, "cb", "f32")
    lev = O.levels_of_sorted_ranks(10)[want[0]]
    hist = np.stack([[np.bincount(lev[l, :, c], minlength=11) for c in range(C)] for l in range(size)])
    for layout, m, s in (("cb", mu.T, sg.T), ("bc->cb", mu, sg)):
        if outside:
            with pytest.raises(VBQError, match=r"failed \(-2\)"):
                ops.level_counts(dev(m), dev(s), dev(tab), lam, N=10, layout=layout)
        else:
            assert np.array_equal(host(ops.level_counts(dev(m), dev(s), dev(tab), lam, N=10, layout=layout)), hist)
    # channel-last in, planes out: the fast kernels only, once the pruned descent (L <= 4, indices only) does not take it
    for kw in ([{"want_zhat": True}, {}] if size > 4 else [{"want_zhat": True}]):
        if outside:
            with pytest.raises(VBQError, match=r"failed \(-2\).*fast f32 kernel"):
                ops.quantize(dev(mu), dev(sg), dev(tab), lam, N=10, layout="bc->cb", **kw)
        else:
            got = ops.quantize(dev(mu), dev(sg), dev(tab), lam, N=10, layout="bc->cb", **kw)
            got = got[0] if isinstance(got, tuple) else got
            assert np.array_equal(host(got).transpose(0, 2, 1), want[0])


def test_refusals(ops):
    from vbq_amd import _lib
    from vbq_amd._lib import VBQError
    rng = np.random.default_rng(1)
    tab = tables(rng, 2, 10)
    mu, sg = latents(rng, 64, 2, tab)
    ll = np.tile(np.arange(11, dtype=F32), (2, 2, 1))
    with pytest.raises(VBQError, match=r"failed \(-2\).*raw integer lengths"):
        ops.quantize(dev(mu.T), dev(sg.T), dev(tab), [0.5, 1.0], N=10, layout="cb", mode="f64", level_len=dev(ll))
    m, s, t = dev(mu.T), dev(sg.T), dev(tab)
    idx = torch.empty((1, 2, 64), dtype=torch.uint16, device="cuda")
    wsb = _lib.lib().vbq_quantize_workspace_bytes(2, 1, 10)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    r = _lib.lib().vbq_quantize_f32(ops._ptr(m), ops._ptr(s), 64, 2, _lib.LAYOUT_CB, ops._ptr(t), None, ops._doubles([0.5]),
                                    1, 10, 7, ops._ptr(idx), None, None, ops._ptr(ws), wsb, ops._stream(m))
    assert r == -1 and "unknown mode 7" in _lib.lib().vbq_last_error().decode()
    for Nb in (3, 13):
        t = np.zeros((2, 2 ** (Nb + 1) - 1), F32)
        for mode in ("f32", "f64"):
            with pytest.raises(VBQError, match=r"failed \(-2\).*N=%d not built" % Nb):
                ops.quantize(dev(mu.T), dev(sg.T), dev(t), [0.5], N=Nb, layout="cb", mode=mode)


# ------------------------------------------------------------------ vbq_n_bit_intervals_f32
@pytest.mark.parametrize("Nb", [4, 5, 6, 7, 8, 9, 10, 11, 12])
def test_n_bit_intervals_all_depths(ops, Nb):
    """ChannelwisePriorCDFQuantizer.get_all_N_bit_intervals against the NumPy oracle: z below the first point, above
    the last (the deepest level has no edge padding), exactly on points and between them."""
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    rng = np.random.default_rng(Nb)
    C = 3
    mean, std = rng.normal(0, 0.3, C), np.exp(rng.uniform(-1, 1, C))
    q = ChannelwisePriorCDFQuantizer(C, Nb)
    q.build_code_points(priors.FactoredGaussianPrior(mean, std))
    grids = q._search_grids
    allp = q.code_points_by_channel                         # every level's points, sorted
    srt = np.sort(q.all_code_points[:, 2 ** Nb - 1:], axis=1)     # the deepest level's points
    B = 600
    Z = (std * rng.normal(0, 1.5, (B, C))).astype(F32)
    Z[:100] = allp[:, rng.integers(0, allp.shape[1], 100)].T                       # exactly on points of every level
    Z[100:110] = allp[:, 0] - F32(1.0)
    Z[110:120] = np.nextafter(allp[:, 0], F32(-np.inf))
    Z[120:130] = allp[:, -1] + F32(1.0)
    Z[130:140] = np.nextafter(allp[:, -1], F32(np.inf))
    Z[140:150] = srt[:, -1]
    Z[150:160] = np.nextafter(srt[:, -2], F32(np.inf))
    Z[160:170] = srt[:, 0]
    left, right = q.get_all_N_bit_intervals(Z)
    lo, ro = O.get_all_N_bit_intervals(grids, Z)
    assert np.array_equal(host(left), lo) and np.array_equal(host(right), ro)
