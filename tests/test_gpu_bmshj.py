"""The K4 BMSHJ2018 prior kernels (vbq_bmshj.hip) against the float64 reference of oracle/bmshj_f64.py
(pdf by autograd, not by the analytic chain the kernels use), at every dispatch branch of the
launchers, and the device-side stopping rule of the inverse-cdf chain against a step-by-step host
loop, bit for bit.

The bounds (cdf 5e-7, pdf 5e-6 x the channel's max pdf, |cdf64(z) - xi| 5e-7) are about 3x what
the float32 NumPy restatement reaches on a CPU (tests/test_bmshj_f64.py pins them there).  Each
comparison prints its worst error next to its bound (run with -s to see them)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import bmshj_f64 as R
from oracle import vbq_oracle as O

pytestmark = pytest.mark.gpu
FLT_MAX = float(np.finfo(np.float32).max)
LOG_EPS = float(np.float32(np.log(np.float32(1e-10))))       # log(pdf + 1e-10) where the f32 pdf is 0, correctly rounded
ULP_LOG_EPS = abs(float(np.spacing(np.float32(LOG_EPS))))
CDF_TOL, PDF_TOL, ICDF_TOL = 5e-7, 5e-6, 5e-7


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a ROCm device")
    from vbq_amd import ops as _ops
    return _ops


def _prior(C, init_scale=10.0, seed=0, sd=0.3):
    from vbq_amd import priors
    p = priors.BMSHJ2018Prior(C, init_scale=init_scale, seed=seed)
    if sd:
        rng = np.random.default_rng(seed + 1000)
        p.set_weights([w + rng.normal(0, sd, w.shape).astype(np.float32) for w in p.get_weights()])
    return p


def _steep_prior(C):
    """Zero biases and factors, effective matrices 200: logits = 200 * 600^3 * x, so every root of
    cdf = xi lies within 2e-10 of 0 and the bisection halves its [-1, 1] bracket exactly for more than
    50 steps -- the stops at steps 47-49 below are reachable."""
    p = _prior(C, sd=0)
    w = p.get_weights()
    p.set_weights([np.full_like(a, 200.0) if k % 3 == 0 else np.zeros_like(a)
                   for k, a in enumerate(w[:9])] + [np.full_like(w[9], 200.0), np.zeros_like(w[10])])
    return p


def _x(shape, seed):
    """|x| log-uniform in [1e-6, 100], both signs, f32 on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    mag = 10.0 ** (torch.rand(shape, generator=g, device="cuda", dtype=torch.float64) * 8 - 6)
    sign = torch.where(torch.rand(shape, generator=g, device="cuda") < 0.5, -1.0, 1.0)
    return (sign * mag).float().contiguous()


def _report(name, err, bound):
    """Print the worst error next to the bound it is held to (for element-wise bounds, at the element with the worst
    ratio); True when every element is within its bound."""
    err = err.double()
    bound = torch.as_tensor(bound, dtype=torch.float64, device=err.device).expand_as(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound).flatten()
    i = int(torch.argmax(ratio))
    print(f"\nBOUND {name}: max err {float(err.max()):.3g}; worst err/bound {float(ratio[i]):.3g} "
          f"(err {float(err.flatten()[i]):.3g} <= {float(bound.flatten()[i]):.3g})")
    return bool(torch.all(err <= bound))


# ---------------------------------------------------------------------------------------- cdf / pdf / logpdf
# (rows..., C): E = rows * C elements; staged = C * 43 * 4 <= 48 KB and E > 7 * 256; capped grid (2 x CUs staged, 4096
# otherwise) with a grid-stride loop when E / 256 exceeds it
CDF_SHAPES = [
    (100, 7),               # 700 elements: unstaged, small
    (777, 16),              # staged, not a multiple of 256 rows
    (65536, 256),           # staged, capped grid, grid-stride
    (4000001, 1),           # staged, C = 1, capped grid, grid-stride
    (1000, 285),            # staged with 49 020 B of LDS
    (1000, 286),            # unstaged: 49 192 B > 48 KB
    (4000, 320),            # unstaged, 5000 blocks -> 4096, grid-stride
    (2, 17, 23, 192),       # 4-D [B, H, W, C]
]


@pytest.mark.parametrize("shape", CDF_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cdf_pdf_vs_f64(ops, shape):
    C = shape[-1]
    p = _prior(C, init_scale=1.0 if C in (7, 285) else 10.0, seed=C)
    params = p._params()
    x = _x(shape, seed=C)
    cdf, pdf, lp = ops.bmshj_cdf_pdf(params, x, cdf=True, pdf=True, logpdf=True)
    # each output alone is the all-outputs call, bit for bit
    assert torch.equal(ops.bmshj_cdf_pdf(params, x, cdf=True, pdf=False)[0], cdf)
    assert torch.equal(ops.bmshj_cdf_pdf(params, x, cdf=False, pdf=True)[1], pdf)
    assert torch.equal(ops.bmshj_cdf_pdf(params, x, cdf=False, pdf=False, logpdf=True)[2], lp)
    c64 = R.cdf64(params, x)
    p64 = R.pdf64(params, x)
    pmax = R.pdf_max64(params, x)                                          # [C], broadcasts over [..., C]
    assert _report(f"cdf {shape}", (cdf.double() - c64).abs(), CDF_TOL)
    assert _report(f"pdf {shape}", (pdf.double() - p64).abs(), (PDF_TOL * pmax).expand_as(p64))
    # the pdf bound carried through log(pdf + 1e-10), plus rounding of a result of magnitude <= 23.03 (ulp 1.9e-6)
    lb = PDF_TOL * pmax / (p64 + 1e-10) + 1e-6
    assert _report(f"logpdf {shape}", (lp.double() - torch.log(p64 + 1e-10)).abs(), lb)


@pytest.mark.parametrize("rows", [1, 400], ids=["unstaged", "staged"])
def test_cdf_pdf_tails(ops, rows):
    """The documented f32 semantics far out: cdf saturates to exactly 0 / 1, pdf to exactly 0 and logpdf to the device's
    logf(1e-10f) everywhere.  logf is faithfully rounded (<= 1 ulp), and log(1e-10) lies 0.32 ulp from its nearest
    float32, so that constant is float32(log(1e-10)) or its neighbour (on an MI355X: the neighbour)."""
    C = 8
    params = _prior(C, 10.0, seed=1)._params()
    v = torch.tensor([np.inf, -np.inf, FLT_MAX, -FLT_MAX, 1e30, -1e30], dtype=torch.float32, device="cuda")
    x = v[:, None].expand(6, C).repeat(rows, 1).contiguous()
    cdf, pdf, lp = ops.bmshj_cdf_pdf(params, x, logpdf=True)
    assert torch.equal(cdf, (x > 0).float())
    assert torch.all(pdf == 0)
    assert torch.all(lp == lp[0, 0]) and abs(float(lp[0, 0]) - LOG_EPS) <= ULP_LOG_EPS


def test_cdf_pdf_nan_and_monotone(ops):
    C = 16
    params = _prior(C, 10.0, seed=2)._params()
    x = torch.sort(_x((2000, C), seed=3), dim=0).values                     # staged: 32 000 elements
    cdf, pdf, lp = ops.bmshj_cdf_pdf(params, x, logpdf=True)
    assert torch.all(cdf[1:] >= cdf[:-1]) and torch.all(pdf >= 0)
    xn = x.clone()
    hole = torch.zeros_like(x, dtype=torch.bool)
    hole[[5, 6, 1000, 1999], [0, 3, 15, 7]] = True
    xn[hole] = float("nan")
    for got, want in zip(ops.bmshj_cdf_pdf(params, xn, logpdf=True), (cdf, pdf, lp)):
        assert torch.all(torch.isnan(got[hole]))
        assert torch.equal(got[~hole], want[~hole])                         # the neighbours are untouched


# ---------------------------------------------------------------------------------------- inverse cdf / code points
@pytest.mark.parametrize("C,N,sd", [(256, 10, 0.0), (320, 10, 0.2), (16, 12, 0.2)])
def test_inverse_cdf_table_vs_f64(C, N, sd):
    """[2047, 256] at init_scale 10 is the table bench.py times (staged chain); C = 320 runs the unstaged chain."""
    from vbq_amd import ChannelwisePriorCDFQuantizer
    p = _prior(C, 10.0, seed=0, sd=sd)
    xi1 = O.dyadic_xi(N)
    xi = np.repeat(xi1[:, None], C, axis=1)
    z = p.inverse_cdf(xi)
    assert z.dtype == np.float32 and z.shape == xi.shape
    err = (R.cdf64(p._params(), torch.from_numpy(z).cuda()) - torch.from_numpy(xi).cuda()).abs()
    assert _report(f"icdf C={C} N={N}", err, ICDF_TOL)
    assert np.all(np.diff(z[np.argsort(xi1)], axis=0) > 0)                    # strictly increasing in xi, every channel
    q = ChannelwisePriorCDFQuantizer(C, N)
    q.build_code_points(p)
    assert np.array_equal(q.all_code_points, z.T)


def test_inverse_cdf_channel_without_bracket(ops):
    """Raw matrices of -200 are 0 after the float32 softplus: that channel's cdf is flat, never crosses xi, and the
    bracket doubling used to spin forever at -inf / +inf."""
    p = _prior(4, 10.0, seed=2, sd=0)
    w = p.get_weights()
    for k in (0, 3, 6, 9):                                                  # the four matrices
        w[k][2] = -200.0
    p.set_weights(w)
    with pytest.raises(ValueError, match="channel 2"):
        p.inverse_cdf(np.full((9, 4), 0.3))


# ---- the chain (k_bmshj_icdf_chain, 48 steps per launch batch) against one k_bmshj_icdf_step per host iteration
def _bracket(ops, params, xi_t):
    def f(z):
        return ops.bmshj_cdf_pdf(params, z, cdf=True, pdf=False)[0] - xi_t
    left = torch.full_like(xi_t, -1.0)
    right = torch.full_like(xi_t, 1.0)
    while not bool(torch.all(f(left) < 0)):
        left = left * 2
    while not bool(torch.all(f(right) > 0)):
        right = right * 2
    return left, right


def _step_loop(ops, p, xi_t, max_iterations, tol):
    """learned_prior.py:196-211 literally, one step kernel per iteration: preset the flags, step, read the flags, apply
    the rule.  Returns mid, the last iteration and the minimum bracket width after every step."""
    params = p._params()
    left, right = _bracket(ops, params, xi_t)
    mid = torch.empty_like(xi_t)
    flags = torch.empty(2, dtype=torch.int32, device=xi_t.device)
    tol32 = np.float32(tol)
    its, widths = 0, []
    for i in range(max_iterations):
        flags[0], flags[1] = 0, 0x7f800000
        ops.bmshj_icdf_step(params, xi_t, left, right, mid, flags)
        nz, wb = flags.cpu().numpy().view(np.uint32)
        w = np.uint32(wb).view(np.float32)
        widths.append(w)
        its = i
        if nz == 0 or w <= tol32:
            break
    return mid, its, widths


def _bits(t):
    return t.view(torch.int32)


def _compare(ops, p, xi_t, max_iterations, tol):
    mid, its, widths = _step_loop(ops, p, xi_t, max_iterations, tol)
    z = p.inverse_cdf(xi_t, max_iterations=max_iterations, tol=tol)
    assert p.last_iterations == its
    assert torch.equal(_bits(z), _bits(mid))
    return its, widths


_CASES = {}


def _case(kind, size):
    """(prior, xi) for the chain tests: a 'wide' fitted-like prior or the 'steep' one, on the staged chain
    (2047 x 16: 32 752 points, 2 752 B of LDS) or the unstaged one (C = 320: 55 040 B)."""
    key = (kind, size)
    if key not in _CASES:
        C, rows = (16, 2047) if size == "staged" else (320, 64)
        p = _prior(C, 10.0, seed=7) if kind == "wide" else _steep_prior(C)
        g = torch.Generator(device="cuda").manual_seed(11)
        xi = (torch.rand((rows, C), generator=g, device="cuda") * 0.998 + 0.001).contiguous()
        if size == "staged" and kind == "wide":
            xi = torch.from_numpy(np.repeat(O.dyadic_xi(10)[:, None], C, axis=1).astype(np.float32)).cuda()
        _CASES[key] = (p, xi)
    return _CASES[key]


KINDS = ["wide", "steep"]
SIZES = ["staged", "unstaged"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("tol", [1e-9, 0.0], ids=["tol_default", "tol0"])
@pytest.mark.parametrize("max_iterations", [1, 47, 48, 49, 96, 97, 1000])
def test_chain_matches_step_loop_max_iterations(ops, kind, size, tol, max_iterations):
    p, xi = _case(kind, size)
    its, _ = _compare(ops, p, xi, max_iterations, tol)
    if tol == 0.0:
        assert its == max_iterations - 1                                  # tol 0: max_iterations cuts the search


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", SIZES)
def test_chain_matches_step_loop_tol(ops, kind, size):
    p, xi = _case(kind, size)
    its, _ = _compare(ops, p, xi, 1000, 1e-2)                               # stops early
    assert its < 20
    _, _, widths = _step_loop(ops, p, xi, 64, 0.0)
    # a tol equal to the minimum width after step k stops the search at k exactly: k on either side of the
    # first chain boundary
    hit = []
    for k in (47, 48, 49):
        if widths[k] < widths[k - 1]:
            assert _compare(ops, p, xi, 1000, float(widths[k]))[0] == k
            hit.append(k)
    if kind == "steep":
        assert hit == [47, 48, 49]
    # a power of two equal to a width the search reaches: `<=` stops at that step, `<` would take one more (the steep
    # prior's bracket [-1, 1] halves exactly: width 2^-k after step k)
    pow2 = [k for k in range(10, 40) if np.frexp(widths[k])[0] == 0.5 and widths[k] < widths[k - 1]]
    if kind == "steep":
        assert 20 in pow2 and widths[20] == 2.0 ** -20
    for k in pow2[:1] + ([20] if kind == "steep" else []):
        assert _compare(ops, p, xi, 1000, float(widths[k]))[0] == k


@pytest.mark.parametrize("size", SIZES)
def test_chain_all_mid_values_zero(ops, size):
    """xi = the kernel's own cdf(0): the bracket stays [-1, 1], the first mid is 0 and f(mid) == 0 everywhere, so the
    search ends at iteration 0 with mid == 0."""
    p, xi = _case("wide", size)
    c0 = ops.bmshj_cdf_pdf(p._params(), torch.zeros_like(xi), cdf=True, pdf=False)[0]
    its, _ = _compare(ops, p, c0, 1000, 1e-9)
    assert its == 0
    assert torch.all(p.inverse_cdf(c0) == 0)


# ---------------------------------------------------------------------------------------- the fit pass
def _nll_data(params, C, n, seed):
    """x_cb [C, n] f32 with every f64 logit inside [-12, 12]: uniform between neighbouring roots of cdf64 at 257
    logits equally spaced in [-12, 12] (so f32 sigmoid saturation cannot make the reference diverge)."""
    lg = torch.linspace(-12, 12, 257, dtype=torch.float64, device="cuda")
    q = R.root64(params, torch.sigmoid(lg)[:, None].expand(257, C)).t().contiguous()     # [C, 257]
    g = torch.Generator(device="cuda").manual_seed(seed)
    idx = torch.randint(0, 256, (C, n), generator=g, device="cuda")
    u = torch.rand((C, n), generator=g, device="cuda", dtype=torch.float64)
    lo = torch.gather(q, 1, idx)
    hi = torch.gather(q, 1, idx + 1)
    return (lo + (hi - lo) * u).float().contiguous()


# (C, n): one block per channel; the 4096 / C + 1 cap with the grid-stride loop; a 4097-block grid
NLL_SHAPES = [(1, 1), (1, 255), (3, 2049), (192, 65553), (256, 65536), (320, 4097), (1, 10000003)]


@pytest.mark.parametrize("C,n", NLL_SHAPES, ids=lambda v: str(v))
def test_nll_grad_vs_f64(ops, C, n):
    p = _prior(C, init_scale=2.0 if C % 2 else 10.0, seed=C + n, sd=0.2)
    params = p._params()
    x_cb = _nll_data(params, C, n, seed=n)
    out = ops.bmshj_nll_grad(params, x_cb)
    ref, absg = R.nll_grad64(params, x_cb)
    # the loss bound adds, per element, the f32 cancellation in the kernel's pdf = s (1 - s) u (learned_prior.py:305): s is
    # rounded to <= 1 ulp (2^-24) of 1, so 1 - s, the pdf and l_i = -log(pdf) carry an error of up to 2^-24 / (1 - s) =
    # 2^-24 (1 + e^lg) -- about 1e-2 at lg = 12.  The f32 restatement does the same; the gradient needs no such term.
    lg = R.logits64(params.double(), x_cb.double().t())
    cancel = (2.0 ** -24 * (1 + torch.exp(lg))).sum(dim=0)
    assert _report(f"nll loss C={C} n={n}", (out[:, 43] - ref[:, 43]).abs(), 1e-5 * absg[:, 43] + cancel)
    assert _report(f"nll grad C={C} n={n}", (out[:, :43] - ref[:, :43]).abs(), 1e-4 * absg[:, :43])
    # column 43 is -sum(logpdf) of the cdf_pdf kernel on the same data (bound relative to sum |logpdf|)
    lp = ops.bmshj_cdf_pdf(params, x_cb.t().contiguous(), cdf=False, pdf=False, logpdf=True)[2].double()
    assert _report(f"nll vs -sum(logpdf) C={C} n={n}", (out[:, 43] + lp.sum(dim=0)).abs(), 1e-5 * lp.abs().sum(dim=0))


def test_nll_grad_saturated(ops):
    """Elements where the f32 pdf is exactly 0 add exactly -logf(1e-10f) each -- the constant the cdf_pdf kernel gives as
    their logpdf (one element per thread, summed exactly in f64) -- and leave the gradient finite."""
    C = 2
    params = _prior(C, 10.0, seed=3)._params()
    v = torch.tensor([1e30, -1e30, 1e6, -1e6, 3e4, -3e4], dtype=torch.float32, device="cuda")
    x_cb = v[None, :].expand(C, 6).contiguous()
    _, pdf, lp = ops.bmshj_cdf_pdf(params, x_cb.t().contiguous(), cdf=False, pdf=True, logpdf=True)
    assert torch.all(pdf == 0) and torch.all(lp == lp[0, 0]) and abs(float(lp[0, 0]) - LOG_EPS) <= ULP_LOG_EPS
    out = ops.bmshj_nll_grad(params, x_cb)
    assert torch.all(out[:, 43] == 6 * -float(lp[0, 0]))
    assert torch.all(torch.isfinite(out[:, :43]))


def test_loss_and_grads_c256_vs_f64_autograd():
    """BMSHJ2018Prior.loss_and_grads (the kernel, then the softplus / tanh chain to the raw variables on the host) at
    C = 256 against f64 autograd from the raw variables."""
    C, n = 256, 4096
    p = _prior(C, 2.0, seed=5, sd=0.2)
    params = p._params()
    x_cb = _nll_data(params, C, n, seed=6)
    loss, grads = p.loss_and_grads(x_cb)
    raw = [torch.tensor(w, dtype=torch.float64, device="cuda", requires_grad=True) for w in p.get_weights()]
    mats = [torch.nn.functional.softplus(raw[k]) for k in (0, 3, 6, 9)]
    bias = [raw[k] for k in (1, 4, 7, 10)]
    fac = [torch.tanh(raw[k]) for k in (2, 5, 8)]
    P = R.pack64(mats, bias, fac)
    xx = x_cb.double().requires_grad_(True)
    cdf = torch.sigmoid(R.logits64(P, xx.t()))
    pdf, = torch.autograd.grad(cdf.sum(), xx, create_graph=True)
    li = -torch.log(pdf + 1e-10)
    ref = li.mean()
    ref.backward()
    # bounds: the loss to 1e-5 of mean |l_i|; each gradient to 1e-4 of sum_i |dl_i/dtheta| / (n C) carried through the
    # chain factor of its raw variable (sigmoid for a matrix, 1 - tanh^2 for a factor, 1 for a bias)
    assert _report("loss_and_grads loss C=256", torch.tensor(abs(loss - float(ref.detach())), dtype=torch.float64),
                   1e-5 * float(li.detach().abs().mean()))
    _, absg = R.nll_grad64(params, x_cb)
    a = absg[:, :43].cpu().numpy() / (n * C)
    o = 0
    for k, (g, r) in enumerate(zip(grads, raw)):
        size = r[0].numel()
        chain = torch.sigmoid(r) if k % 3 == 0 else (1 - torch.tanh(r) ** 2 if k % 3 == 2 and k < 9 else torch.ones_like(r))
        bound = torch.from_numpy(a[:, o:o + size].reshape(r.shape)).cuda() * chain.detach()
        o += size
        assert g.shape == tuple(r.shape)
        assert _report(f"loss_and_grads grad[{k}] C=256", (torch.from_numpy(g).cuda().double() - r.grad).abs(), 1e-4 * bound)
