"""The float64 BMSHJ2018 reference (oracle/bmshj_f64.py) against the float32 NumPy restatement, and
the argument checks of BMSHJ2018Prior.inverse_cdf.  CPU only: the reference is pinned here before
any GPU test leans on it."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import bmshj_f64 as R
from oracle import vbq_oracle as O
from vbq_amd import priors


def _prior_params(C, init_scale, seed):
    """Effective [C, 43] parameters of an initial prior with perturbed weights, and the f32 restatement."""
    rng = np.random.default_rng(seed)
    p = priors.BMSHJ2018Prior(C, init_scale=init_scale, seed=seed)
    p.set_weights([w + rng.normal(0, 0.3, w.shape).astype(np.float32) for w in p.get_weights()])
    eff = p.effective_parameters()
    return priors.pack_bmshj_params(*eff), O.BMSHJ2018Oracle(*eff)


def _x(rng, rows, C):
    """|x| log-uniform in [1e-6, 100], both signs."""
    return (rng.choice([-1.0, 1.0], (rows, C)) * 10.0 ** rng.uniform(-6, 2, (rows, C))).astype(np.float32)


@pytest.mark.parametrize("C", [7, 256, 320])
@pytest.mark.parametrize("init_scale", [1.0, 10.0])
def test_f64_reference_vs_f32_restatement(C, init_scale):
    params, orc = _prior_params(C, init_scale, seed=C)
    x = _x(np.random.default_rng(C + 1), 600 if C == 7 else 60, C)
    c32, p32 = orc.cdf_pdf(x)
    c64 = R.cdf64(params, x).numpy()
    p64 = R.pdf64(params, x).numpy()
    pmax = R.pdf_max64(params, x).numpy()
    # measured for the f32 restatement: |cdf err| <= 1.7e-7, |pdf err| <= 8.4e-7 max
    assert np.abs(c32 - c64).max() <= 5e-7
    assert np.all(np.abs(p32 - p64) <= 5e-6 * pmax)
    assert np.all(p64 >= 0) and np.all((c64 >= 0) & (c64 <= 1))
    # the oracle's inverse cdf on the N = 10 dyadic grid (measured <= 1.2e-7)
    xi = np.repeat(O.dyadic_xi(10)[:, None], C, axis=1).astype(np.float32)
    if C != 7:
        xi = xi[::16]
    z = orc.inverse_cdf(xi)
    assert np.abs(R.cdf64(params, z).numpy() - xi).max() <= 5e-7
    # root64 solves cdf64(z) = xi to f64 precision, and the f32 z lies within the bound's width of it
    r = R.root64(params, xi)
    assert np.abs(R.cdf64(params, r).numpy() - xi).max() <= 1e-13
    pr = np.minimum(R.pdf64(params, r).numpy(), R.pdf64(params, z).numpy())
    assert np.all(np.abs(z - r.numpy()) <= 2 * 5e-7 / pr + np.spacing(np.abs(z)))


def test_f64_pdf_matches_finite_difference():
    """pdf64 (autograd) against a central difference of cdf64 in f64."""
    params, _ = _prior_params(5, 10.0, seed=9)
    x = torch.linspace(-30, 30, 601, dtype=torch.float64)[:, None].expand(601, 5).contiguous()
    h = 1e-5
    fd = (R.cdf64(params, x + h) - R.cdf64(params, x - h)) / (2 * h)
    assert torch.allclose(R.pdf64(params, x), fd, rtol=1e-6, atol=1e-12)


def test_nll_grad64_vs_finite_difference():
    """The per-element broadcast of nll_grad64 gives the gradient of its own loss (central differences
    in f64 on every parameter), and sum |dl_i| bounds |sum dl_i|."""
    params, _ = _prior_params(2, 1.0, seed=4)
    rng = np.random.default_rng(5)
    x_cb = rng.normal(0, 1.5, (2, 50))
    out, absg = R.nll_grad64(params, x_cb, chunk=37)                 # several chunks
    full, _ = R.nll_grad64(params, x_cb)
    assert torch.allclose(out, full, rtol=1e-12, atol=1e-12)
    P = torch.tensor(params, dtype=torch.float64)
    xt = torch.tensor(x_cb)

    def loss(Pc):
        xx = xt.clone().requires_grad_(True)
        with torch.enable_grad():
            c = torch.sigmoid(R.logits64(Pc, xx.t()))
            pdf, = torch.autograd.grad(c.sum(), xx)
        return -torch.log(pdf + 1e-10).sum(dim=1)
    assert torch.allclose(out[:, 43], loss(P), rtol=1e-12)
    h = 1e-6
    for k in range(43):
        e = torch.zeros_like(P)
        e[:, k] = h
        fd = (loss(P + e) - loss(P - e)) / (2 * h)
        assert torch.allclose(out[:, k], fd, rtol=1e-5, atol=1e-6), k
    assert torch.all(absg >= out.abs() * (1 - 1e-12))


@pytest.mark.parametrize("bad", [0.0, 1.0, -0.25, 1.5, np.nan, np.inf, -np.inf, 1 - 1e-9])
def test_inverse_cdf_rejects_xi_outside_unit_interval(bad, monkeypatch):
    """An xi <= 0, >= 1 (1 - 1e-9 is 1.0 as a float32) or NaN made the bracket doubling spin forever; it is
    refused before anything touches a device."""
    def no_device():
        raise AssertionError("inverse_cdf reached the device with a bad xi")
    monkeypatch.setattr(priors, "_device", no_device)
    p = priors.BMSHJ2018Prior(3, init_scale=10.0, seed=0)
    xi = np.full((5, 3), 0.5)
    xi[2, 1] = bad
    with pytest.raises(ValueError, match="xi"):
        p.inverse_cdf(xi)
    with pytest.raises(ValueError, match="xi"):
        p.inverse_cdf(torch.from_numpy(xi))
