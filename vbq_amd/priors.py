"""Priors whose inverse CDF defines the code-point tables.

    StandardGaussianPrior / FactoredGaussianPrior   img-compression/vae_models.py:14-43
    BMSHJ2018Prior                                  img-compression/learned_prior.py:6-334

The Gaussian priors are table builders: 2047*C calls of scipy's ppf on the host, exactly as the
reference does.  BMSHJ2018Prior evaluates cdf / pdf / logpdf and the bisection inverse CDF with
the K4 HIP kernels.  Its TF numerics are not reproducible here (no TensorFlow, no stored table
in the reference), so parity for this class is "unpinned": tests check self-consistency and
agreement with the NumPy restatement in oracle/ to float tolerance.
"""
from __future__ import annotations

from functools import partial

import numpy as np
import torch

from . import ops

log2pi = np.log(2.0 * np.pi).astype("float32")


def log_normal_pdf(sample, mean, logvar):
    """vae_models.py:9-11."""
    return -0.5 * ((sample - mean) ** 2.0 * np.exp(-logvar) + logvar + log2pi)


class StandardGaussianPrior:
    @staticmethod
    def logpdf(z):
        return log_normal_pdf(z, 0.0, 0.0)

    @staticmethod
    def pdf(z):
        return np.exp(StandardGaussianPrior.logpdf(z))

    @staticmethod
    def inverse_cdf(xi):
        from scipy.stats import norm
        return norm.ppf(xi)


class FactoredGaussianPrior:
    def __init__(self, mean, std):
        self.mean = np.asarray(mean)
        self.std = np.asarray(std)
        self.logvar = 2 * np.log(self.std)

    def logpdf(self, z):
        return log_normal_pdf(z, self.mean, self.logvar)

    def pdf(self, z):
        return np.exp(self.logpdf(z))

    def inverse_cdf(self, xi):
        from scipy.stats import norm
        assert xi.shape[-1] == len(self.mean)
        return norm.ppf(xi, loc=self.mean, scale=self.std)


def pack_bmshj_params(matrices, biases, factors) -> np.ndarray:
    """Effective BMSHJ2018 parameters -> [C, 43] in the order include/vbq.h documents."""
    C = matrices[0].shape[0]
    parts = []
    for i in range(4):
        parts.append(np.asarray(matrices[i], np.float32).reshape(C, -1))
        parts.append(np.asarray(biases[i], np.float32).reshape(C, -1))
        if i < 3:
            parts.append(np.asarray(factors[i], np.float32).reshape(C, -1))
    out = np.concatenate(parts, axis=1)
    assert out.shape == (C, 43)
    return np.ascontiguousarray(out)


_device = partial(ops.current_device, "BMSHJ2018Prior")        # a name of its own: tests put a tripwire here


class BMSHJ2018Prior:
    """Per-channel non-parametric CDF of Balle et al. 2018 (learned_prior.py:6-58).

    Raw variables matrix_i / bias_i / factor_i are kept as float32 NumPy arrays with the
    reference's shapes; softplus / tanh are applied when a method is called (the reference
    applies them once in __init__, learned_prior.py:43,57 -- SURVEY 7.2 item 7)."""

    def __init__(self, channels, dims=(3, 3, 3), init_scale=10.0, seed=None, **kwargs):
        self._channels = int(channels)
        self._init_scale = float(init_scale)
        self._dims = tuple(int(f) for f in dims)
        if self._dims != (3, 3, 3):
            raise ValueError("the HIP kernels are built for dims=(3, 3, 3) (the reference default and the only "
                             "setting post_process.py:78 uses)")
        d = (1,) + self._dims + (1,)
        scale = self._init_scale ** (1 / (len(self._dims) + 1))
        rng = np.random.default_rng(seed)
        self.matrices, self.biases, self.factors = [], [], []
        for i in range(len(self._dims) + 1):
            init = np.log(np.expm1(1 / scale / d[i + 1]))
            self.matrices.append(np.full((self._channels, d[i + 1], d[i]), init, dtype=np.float32))
            self.biases.append(rng.uniform(-0.5, 0.5, (self._channels, d[i + 1], 1)).astype(np.float32))
            if i < len(self._dims):
                self.factors.append(np.zeros((self._channels, d[i + 1], 1), dtype=np.float32))
        self._params_dev = None

    init_scale = property(lambda self: self._init_scale)
    dims = property(lambda self: self._dims)
    channels = property(lambda self: self._channels)

    # ---- weights ----------------------------------------------------------------------------
    def get_weights(self):
        out = []
        for i in range(4):
            out += [self.matrices[i], self.biases[i]] + ([self.factors[i]] if i < 3 else [])
        return out

    def set_weights(self, weights):
        it = iter(weights)
        for i in range(4):
            self.matrices[i] = np.asarray(next(it), np.float32)
            self.biases[i] = np.asarray(next(it), np.float32)
            if i < 3:
                self.factors[i] = np.asarray(next(it), np.float32)
        self._params_dev = None

    def save_weights(self, path):
        np.savez(path, *self.get_weights(), channels=self._channels, init_scale=self._init_scale)

    def load_weights(self, path):
        z = np.load(path)
        self.set_weights([z[f"arr_{i}"] for i in range(11)])

    def effective_parameters(self):
        sp = [np.logaddexp(np.float32(0), m).astype(np.float32) for m in self.matrices]       # softplus (:43)
        return sp, self.biases, [np.tanh(f).astype(np.float32) for f in self.factors]       # tanh (:57)

    def _params(self):
        if self._params_dev is None:
            self._params_dev = torch.from_numpy(pack_bmshj_params(*self.effective_parameters())).to(_device())
        return self._params_dev

    # ---- evaluation (learned_prior.py:109-171, 235-334) ---------------------------------------
    def _x(self, inputs):
        t = ops.upload(inputs, _device(), torch.float32)          # any layout or real dtype; a tensor that requires grad is detached
        assert t.shape[-1] == self._channels, \
            "Innermost dimension of inputs = %d, does not match number of channels = %d" % (t.shape[-1], self._channels)
        return t

    def _ret(self, t, like):
        return t if isinstance(like, torch.Tensor) else t.cpu().numpy()

    def cdf(self, inputs, stop_gradient=None):
        return self._ret(ops.bmshj_cdf_pdf(self._params(), self._x(inputs), cdf=True, pdf=False)[0], inputs)

    def pdf(self, inputs, stop_gradient=False):
        return self._ret(ops.bmshj_cdf_pdf(self._params(), self._x(inputs), cdf=False, pdf=True)[1], inputs)

    def logpdf(self, inputs, stop_gradient=False):
        return self._ret(ops.bmshj_cdf_pdf(self._params(), self._x(inputs), cdf=False, pdf=False, logpdf=True)[2], inputs)

    def cdf_pdf(self, inputs, stop_gradient=False):
        c, p, _ = ops.bmshj_cdf_pdf(self._params(), self._x(inputs), cdf=True, pdf=True)
        return self._ret(c, inputs), self._ret(p, inputs)

    # ---- fit (learned_prior.py:363-465) -------------------------------------------------------
    def loss_and_grads(self, x_cb: torch.Tensor):
        """-mean(log(pdf + 1e-10)) over all elements (learned_prior.py:405-408) and its gradient with
        respect to the RAW variables, in get_weights() order.  x_cb: f32 device planes [C, n]."""
        Cc, n = x_cb.shape
        out = ops.bmshj_nll_grad(self._params(), x_cb).cpu().numpy()            # [C, 44] f64
        scale = 1.0 / (float(n) * Cc)
        loss = float(out[:, 43].sum() * scale)
        g = out[:, :43] * scale
        grads, o = [], 0
        for i in range(4):
            m = self.matrices[i]
            k = m[0].size
            gm = g[:, o:o + k].reshape(m.shape); o += k
            sig = 1.0 / (1.0 + np.exp(-m.astype(np.float64)))                    # d softplus / d raw
            grads.append((gm * sig).astype(np.float32))
            b = self.biases[i]
            k = b[0].size
            grads.append(g[:, o:o + k].reshape(b.shape).astype(np.float32)); o += k
            if i < 3:
                f = self.factors[i]
                k = f[0].size
                gf = g[:, o:o + k].reshape(f.shape); o += k
                grads.append((gf * (1.0 - np.tanh(f.astype(np.float64)) ** 2)).astype(np.float32))   # d tanh / d raw
        return loss, grads

    def fit(self, data, lr=0.01, its=500, tol=1e-3, logging_freq=10, verbose=False, early_stop=False):
        """Full-batch Adam on the negative log-likelihood, as learned_prior.train
        (learned_prior.py:363-465; post_process.py:73-81 calls it with --lr 0.1 --its 400 --tol 1e-2).
        `data` is [n, C] (the validation latent means).  Returns the record list [{it, loss}, ...].

        The reference tests |prev_loss - loss| / |loss| < tol after every step (:427) but never
        assigns prev_loss (it stays inf, :421), so its loop always runs all `its` iterations.
        That behaviour is the default here; early_stop=True applies the evidently intended rule."""
        x = ops.upload(data, _device(), torch.float32).reshape(-1, self._channels).contiguous()
        x_cb = ops.transpose(x)
        beta1, beta2, eps = 0.9, 0.999, 1e-8                                     # tf.train.AdamOptimizer defaults
        weights = [w.copy() for w in self.get_weights()]
        m = [np.zeros_like(w) for w in weights]
        v = [np.zeros_like(w) for w in weights]
        record = []
        prev_loss = float("inf")
        _, grads = self.loss_and_grads(x_cb)
        for it in range(its):
            t = it + 1
            lr_t = lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
            for k in range(len(weights)):
                m[k] = (beta1 * m[k] + (1.0 - beta1) * grads[k]).astype(np.float32)
                v[k] = (beta2 * v[k] + (1.0 - beta2) * grads[k] * grads[k]).astype(np.float32)
                weights[k] = (weights[k] - lr_t * m[k] / (np.sqrt(v[k]) + eps)).astype(np.float32)
            self.set_weights(weights)
            loss_, grads = self.loss_and_grads(x_cb)                             # loss after the step (:423)
            if early_stop:
                if abs(prev_loss - loss_) / abs(loss_) < tol:
                    break
                prev_loss = loss_
            if it % logging_freq == 0 or it + 1 == its:
                record.append(dict(it=it, loss=loss_))
                if verbose:
                    print("it=%d,\t\tloss=%g" % (it, loss_))
        self.last_loss = loss_
        return record

    def inverse_cdf(self, xi, method="bisection", max_iterations=1000, tol=1e-9, **kwargs):
        """learned_prior.py:173-218: global bracket doubling, masked bisection, the reference's
        stopping rule (all mid values exactly 0, or the smallest bracket <= tol)."""
        if method != "bisection":
            raise NotImplementedError
        # The bracket doubling below never ends for an xi outside (0, 1) (or NaN) after the float32 cast: check on the host,
        # before anything goes to the device.
        xi32 = xi.detach().to(torch.float32) if isinstance(xi, torch.Tensor) else \
            ops.host_tensor(np.asarray(xi, dtype=np.float32))
        if not bool(torch.all((xi32 > 0) & (xi32 < 1))):
            raise ValueError("inverse_cdf: every xi must be finite and lie in (0, 1) as a float32")
        xi_t = self._x(xi)
        params = self._params()

        def f(z):
            return ops.bmshj_cdf_pdf(params, z, cdf=True, pdf=False)[0] - xi_t

        def bracket(z, side):
            # double until every f(z) has the sign `side`; a channel whose CDF never crosses its xi (e.g. zero matrices
            # after a float32 softplus) would take z to -inf / +inf and then spin there
            while True:
                miss = ~(f(z) * side > 0)
                if not bool(miss.any()):
                    return z
                z = z * 2
                if not bool(torch.isfinite(z).all()):
                    c = int(torch.nonzero(miss.reshape(-1))[0]) % self._channels
                    raise ValueError(f"inverse_cdf: the CDF of channel {c} does not cross its xi on "
                                     f"[-3.4e38, 3.4e38]: no bracket")
        left = bracket(torch.full_like(xi_t, -1.0), -1)
        right = bracket(torch.full_like(xi_t, 1.0), 1)
        mid = torch.empty_like(xi_t)
        # The bisection steps are enqueued in chains of 48 with the stopping rule (:210-211) applied on the device between them
        # (vbq_bmshj_icdf_chain_f32): ONE host read per chain instead of one per step -- the loop was 40 synchronisations long.
        chain = 48
        flags = torch.empty((chain + 1, 2), dtype=torch.int32, device=xi_t.device)
        self.last_iterations = 0
        done, ran = False, 0
        while not done and ran < max_iterations:
            n = min(chain, max_iterations - ran)
            ops.bmshj_icdf_chain(params, xi_t, left, right, mid, flags[: n + 1], n, float(np.float32(tol)), first=(ran == 0))
            f = flags[: n + 1].cpu().numpy().view(np.uint32)
            widths = f[:, 1].copy().view(np.float32)
            for j in range(1, n + 1):                             # pair j: what step j - 1 of this chain accumulated
                if f[j, 0] == 0 or widths[j] <= np.float32(tol):
                    self.last_iterations = ran + j - 1
                    done = True
                    break
            else:
                self.last_iterations = ran + n - 1
                flags[0].copy_(flags[n])                         # the next chain continues from the last step's pair
            ran += n
        if kwargs.get("return_np", False) or not isinstance(xi, torch.Tensor):
            return mid.cpu().numpy()
        return mid
