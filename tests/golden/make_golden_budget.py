#!/usr/bin/env python
"""Generate tests/golden/g14_budget_dp.npz by RUNNING THE REFERENCE's own code (img-compression/utils.py, read-only, from the
reference tree) in the build container.  Only data is written: inputs, the per-level score / value tables built from the
reference's own functions, and the reference's outputs.  The reference tree does not exist on the GPU box; this script is never
run there.

What is executed from the reference (utils.py imported as a module behind an identity `numba.jit`, as make_golden.py does):
  * encode_mode_dp (:106-160) with nbits = N           -> dp_mode_hat, dp_obj, dp_num_bits
  * encode_mode (:163-208) at several lambdas            -> em_mode_hat, em_obj, em_num_bits
  * get_all_N_bit_intervals (:215-260) + the endpoint pick of encode_mode_1d (:88-103), to record the tables the DP walks over
  * get_n_bit_interval (:27-57), truncate_float_to_n_bits (:60-78), encode_mode_1d on a few scalars

Cases: K in {1, 2, 5, 8, 20} x N in {1, 3, 8, 12}; f_k(z) = -0.5 * ((z - mu_k) / sigma_k)**2; squash_k / unsquash_k =
norm.cdf / norm.ppf of the prior N(0, prior_scale_k**2); zero_bit_mode_hat = the prior mode 0.
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("VBQ_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "g14_budget_dp.npz")

KS, NS = (1, 2, 5, 8, 20), (1, 3, 8, 12)
EM_LAMBDAS = (0.0, 0.02, 0.3, 1.0, 4.0)
EM_MAX_BITS = 12


def callables(mu, sigma, prior_scale):
    """The per-coordinate scalar functions of one case (tests rebuild exactly these from the stored arrays)."""
    from scipy.stats import norm
    f = [lambda z, m=m, s=s: -0.5 * ((z - m) / s) ** 2 for m, s in zip(mu, sigma)]
    squash = [lambda z, p=p: norm.cdf(z, loc=0.0, scale=p) for p in prior_scale]
    unsquash = [lambda xi, p=p: norm.ppf(xi, loc=0.0, scale=p) for p in prior_scale]
    return f, squash, unsquash


def level_tables(ref_utils, f, mode, N, squash, unsquash, zero_bit_mode_hat):
    K = len(f)
    xi = np.array([squash[k](mode[k]) for k in range(K)], dtype=np.float64)
    left, right = np.empty((N + 1, K)), np.empty((N + 1, K))
    ref_utils.get_all_N_bit_intervals(xi, N, left, right)
    scores, values = np.empty((N + 1, K)), np.empty((N + 1, K))
    for k in range(K):
        values[0, k] = zero_bit_mode_hat[k]
        scores[0, k] = f[k](zero_bit_mode_hat[k])
        for n in range(1, N + 1):
            v = unsquash[k](left[n, k])
            s = f[k](v)
            if right[n, k] != left[n, k]:
                v_r = unsquash[k](right[n, k])
                s_r = f[k](v_r)
                if s_r > s:
                    v, s = v_r, s_r
            values[n, k], scores[n, k] = v, s
    return scores, values


def main():
    assert os.path.isdir(REF), "reference tree not found; this script only runs in the build container"
    nb = types.ModuleType("numba")
    nb.jit = lambda *a, **kw: (lambda fn: fn)
    sys.modules.setdefault("numba", nb)
    sys.path.insert(0, os.path.join(REF, "img-compression"))
    import utils as ref_utils

    out = {"Ks": np.array(KS), "Ns": np.array(NS), "em_lambdas": np.array(EM_LAMBDAS), "em_max_bits": np.array(EM_MAX_BITS)}
    rng = np.random.default_rng(14)
    cases, case_K, case_N = [], [], []
    for K in KS:
        for N in NS:
            prior_scale = np.exp(rng.uniform(np.log(0.5), np.log(2.0), K))
            mu = prior_scale * rng.standard_normal(K)
            sigma = np.exp(-2.5 + 1.2 * rng.standard_normal(K))
            zero = np.zeros(K)
            f, squash, unsquash = callables(mu, sigma, prior_scale)
            c = {"mu": mu, "sigma": sigma, "prior_scale": prior_scale, "zero_bit_mode_hat": zero}
            c["scores"], c["values"] = level_tables(ref_utils, f, mu, N, squash, unsquash, zero)
            mode_hat, obj, num_bits = ref_utils.encode_mode_dp(f, mu, N, squash, unsquash, zero)
            c["dp_mode_hat"], c["dp_obj"], c["dp_num_bits"] = mode_hat, np.float64(obj), np.asarray(num_bits, np.int64)
            c["em_scores"], c["em_values"] = level_tables(ref_utils, f, mu, EM_MAX_BITS, squash, unsquash, zero)
            em = [ref_utils.encode_mode(f, mu, lamb, squash, unsquash, zero, max_bits_per_coord=EM_MAX_BITS) for lamb in EM_LAMBDAS]
            c["em_mode_hat"] = np.stack([e[0] for e in em])
            c["em_obj"] = np.array([e[1] for e in em], dtype=np.float64)
            c["em_num_bits"] = np.stack([np.asarray(e[2], np.int64) for e in em])
            cases.append(c)
            case_K.append(K)
            case_N.append(N)
    # one flat array per field, the cases one after the other (tests/budget_reference.py:g14_cases cuts them apart again)
    out["case_K"], out["case_N"] = np.array(case_K), np.array(case_N)
    for key in cases[0]:
        out[key] = np.concatenate([np.ravel(c[key]) for c in cases])
    # scalar helpers
    xs = np.concatenate([[0.4375, 0.004375, 0.04375, 0.0, 1.0, 0.5, 0.25, 0.75, 1e-9, 1 - 1e-9], rng.uniform(0, 1, 22)])
    ns = np.concatenate([[2, 2, 5, 3, 3, 0, 1, 2, 12, 12], rng.integers(0, 16, 22)])
    out["iv_x"], out["iv_n"] = xs, ns
    out["iv_lr"] = np.array([list(ref_utils.get_n_bit_interval(float(x), int(n))) for x, n in zip(xs, ns)], dtype=np.float64)
    tr = [ref_utils.truncate_float_to_n_bits(float(x), int(n)) for x, n in zip(xs, ns)]
    out["tr_x_hat"], out["tr_bits"] = np.array([t[0] for t in tr]), np.array([t[1] for t in tr])
    f, squash, unsquash = callables([0.3], [0.05], [1.5])
    e1 = [ref_utils.encode_mode_1d(f[0], 0.3, int(n), squash[0], unsquash[0]) for n in range(0, 14)]
    out["e1_mode_hat"], out["e1_f_hat"] = np.array([e[0] for e in e1]), np.array([e[1] for e in e1])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
