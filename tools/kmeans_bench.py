"""Host-clock timings of the exact k-means baseline (ChannelwiseOptimalKmeansWrapper: one dynamic programme over all channels
and all level counts, one nearest-code launch per level count) against the path it stands beside:
ChannelwiseSimpleQuantizerWrapper(KmeansQuantizer, ...) -- one sklearn KMeans fit and one nearest-code launch per (level count,
channel).  The comparison runs at a reduced shape (default C = 32, 36 864 rows, the reference's nine level counts) so that the
sklearn side stays reasonable; the new path alone is also timed at full width (C = 256).  Next to the times: the ratio of summed
within-cluster sums of squares, sklearn to optimal, per level count (>= 1: the DP is the global optimum), from the code
points each side fitted and nearest assignment in float64.  Every call ends in a device synchronise; fit times are one run
(sklearn's is minutes), the others the median of --reps.  Without sklearn the new path is reported alone, and says so.  One JSON
line per measurement."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

LEVELS = [2, 4, 6, 8, 16, 32, 64, 128, 256]              # post_process.py:147-150


class Latents:
    """A stand-in VAE: the 'images' are the latents."""

    def encode(self, X):
        return X, None

    def decode(self, Z):
        return Z


def _timed(fn, reps=1):
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        t.append(1e3 * (time.perf_counter() - t0))
    return round(sorted(t)[len(t) // 2], 3), out


def _sse(x, codes):
    """Summed over channels: nearest assignment of x [B, C] (f64) to codes [C, k]."""
    return float(sum((np.abs(x[:, c, None] - np.sort(codes[c])[None, :]).min(axis=1) ** 2).sum() for c in range(x.shape[1])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=36864)
    ap.add_argument("--channels", type=int, default=32)
    ap.add_argument("--full-channels", type=int, default=256)
    ap.add_argument("--levels", type=int, nargs="+", default=LEVELS)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-sklearn", action="store_true", help="skip the sklearn path even where it is importable")
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_bench needs a ROCm device")
    import vbq_amd
    from vbq_amd import baselines, kmeans1d
    B, Cn, levels = args.rows, args.channels, list(args.levels)
    rng = np.random.default_rng(B + Cn)
    scale = np.exp(rng.uniform(np.log(0.3), np.log(3.0), args.full_channels))
    full = (scale * rng.standard_normal((B, args.full_channels))).astype(np.float32)
    x = np.ascontiguousarray(full[:, :Cn])
    vae, res = Latents(), []

    def report(**r):
        print(json.dumps(r), flush=True)
        res.append(r)

    try:
        import sklearn
        have = not args.no_sklearn
        note = f"sklearn {sklearn.__version__}" if have else "sklearn skipped on request"
    except ImportError:
        have, note = False, "sklearn is not importable here: the new path is reported alone"

    new = vbq_amd.ChannelwiseOptimalKmeansWrapper(Cn, levels)
    new.fit(x[:max(levels) + 256], vae, 1.0)                                   # warm: allocator, library load
    fit_ms, _ = _timed(lambda: new.fit(x, vae, 1.0), args.reps)
    compress_ms, out = _timed(lambda: new.compress(x, vae, levels, clip=False), args.reps)
    dp_ms, _ = _timed(lambda: kmeans1d.sse_curve(x, max(levels)), args.reps)
    x64 = x.astype(np.float64)
    report(what="optimal", shape=[B, Cn], levels=levels, fit_ms=fit_ms, compress_ms=compress_ms, sums_and_dp_alone_ms=dp_ms, note=note)
    if have:
        old = baselines.ChannelwiseSimpleQuantizerWrapper(baselines.KmeansQuantizer, Cn, levels)
        old_fit_ms, _ = _timed(lambda: old.fit(x, vae, 1.0))
        old_compress_ms, _ = _timed(lambda: old.compress(x, vae, levels, clip=False), args.reps)
        ratio = {l: round(_sse(x64, q.code_points) / _sse(x64, new.code_points[l]), 6) for l, q in zip(levels, old._quantizers)}
        report(what="sklearn", shape=[B, Cn], levels=levels, fit_ms=old_fit_ms, compress_ms=old_compress_ms,
               fit_over_optimal=round(old_fit_ms / fit_ms, 1), compress_over_optimal=round(old_compress_ms / compress_ms, 1),
               sse_sklearn_over_optimal=ratio)
    wide = vbq_amd.ChannelwiseOptimalKmeansWrapper(args.full_channels, levels)
    wide_fit_ms, _ = _timed(lambda: wide.fit(full, vae, 1.0))
    wide_compress_ms, _ = _timed(lambda: wide.compress(full, vae, levels, clip=False))
    report(what="optimal_full_width", shape=[B, args.full_channels], levels=levels, fit_ms=wide_fit_ms, compress_ms=wide_compress_ms)
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
