"""Device-event timings of rate control at the sizes users run: the exact file length of every rate (coded_nbytes) and the file
of a byte budget (compress_latents_to_budget / embeddings.compress_to_budget) against the loop that builds every candidate file
(compress_latents_to_bytes over 16 lambdas, embeddings.compress_to_bytes over the notebook's 50 betas), and k_rans_sizes next
to k_rans_encode on the same index streams (RansCodec.sizes / .encode).  Every timed call ends in a device synchronise (it
reads a result back, or is wrapped in one), so the events bracket the whole call.  Before timing, each workload checks that
coded_nbytes equals the lengths of the files it stands for.  Prints one JSON line per workload.

Run it once plainly for the times and once under `rocprofv3 --kernel-trace --stats -d <dir> -- python tools/budget_bench.py
--reps 3` for the kernel times (k_rans_sizes / k_rans_encode and the solve kernels)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import BETAS_50, LAMBDAS_16, make_inputs


def _median_ms(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return round(sorted(t)[len(t) // 2], 4)


def _synced(fn):
    def run():
        fn()
        torch.cuda.synchronize()
    return run


def images(reps, out):
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    C = 256
    mu, sg = make_inputs(24 * 32 * 48, C, 0)
    lv = (2 * np.log(sg)).astype(np.float32)
    q = ChannelwisePriorCDFQuantizer(C, 10)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C), mu.std(axis=0).astype(np.float64)))
    q.build_entropy_models_from_latents(mu, lv, LAMBDAS_16, add_n_smoothing=1, spread="logvar")
    lambs = q.lambs
    for B in (1, 24):
        shape = (B, 32, 48, C)
        m = torch.from_numpy(mu[: B * 32 * 48].reshape(shape)).cuda()
        v = torch.from_numpy(lv[: B * 32 * 48].reshape(shape)).cuda()
        sizes = q.coded_nbytes(m, v)
        assert list(sizes.values()) == [len(q.compress_latents_to_bytes(m, v, l)) for l in lambs], "coded_nbytes != files"
        budget = sorted(sizes.values())[len(sizes) // 2]
        idx = q._file_indices(m, v, lambs)                                       # [16, C, B]: the streams coded_nbytes sizes
        codec = q._coder_stack(lambs, 1024)
        r = dict(workload="images", shape=list(shape), lambdas=len(lambs), segment=1024, budget_bytes=budget,
                 sizes_bytes=[min(sizes.values()), max(sizes.values())],
                 coded_nbytes_ms=_median_ms(lambda: q.coded_nbytes(m, v), reps),
                 budget_ms=_median_ms(lambda: q.compress_latents_to_budget(m, v, budget), reps),
                 loop_of_16_files_ms=_median_ms(lambda: [q.compress_latents_to_bytes(m, v, l) for l in lambs], reps),
                 one_file_ms=_median_ms(lambda: q.compress_latents_to_bytes(m, v, lambs[8]), reps),
                 solve_16_ms=_median_ms(_synced(lambda: q._file_indices(m, v, lambs)), reps),
                 rans_sizes_call_ms=_median_ms(_synced(lambda: codec.sizes(idx)), reps),
                 rans_encode_call_ms=_median_ms(_synced(lambda: codec.encode(idx)), reps))
        print(json.dumps(r), flush=True)
        out.append(r)
        del idx, m, v
        torch.cuda.empty_cache()


def embeddings(reps, out):
    from vbq_amd import coder, embeddings as E, ops
    V, D = 100_000, 100
    cp, _ = E.make_code_book(1.0)
    g = torch.Generator(device="cuda").manual_seed(V + D)
    means = torch.randn((V, D), generator=g, device="cuda")
    stds = torch.rand((V, D), generator=g, device="cuda") * 0.5 + 0.05
    seg = E.default_segment(D)
    sizes = E.coded_nbytes(means, stds, BETAS_50, cp)
    assert sizes.tolist() == [len(E.compress_to_bytes(means, stds, b, cp)) for b in BETAS_50], "coded_nbytes != files"
    budget = int(np.median(sizes))
    idx, _ = E.compress_coordinates_sweep(means, stds, BETAS_50, cp, want_values=False)
    idx = idx.reshape(len(BETAS_50), -1)
    counts = ops.histogram(idx, 1, N=10).cpu().numpy().reshape(len(BETAS_50), -1)
    t0 = time.perf_counter()
    for _ in range(reps):
        freq = np.stack([coder.exact_frequencies(c) for c in counts])
    fit_ms = (time.perf_counter() - t0) * 1e3 / reps
    codec = coder.RansCodec(freq, N=10, segment=seg, allow_zero=True)
    r = dict(workload="embeddings", shape=[V, D], betas=len(BETAS_50), segment=seg, budget_bytes=budget,
             sizes_bytes=[int(sizes.min()), int(sizes.max())],
             coded_nbytes_ms=_median_ms(lambda: E.coded_nbytes(means, stds, BETAS_50, cp), reps),
             budget_ms=_median_ms(lambda: E.compress_to_budget(means, stds, cp, budget), reps),
             loop_of_50_files_ms=_median_ms(lambda: [E.compress_to_bytes(means, stds, b, cp) for b in BETAS_50], reps),
             one_file_ms=_median_ms(lambda: E.compress_to_bytes(means, stds, BETAS_50[25], cp), reps),
             sweep_50_ms=_median_ms(_synced(lambda: E.compress_coordinates_sweep(means, stds, BETAS_50, cp, want_values=False)),
                                    reps),
             table_fit_50_host_ms=round(fit_ms, 3),
             rans_sizes_call_ms=_median_ms(_synced(lambda: codec.sizes(idx)), reps),
             rans_encode_call_ms=_median_ms(_synced(lambda: codec.encode(idx)), reps))
    print(json.dumps(r), flush=True)
    out.append(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=["images", "embeddings"])
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("budget_bench needs a ROCm device")
    res = []
    if args.only in (None, "images"):
        images(args.reps, res)
    if args.only in (None, "embeddings"):
        embeddings(args.reps, res)
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
