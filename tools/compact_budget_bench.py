"""Rate control for a batch of compact latent files against the loop of one-file calls, at C = 256, N = 10, part 1 << 17.

  F Kodak-shaped latents [1, 32, 48, 256] (F = 1, 24, 256; 24 distinct tensors, repeated for F = 256) and the 16 lambdas
  2 ** linspace(-8, 7, 16): ONE coded_nbytes_compact_batch against the loop of coded_nbytes(layout="interleaved"), and ONE
  compress_latents_to_compact_budget_batch against the loop of compress_latents_to_budget(layout="interleaved") -- the loops
  are the one-file paths the batch calls do not touch --, each with the latents given as NumPy arrays and as device tensors,
  alternated in one process.  One more column, `composed_ms`: coded_nbytes_compact_batch followed by
  compress_latents_to_compact_batch at the lambdas it leads to -- the budget call without the re-use of the part sizes, which
  sizes the parts of the chosen lambdas a second time.  The budget of a file is the median of its 16 lengths.  All results are
  asserted equal (dicts, then bytes) before anything is timed.

One clock: device events around a whole call -- staging, upload, launches, the device-to-host copies and the host's share
between them --, median of --reps calls (default 10) after 2 warm-up calls.  One JSON line per case."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import make_inputs
from vbq_amd import bitstream

LAMBS = [float(v) for v in 2.0 ** np.linspace(-8, 7, 16)]


def event_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return round(sorted(t)[len(t) // 2], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--files", type=int, nargs="*", default=[1, 24, 256])
    ap.add_argument("--part", type=int, default=1 << 17)
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("compact_budget_bench needs a ROCm device")
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    C, distinct, part = 256, 24, args.part
    mu, sg = make_inputs(distinct * 32 * 48, C, 0)
    lv = (2 * np.log(sg)).astype(np.float32)
    q = ChannelwisePriorCDFQuantizer(C, 10)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C), mu.std(axis=0).astype(np.float64)))
    q.build_entropy_models_from_latents(mu, lv, LAMBS, add_n_smoothing=1, spread="logvar")
    m, v = mu.reshape(distinct, 1, 32, 48, C), lv.reshape(distinct, 1, 32, 48, C)
    dev = [(torch.from_numpy(m[i]).to(q.device), torch.from_numpy(v[i]).to(q.device)) for i in range(distinct)]
    order = sorted(range(len(LAMBS)), key=lambda j: LAMBS[j])
    res = []
    for F in args.files:
        for name, latents in (("numpy", [(m[i % distinct], v[i % distinct]) for i in range(F)]),
                              ("device", [dev[i % distinct] for i in range(F)])):
            sizes_loop = lambda: [q.coded_nbytes(a, b, LAMBS, layout="interleaved", part=part) for a, b in latents]   # noqa: E731
            sizes_batch = lambda: q.coded_nbytes_compact_batch(latents, LAMBS, part=part)                             # noqa: E731
            table = sizes_loop()
            assert sizes_batch() == table, "the batch's lengths differ from the loop's"
            budgets = [int(np.median(list(t.values()))) for t in table]
            files_loop = lambda: [q.compress_latents_to_budget(a, b, x, LAMBS, layout="interleaved", part=part)       # noqa: E731
                                  for (a, b), x in zip(latents, budgets)]
            files_batch = lambda: q.compress_latents_to_compact_budget_batch(latents, budgets, LAMBS, part=part)      # noqa: E731

            def composed():
                """The budget call as a user composes it from the two public batch calls: the parts are sized twice."""
                nb = np.array([[t[k] for k in LAMBS] for t in q.coded_nbytes_compact_batch(latents, LAMBS, part=part)])
                cols = bitstream.smallest_rates_within(nb[:, order], budgets, rates=[LAMBS[j] for j in order])
                return q.compress_latents_to_compact_batch(latents, [LAMBS[order[c]] for c in cols], part=part)
            want = files_loop()
            assert files_batch() == want, "the batch's files differ from the loop's"
            assert composed() == want, "the composed call's files differ from the loop's"
            r = dict(inputs=name, F=F, lambdas=len(LAMBS), shape=[1, 32, 48, C], part=part, bytes=sum(len(d) for d in want),
                     nbytes_loop_ms=event_ms(sizes_loop, args.reps), nbytes_batch_ms=event_ms(sizes_batch, args.reps),
                     budget_loop_ms=event_ms(files_loop, args.reps), budget_batch_ms=event_ms(files_batch, args.reps),
                     composed_ms=event_ms(composed, args.reps))
            print(json.dumps(r), flush=True)
            res.append(r)
            del want, table
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
