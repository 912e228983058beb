"""Lambda-map files to a byte budget: one rates launch over every candidate palette against the loop over candidates, at
C = 256, N = 10, segment 1024.

  F Kodak-shaped latents [1, 32, 48, 256] (F = 1, 24, 256; 24 distinct tensors, repeated for F = 256), a smooth class map (P
  bands of rows) and a checkerboard (a change at every position), and the candidates of bitstream.palette_ladder over the 16
  bench lambdas: neighbouring rungs, P = 2 (15 candidates) and P = 4 (13 candidates).  Every file's budget is its length under
  the middle candidate.

  loop:  what a caller writes without the budget calls -- per candidate one coded_nbytes_mapped_batch (F = 1: one
         coded_nbytes_mapped), the first candidate that fits per file, then ONE compress_latents_to_bytes_mapped_batch.
  call:  ONE compress_latents_to_budget_mapped_batch.
  lengths_*: the length table alone (the loop of sizes calls against ONE coded_nbytes_mapped_palettes_batch).

The length tables are asserted equal, and the files byte for byte, before anything is timed.  The clocks are those of
tools/mapped_batch_bench.py: wall -- the host clock around a call, NumPy latents in and bytes out, median of --reps calls after 3
warm-up calls; wall_dev_in -- the same clock with the latents given as device tensors.  One JSON line per case."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from bench import LAMBDAS_16, make_inputs
from encode_batch_bench import wall_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--files", type=int, nargs="*", default=[1, 24, 256])
    ap.add_argument("--segment", type=int, default=1024)
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mapped_budget_bench needs a ROCm device")
    from vbq_amd import ChannelwisePriorCDFQuantizer, bitstream, priors
    C, distinct, seg = 256, 24, args.segment
    mu, sg = make_inputs(distinct * 32 * 48, C, 0)
    lv = (2 * np.log(sg)).astype(np.float32)
    q = ChannelwisePriorCDFQuantizer(C, 10)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C), mu.std(axis=0).astype(np.float64)))
    q.build_entropy_models_from_latents(mu, lv, LAMBDAS_16, add_n_smoothing=1, spread="logvar")
    m, v = mu.reshape(distinct, 1, 32, 48, C), lv.reshape(distinct, 1, 32, 48, C)
    i0, i1 = np.arange(32)[None, :, None], np.arange(48)[None, None, :]
    res = []
    for F in args.files:
        latents = [(m[i % distinct], v[i % distinct]) for i in range(F)]
        on_dev = [(torch.from_numpy(x).to(q.device), torch.from_numpy(y).to(q.device)) for x, y in latents[:distinct]]
        on_dev = [on_dev[i % distinct] for i in range(F)]
        for P in (2, 4):
            cands = bitstream.palette_ladder(LAMBDAS_16, list(range(P)))
            maps = {"smooth": np.broadcast_to(i0 * P // 32, (1, 32, 48)).astype(np.uint8),
                    "checkerboard": ((i0 + i1) % P).astype(np.uint8)}
            for map_name, cls in maps.items():
                classes = [cls] * F

                def loop_lengths(lat=latents):
                    if F == 1:
                        return np.array([[q.coded_nbytes_mapped(lat[0][0], lat[0][1], list(c), cls, segment=seg) for c in cands]])
                    return np.array([q.coded_nbytes_mapped_batch(lat, list(c), classes, segment=seg) for c in cands]).T

                def call_lengths(lat=latents):
                    return q.coded_nbytes_mapped_palettes_batch(lat, cands, classes, segment=seg)
                table = loop_lengths()
                assert np.array_equal(call_lengths(), table), "the length table differs from the loop over candidates"
                assert np.array_equal(call_lengths(on_dev), table), "the length table of device tensors differs"
                budgets = [int(b) for b in table[:, len(cands) // 2]]

                def loop(lat=latents):
                    cols = bitstream.smallest_rates_within(loop_lengths(lat), budgets, name="palette")
                    return q.compress_latents_to_bytes_mapped_batch(lat, [list(cands[c]) for c in cols], classes, segment=seg)

                def call(lat=latents):
                    return q.compress_latents_to_budget_mapped_batch(lat, budgets, cands, classes, segment=seg)
                want = loop()
                assert call() == want and call(on_dev) == want, "the budget call differs from the loop over candidates"
                r = dict(map=map_name, P=P, F=F, K=len(cands), lambdas=len({l for c in cands for l in c}), shape=[1, 32, 48, C],
                         segment=seg, bytes=sum(len(f) for f in want),
                         loop_wall_ms=wall_ms(loop, args.reps), call_wall_ms=wall_ms(call, args.reps),
                         loop_wall_dev_in_ms=wall_ms(lambda: loop(on_dev), args.reps),
                         call_wall_dev_in_ms=wall_ms(lambda: call(on_dev), args.reps),
                         lengths_loop_wall_dev_in_ms=wall_ms(lambda: loop_lengths(on_dev), args.reps),
                         lengths_call_wall_dev_in_ms=wall_ms(lambda: call_lengths(on_dev), args.reps))
                print(json.dumps(r), flush=True)
                res.append(r)
                del want
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
