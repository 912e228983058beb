"""Batches of compact latent files (magic b"VBQc") against the loop of one-file calls, at C = 256, N = 10.

  F Kodak-shaped latents [1, 32, 48, 256] (F = 1, 24, 256; 24 distinct tensors, repeated for F = 256) at four lambdas mixed
  from file to file, in parts of 1 << 17 and 1 << 15 symbols:

    write       a loop of compress_latents_to_bytes(..., layout="interleaved") against ONE compress_latents_to_compact_batch,
                from NumPy latents and (dev_in) from device tensors;
    read        a loop of decompress_latents(return_np=False) against ONE decompress_latents_compact_batch, from bytes;
    segments    beside them the batch calls for files in segments (compress_latents_to_bytes_batch / decompress_latents_batch
                at --segment) on the same latents.

  The batch results are asserted equal to the loop's -- byte for byte, bit for bit -- before anything is timed.

One clock: the host clock around a call, bytes or latents in and files or device tensors out, ending in a device-to-host copy
or a synchronise.  Per repetition the calls of a case run one after the other (loop, batch, loop, ...), so that a drift of the
machine hits all alike; --reps repetitions after 3 warm-up rounds; the median and the spread [min, max] are reported, in ms.
One JSON line per case."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import LAMBDAS, make_inputs


def timed(fns, reps, warmup=3):
    """{name: (median, min, max) ms} of the calls of `fns`, alternated within every repetition."""
    t = {k: [] for k in fns}
    for r in range(warmup + reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warmup:
                t[k].append((time.perf_counter() - t0) * 1e3)
    return {k: [round(sorted(v)[len(v) // 2], 3), round(min(v), 3), round(max(v), 3)] for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--lambda-indices", type=int, nargs=4, default=[17, 5, 11, 25])
    ap.add_argument("--files", type=int, nargs="*", default=[1, 24, 256])
    ap.add_argument("--parts", type=int, nargs="*", default=[1 << 17, 1 << 15])
    ap.add_argument("--segment", type=int, default=1024)
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("compact_batch_bench needs a ROCm device")
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    C, distinct, seg = 256, 24, args.segment
    mu, sg = make_inputs(distinct * 32 * 48, C, 0)
    lv = (2 * np.log(sg)).astype(np.float32)
    q = ChannelwisePriorCDFQuantizer(C, 10)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C), mu.std(axis=0).astype(np.float64)))
    q.build_entropy_models_from_latents(mu, lv, LAMBDAS, add_n_smoothing=1, spread="logvar")
    four = [LAMBDAS[i] for i in args.lambda_indices]
    m, v = mu.reshape(distinct, 1, 32, 48, C), lv.reshape(distinct, 1, 32, 48, C)
    dev = [(torch.from_numpy(m[i]).to(q.device), torch.from_numpy(v[i]).to(q.device)) for i in range(distinct)]
    res = []
    for F in args.files:
        lat = [(m[i % distinct], v[i % distinct]) for i in range(F)]
        on_dev = [dev[i % distinct] for i in range(F)]
        lambs = [four[(i * 7 + i // 4) % 4] for i in range(F)]
        seg_files = q.compress_latents_to_bytes_batch(lat, lambs, segment=seg)
        for part in args.parts:
            write_loop = lambda src: [q.compress_latents_to_bytes(a, b, l, layout="interleaved", part=part)            # noqa: E731
                                      for (a, b), l in zip(src, lambs)]
            files = write_loop(lat)
            assert q.compress_latents_to_compact_batch(lat, lambs, part=part) == files, "the batch differs from the loop"
            assert q.compress_latents_to_compact_batch(on_dev, lambs, part=part) == files, "the batch of device tensors differs"
            want = [q.decompress_latents(d, return_np=False) for d in files]
            got = q.decompress_latents_compact_batch(files)
            assert all(torch.equal(g.view(torch.int32), w.view(torch.int32)) for g, w in zip(got, want)), "the reader differs"
            del want, got
            t = timed({
                "write_loop": lambda: write_loop(lat),
                "write_batch": lambda: q.compress_latents_to_compact_batch(lat, lambs, part=part),
                "write_loop_dev_in": lambda: write_loop(on_dev),
                "write_batch_dev_in": lambda: q.compress_latents_to_compact_batch(on_dev, lambs, part=part),
                "write_segments_batch": lambda: q.compress_latents_to_bytes_batch(lat, lambs, segment=seg),
                "read_loop": lambda: [q.decompress_latents(d, return_np=False) for d in files],
                "read_batch": lambda: q.decompress_latents_compact_batch(files),
                "read_segments_batch": lambda: q.decompress_latents_batch(seg_files),
            }, args.reps)
            r = dict(F=F, part=part, parts_per_file=-(-32 * 48 * C // part), segment=seg, shape=[1, 32, 48, C],
                     compact_bytes=sum(len(d) for d in files), segments_bytes=sum(len(d) for d in seg_files), ms=t,
                     write_speedup=round(t["write_loop"][0] / t["write_batch"][0], 2),
                     write_dev_in_speedup=round(t["write_loop_dev_in"][0] / t["write_batch_dev_in"][0], 2),
                     read_speedup=round(t["read_loop"][0] / t["read_batch"][0], 2))
            print(json.dumps(r), flush=True)
            res.append(r)
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
