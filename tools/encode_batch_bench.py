"""Batch compression of latent files against the one-file path, at C = 256, N = 10, segment 1024.

  F Kodak-shaped latents [1, 32, 48, 256] (F = 1, 24, 256; 24 distinct tensors, repeated for F = 256), once all at one lambda
  and once at four lambdas mixed from file to file: a loop of compress_latents_to_bytes (the path the batch does not touch)
  against ONE compress_latents_to_bytes_batch, alternated in one process.  The two results are asserted equal byte for byte
  before anything is timed.

Two clocks per case.  wall: the host clock around a call, NumPy latents in and bytes out -- staging, upload, launches, both
device-to-host copies and the assembly of the files included; the call ends in its last device-to-host copy --, median of --reps
calls after 3 warm-up calls.  wall_dev_in: the same clock with the latents given as device tensors (what a VAE encoder on the
device returns): no upload on either side.  dev: device events around the launches alone, on inputs uploaded beforehand and with nothing read
back (the loop: planes, solve, encode and pack per file; the batch: planes and solve per distinct lambda, one encode, one
pack), median of --reps.  One JSON line per case."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import LAMBDAS, make_inputs


def median(t):
    return sorted(t)[len(t) // 2]


def wall_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                                      # (ends in a device-to-host copy: nothing is left in flight)
        t.append(time.perf_counter() - t0)
    return round(median(t) * 1e3, 3)


def device_ms(fn, reps, warmup=3):
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
    return round(median(t), 3)


def one_file_launches(q, means, logvars, lamb, segment):
    """The launches of compress_latents_to_bytes on latents uploaded once: planes, solve, (canonical gather), encode, pack."""
    C = q.num_channels
    key = q._lambda_key(lamb)
    codec, _ = q._coder_tables(key, segment)
    m, lv = q._f32_dev(means).reshape(-1, C), q._f32_dev(logvars).reshape(-1, C)
    S, nseg = C, codec._nseg(m.shape[0])
    words = torch.empty((S, nseg, segment + 2), dtype=torch.uint16, device=q.device)
    sizes = torch.empty((S, nseg), dtype=torch.uint32, device=q.device)
    payload = torch.empty(S * nseg * (segment + 2), dtype=torch.uint16, device=q.device)
    offsets = torch.empty((S, nseg), dtype=torch.int64, device=q.device)
    total = torch.empty(1, dtype=torch.uint64, device=q.device)

    def launch():
        idx = q._file_indices(m, lv, [key])[0]
        codec._encode(idx, None, m.shape[0], words, sizes)
        codec._pack(words, sizes, payload, offsets, total)
    return launch


def batch_launches(q, latents, lambs, segment):
    """The launches of compress_latents_to_bytes_batch on a staging buffer uploaded once."""
    b = q._encode_batch_plan(latents, lambs, segment)
    d_host, lat = q._encode_batch_upload(b)
    return lambda: q._encode_batch_run(b, d_host, lat)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lambda-indices", type=int, nargs=4, default=[17, 5, 11, 25], help="the first is the one lambda of the "
                    "single-lambda cases; all four are mixed from file to file in the others")
    ap.add_argument("--files", type=int, nargs="*", default=[1, 24, 256])
    ap.add_argument("--segment", type=int, default=1024)
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("encode_batch_bench needs a ROCm device")
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    C, distinct, seg = 256, 24, args.segment
    mu, sg = make_inputs(distinct * 32 * 48, C, 0)
    lv = (2 * np.log(sg)).astype(np.float32)
    q = ChannelwisePriorCDFQuantizer(C, 10)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C), mu.std(axis=0).astype(np.float64)))
    q.build_entropy_models_from_latents(mu, lv, LAMBDAS, add_n_smoothing=1, spread="logvar")
    four = [LAMBDAS[i] for i in args.lambda_indices]
    m, v = mu.reshape(distinct, 1, 32, 48, C), lv.reshape(distinct, 1, 32, 48, C)
    res = []
    for F in args.files:
        latents = [(m[i % distinct], v[i % distinct]) for i in range(F)]
        for name, lambs in (("one-lambda", [four[0]] * F), ("four-lambdas", [four[(i * 7 + i // 4) % 4] for i in range(F)])):
            loop = lambda: [q.compress_latents_to_bytes(a, b, l, segment=seg) for (a, b), l in zip(latents, lambs)]   # noqa: E731
            batch = lambda: q.compress_latents_to_bytes_batch(latents, lambs, segment=seg)                             # noqa: E731
            want, got = loop(), batch()
            assert len(got) == F and all(g == w for g, w in zip(got, want)), "the batch differs from the loop"
            on_dev = [(torch.from_numpy(a).to(q.device), torch.from_numpy(b).to(q.device)) for a, b in latents[:distinct]]
            on_dev = [on_dev[i % distinct] for i in range(F)]
            loop_dev_in = lambda: [q.compress_latents_to_bytes(a, b, l, segment=seg) for (a, b), l in zip(on_dev, lambs)]  # noqa: E731
            batch_dev_in = lambda: q.compress_latents_to_bytes_batch(on_dev, lambs, segment=seg)                          # noqa: E731
            assert batch_dev_in() == want, "the batch of device tensors differs from the loop"
            one = [one_file_launches(q, a, b, l, seg) for (a, b), l in zip(latents, lambs)]
            r = dict(case=name, F=F, distinct_lambdas=len(set(lambs)), shape=[1, 32, 48, C], segment=seg,
                     bytes=sum(len(d) for d in want),
                     loop_wall_ms=wall_ms(loop, args.reps), batch_wall_ms=wall_ms(batch, args.reps),
                     loop_wall_dev_in_ms=wall_ms(loop_dev_in, args.reps), batch_wall_dev_in_ms=wall_ms(batch_dev_in, args.reps),
                     loop_dev_ms=device_ms(lambda: [launch() for launch in one], args.reps),
                     batch_dev_ms=device_ms(batch_launches(q, latents, lambs, seg), args.reps))
            print(json.dumps(r), flush=True)
            res.append(r)
            del one, want, got, on_dev
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
