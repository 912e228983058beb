"""Batch compression of lambda-map files against the one-file path, at C = 256, N = 10, segment 1024.

  F Kodak-shaped latents [1, 32, 48, 256] (F = 1, 24, 256; 24 distinct tensors, repeated for F = 256) with palettes of P = 2 and
  P = 4 lambdas, a smooth class map (P bands of rows) and a checkerboard (a change at every position), once with one palette for
  all files and once with four palettes mixed from file to file: a loop of compress_latents_to_bytes_mapped (the path the batch
  does not touch) against ONE compress_latents_to_bytes_mapped_batch, alternated in one process.  The two results are asserted
  equal byte for byte before anything is timed.

The clocks are those of tools/encode_batch_bench.py.  wall: the host clock around a call, NumPy latents in and bytes out, median
of --reps calls after 3 warm-up calls.  wall_dev_in: the same clock with the latents given as device tensors.  dev: device events
around the launches alone, on inputs uploaded beforehand and with nothing read back (the loop: planes, solve, encode and pack per
file; the batch: planes and solve per distinct palette, one encode, one pack), median of --reps.  One JSON line per case."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from bench import LAMBDAS, make_inputs
from encode_batch_bench import device_ms, wall_ms


def one_file_launches(q, means, logvars, palette, cls, segment):
    """The launches of compress_latents_to_bytes_mapped on latents and classes uploaded once: planes, solve of the palette,
    (canonical gather), encode, pack."""
    C = q.num_channels
    keys = [q._lambda_key(l) for l in palette]
    codec, _ = q._mapped_codec(keys, segment)
    m, lv = q._f32_dev(means).reshape(-1, C), q._f32_dev(logvars).reshape(-1, C)
    n = m.shape[0]
    sel = (len(keys), codec._classes(cls.reshape(-1), n, q.device, check=True))
    S, nseg = C, codec._nseg(n)
    words = torch.empty((S, nseg, segment + 2), dtype=torch.uint16, device=q.device)
    sizes = torch.empty((S, nseg), dtype=torch.uint32, device=q.device)
    payload = torch.empty(S * nseg * (segment + 2), dtype=torch.uint16, device=q.device)
    offsets = torch.empty((S, nseg), dtype=torch.int64, device=q.device)
    total = torch.empty(1, dtype=torch.uint64, device=q.device)

    def launch():
        idx = q._file_indices(m, lv, keys)
        codec._encode(idx, sel, n, words, sizes)
        codec._pack(words, sizes, payload, offsets, total)
    return launch


def batch_launches(q, latents, palettes, classes, segment):
    """The launches of compress_latents_to_bytes_mapped_batch on a staging buffer uploaded once."""
    mb = q._mapped_batch_plan(latents, palettes, classes, segment)
    d_host, lat = q._encode_batch_upload(mb.b)
    return lambda: q._mapped_batch_run(mb, d_host, lat, words=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lambda-indices", type=int, nargs=4, default=[17, 5, 11, 25], help="the lambdas the palettes are made of")
    ap.add_argument("--files", type=int, nargs="*", default=[1, 24, 256])
    ap.add_argument("--segment", type=int, default=1024)
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mapped_batch_bench needs a ROCm device")
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    C, distinct, seg = 256, 24, args.segment
    mu, sg = make_inputs(distinct * 32 * 48, C, 0)
    lv = (2 * np.log(sg)).astype(np.float32)
    q = ChannelwisePriorCDFQuantizer(C, 10)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C), mu.std(axis=0).astype(np.float64)))
    q.build_entropy_models_from_latents(mu, lv, LAMBDAS, add_n_smoothing=1, spread="logvar")
    a, b, c, d = (LAMBDAS[i] for i in args.lambda_indices)
    four = {2: [(a, b), (b, a), (c, d), (a, d)], 4: [(a, b, c, d), (d, c, b, a), (b, a, d, c), (c, a, d, b)]}
    m, v = mu.reshape(distinct, 1, 32, 48, C), lv.reshape(distinct, 1, 32, 48, C)
    i0, i1 = np.arange(32)[None, :, None], np.arange(48)[None, None, :]
    res = []
    for F in args.files:
        latents = [(m[i % distinct], v[i % distinct]) for i in range(F)]
        on_dev = [(torch.from_numpy(x).to(q.device), torch.from_numpy(y).to(q.device)) for x, y in latents[:distinct]]
        on_dev = [on_dev[i % distinct] for i in range(F)]
        for P in (2, 4):
            maps = {"smooth": np.broadcast_to(i0 * P // 32, (1, 32, 48)).astype(np.uint8),
                    "checkerboard": ((i0 + i1) % P).astype(np.uint8)}
            for map_name, cls in maps.items():
                classes = [cls] * F
                for name, pals in (("one-palette", [four[P][0]] * F), ("four-palettes", [four[P][(i * 7 + i // 4) % 4] for i in range(F)])):
                    def loop(lat=latents):
                        return [q.compress_latents_to_bytes_mapped(x, y, list(p), cls, segment=seg) for (x, y), p in zip(lat, pals)]

                    def batch(lat=latents):
                        return q.compress_latents_to_bytes_mapped_batch(lat, pals, classes, segment=seg)
                    want, got = loop(), batch()
                    assert len(got) == F and all(g == w for g, w in zip(got, want)), "the batch differs from the loop"
                    assert batch(on_dev) == want, "the batch of device tensors differs from the loop"
                    one = [one_file_launches(q, x, y, p, cls, seg) for (x, y), p in zip(latents, pals)]
                    r = dict(case=name, map=map_name, P=P, F=F, distinct_palettes=len(set(pals)), shape=[1, 32, 48, C], segment=seg,
                             bytes=sum(len(f) for f in want),
                             loop_wall_ms=wall_ms(loop, args.reps), batch_wall_ms=wall_ms(batch, args.reps),
                             loop_wall_dev_in_ms=wall_ms(lambda: loop(on_dev), args.reps),
                             batch_wall_dev_in_ms=wall_ms(lambda: batch(on_dev), args.reps),
                             loop_dev_ms=device_ms(lambda: [launch() for launch in one], args.reps),
                             batch_dev_ms=device_ms(batch_launches(q, latents, pals, classes, seg), args.reps))
                    print(json.dumps(r), flush=True)
                    res.append(r)
                    del one, want, got
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
