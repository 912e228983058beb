"""Wall time of ChannelwisePriorCDFQuantizer.compress_latents_to_bytes / decompress_latents (one lambda) on a Kodak-shaped
latent [1, 32, 48, 256] and the Kodak-24 tensor [24, 32, 48, 256].  Host clock around calls that end in a device
synchronise (both methods return host data, so every call synchronises).  Run once plainly for the times and once under
`rocprofv3 --kernel-trace --stats` for the kernel times of pack / unpack against the rANS encode / decode kernels."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import LAMBDAS, make_inputs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lambda-index", type=int, default=17)
    ap.add_argument("--segment", type=int, default=1024)
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bitstream_bench needs a ROCm device")
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    C = 256
    mu, sg = make_inputs(24 * 32 * 48, C, 0)
    lv = (2 * np.log(sg)).astype(np.float32)
    q = ChannelwisePriorCDFQuantizer(C, 10)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C), mu.std(axis=0).astype(np.float64)))
    q.build_entropy_models_from_latents(mu, lv, LAMBDAS, add_n_smoothing=1, spread="logvar")
    lamb = LAMBDAS[args.lambda_index]
    res = []
    for B in (1, 24):
        shape = (B, 32, 48, C)
        m = torch.from_numpy(mu[: B * 32 * 48].reshape(shape)).cuda()
        v = torch.from_numpy(lv[: B * 32 * 48].reshape(shape)).cuda()
        data = q.compress_latents_to_bytes(m, v, lamb, segment=args.segment)
        want = np.asarray(q.compress_latents(m, v, [lamb])["Z_hat"][lamb])
        assert np.array_equal(q.decompress_latents(data), want), "round trip differs from compress_latents"
        for _ in range(3):
            q.compress_latents_to_bytes(m, v, lamb, segment=args.segment)
            q.decompress_latents(data, return_np=False)
        torch.cuda.synchronize()
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            q.compress_latents_to_bytes(m, v, lamb, segment=args.segment)
            t.append(time.perf_counter() - t0)
        enc = sorted(t)[len(t) // 2] * 1e3
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            q.decompress_latents(data, return_np=False)
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        dec = sorted(t)[len(t) // 2] * 1e3
        r = dict(shape=list(shape), lamb=lamb, segment=args.segment, bytes=len(data),
                 bits_per_latent=8 * len(data) / m.numel(), compress_ms=round(enc, 3), decompress_ms=round(dec, 3))
        print(json.dumps(r), flush=True)
        res.append(r)
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
