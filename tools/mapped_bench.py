"""Timings of the lambda-map file (vbq_rans_map.hip, ChannelwisePriorCDFQuantizer.compress_latents_to_bytes_mapped) on one
Kodak-sized latent [32, 48, 256] and on [24, 32, 48, 256], N = 10, Gaussian prior, segment 1024, for palettes of P = 1, 2 and 4
lambdas.  Per (shape, P), in one process:

    encode_ms        compress_latents_to_bytes_mapped: the solve of the P lambdas, the mapped encoder, pack, two copies, the file
    decode_ms        decompress_latents(file, return_np=False): parse, upload, unpack, the mapped decoder, the gather
    nbytes_ms        coded_nbytes_mapped: the solve and the sizes kernel alone
    base_encode_ms   compress_latents_to_bytes at ONE lambda (the palette's first), the file that existed before
    base_decode_ms   decompress_latents of that file

The map is made of 4 x 4 blocks of latent positions with a random class each (a map follows objects, so its classes come in
patches), except `map=checker`, which changes class at every position: the worst case for the encoder's 8-symbol steps.  With
P = 1 the two files hold the same payload; P > 1 solves P lambdas where the base solves one, which is most of the difference.
Every timed call is followed by a device synchronise; median of --reps after two warm-up calls.  `bytes` / `base_bytes` are
the file lengths.  Prints one JSON line per (shape, P, map)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.records_bench import _median_ms

LAMBS = [2.0 ** -6, 2.0 ** -2, 2.0, 16.0]


def block_map(rng, lead, P, block=4):
    """Classes shaped `lead` (the latent shape without channels): one random class per block x block patch of the last two axes."""
    h, w = lead[-2], lead[-1]
    coarse = rng.integers(0, P, lead[:-2] + ((h + block - 1) // block, (w + block - 1) // block))
    return np.repeat(np.repeat(coarse, block, axis=-2), block, axis=-1)[..., :h, :w]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="32x48x256,24x32x48x256")
    ap.add_argument("--segment", type=int, default=1024)
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mapped_bench needs a ROCm device")
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    N, seg = 10, args.segment
    res = []
    for spec in args.shapes.split(","):
        shape = tuple(int(x) for x in spec.split("x"))
        C = shape[-1]
        rng = np.random.default_rng(C + len(shape))
        scale = np.exp(rng.uniform(np.log(0.3), np.log(3.0), C))
        q = ChannelwisePriorCDFQuantizer(C, N)
        q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C), scale))
        m = torch.from_numpy((scale * rng.standard_normal(shape)).astype(np.float32)).cuda()
        lv = torch.from_numpy((2 * (-2 + 0.7 * rng.standard_normal(shape))).astype(np.float32)).cuda()
        q.build_entropy_models_from_latents(m.reshape(-1, C), lv.reshape(-1, C), LAMBS, add_n_smoothing=1, spread="logvar")
        base = q.compress_latents_to_bytes(m, lv, LAMBS[0], segment=seg)
        base_enc = _median_ms(lambda: q.compress_latents_to_bytes(m, lv, LAMBS[0], segment=seg), args.reps)
        base_dec = _median_ms(lambda: q.decompress_latents(base, return_np=False), args.reps)
        for P, kind in ((1, "blocks"), (2, "blocks"), (4, "blocks"), (4, "checker")):
            lambs = LAMBS[:P]
            cls = block_map(rng, shape[:-1], P) if kind == "blocks" else (np.arange(int(np.prod(shape[:-1]))) % P).reshape(shape[:-1])
            data = q.compress_latents_to_bytes_mapped(m, lv, lambs, cls, segment=seg)
            want = q.compress_latents_mapped(m, lv, lambs, cls, return_np=False)["Z_hat"]
            r = dict(shape=list(shape), P=P, map=kind, segment=seg, bytes=len(data), base_bytes=len(base),
                     round_trip=bool(torch.equal(q.decompress_latents(data, return_np=False), want)),
                     nbytes_exact=q.coded_nbytes_mapped(m, lv, lambs, cls, segment=seg) == len(data),
                     encode_ms=_median_ms(lambda: q.compress_latents_to_bytes_mapped(m, lv, lambs, cls, segment=seg), args.reps),
                     decode_ms=_median_ms(lambda: q.decompress_latents(data, return_np=False), args.reps),
                     nbytes_ms=_median_ms(lambda: q.coded_nbytes_mapped(m, lv, lambs, cls, segment=seg), args.reps),
                     base_encode_ms=base_enc, base_decode_ms=base_dec)
            print(json.dumps(r), flush=True)
            res.append(r)
        del q, m, lv
        torch.cuda.empty_cache()
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
