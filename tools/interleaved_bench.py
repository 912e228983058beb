"""Encode / decode time and file length of the two latent file layouts -- segments of 1024 symbols (magic b"VBQb") and the
wave-interleaved parts (magic b"VBQc") -- on one Kodak-shaped latent [1, 32, 48, 256] (256 channels x 1536 latents) and on
the Kodak-24 planes [24, 32, 48, 256] (256 x 36 864), at one lambda.

Timed at the codec, on indices already on the device: encode = RansCodec.encode_packed / encode_interleaved (kernels and the
copies of sizes and payload to the host), decode = decode_packed / decode_interleaved on a payload already on the device
(kernels and the read of the status word).  Host clock around calls that end in a synchronising copy; median of --reps.
The interleaved layout is run at several part sizes: one part per image (C * B) shows what the serial table staging of one
wave costs, the default 1 << 17 and smaller parts what spreading the image over more waves buys and what it adds in bytes.
One JSON line per (tensor, layout, part)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import LAMBDAS, make_inputs


def median_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return round(sorted(t)[len(t) // 2] * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lambda-index", type=int, default=17)
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("interleaved_bench needs a ROCm device")
    from vbq_amd import ChannelwisePriorCDFQuantizer, bitstream, priors
    from vbq_amd.coder import ideal_bits
    C, T = 256, 2047
    mu, sg = make_inputs(24 * 32 * 48, C, 0)
    lv = (2 * np.log(sg)).astype(np.float32)
    q = ChannelwisePriorCDFQuantizer(C, 10)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C), mu.std(axis=0).astype(np.float64)))
    q.build_entropy_models_from_latents(mu, lv, LAMBDAS, add_n_smoothing=1, spread="logvar")
    lamb = LAMBDAS[args.lambda_index]
    key = q._lambda_key(lamb)
    codec, _ = q._coder_tables(key, 1024)
    res = []
    for images in (1, 24):
        shape = (images, 32, 48, C)
        B = images * 32 * 48
        m = torch.from_numpy(mu[:B].reshape(shape)).cuda()
        v = torch.from_numpy(lv[:B].reshape(shape)).cuda()
        idx = q._file_indices(m, v, [key])[0].contiguous()                                  # u16 [C, B]
        want = idx.view(torch.int16)
        counts = np.stack([np.bincount(r, minlength=T) for r in idx.view(torch.int16).cpu().numpy().view(np.uint16)])
        entropy = ideal_bits(counts, codec.freq_host.numpy()) / 8
        base = dict(shape=list(shape), lamb=lamb, cross_entropy_bytes=round(entropy))

        sizes, payload = codec.encode_packed(idx)
        d_pay, d_sz = torch.from_numpy(payload).cuda(), torch.from_numpy(sizes.astype(np.uint16).reshape(-1)).cuda()
        assert torch.equal(codec.decode_packed(d_pay, d_sz, B).view(torch.int16), want)
        nbytes = bitstream.latent_nbytes(shape, C, 1024, payload.size)
        assert nbytes == len(q.compress_latents_to_bytes(m, v, lamb))
        r = dict(base, layout="segments", segment=1024, bytes=nbytes, over_entropy=round(nbytes / entropy - 1, 4),
                 encode_ms=median_ms(lambda: codec.encode_packed(idx), args.reps),
                 decode_ms=median_ms(lambda: codec.decode_packed(d_pay, d_sz, B), args.reps))
        print(json.dumps(r), flush=True)
        res.append(r)

        for part in ([C * B, 1 << 17, 1 << 16, 1 << 14] if images == 1 else [1 << 20, 1 << 17, 1 << 15]):
            sizes, payload = codec.encode_interleaved(idx, part)
            d_pay, d_sz = torch.from_numpy(payload).cuda(), torch.from_numpy(sizes).cuda()
            assert torch.equal(codec.decode_interleaved(d_pay, d_sz, B, part).view(torch.int16), want)
            nbytes = bitstream.compact_nbytes(shape, C, part, payload.size)
            assert nbytes == len(q.compress_latents_to_bytes(m, v, lamb, layout="interleaved", part=part))
            r = dict(base, layout="interleaved", part=part, parts=int(sizes.size), bytes=nbytes,
                     over_entropy=round(nbytes / entropy - 1, 4),
                     encode_ms=median_ms(lambda: codec.encode_interleaved(idx, part), args.reps),
                     decode_ms=median_ms(lambda: codec.decode_interleaved(d_pay, d_sz, B, part), args.reps))
            print(json.dumps(r), flush=True)
            res.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
