"""Window and batch decode of lambda-map files (magic b"VBQm") against the one-file path, at C = 256, segment 1024.

  files    a loop of decompress_latents(return_np=False) over F Kodak-shaped lambda-map files [1, 32, 48, 256] (F = 1, 24, 256;
           24 distinct files, repeated for F = 256) against ONE decompress_latents_mapped_batch of the same files, for palettes
           of P = 2 and 4 lambdas and two class maps: `smooth` (P bands of rows) and `checker` (a change at every position).
  window   one [1, 256, 256, 256] lambda-map file (P = 2, smooth) decoded whole (decompress_latents) against a 64 x 64 window
           of it (decompress_latents_mapped_window).
  plain    what the class walk and the missing fc table cost per symbol: the same 24 latents as b"VBQb" files at one lambda
           through decompress_latents_batch (the plain kernel: fc table, no classes), the same files through
           decompress_latents_mapped_batch (no fc table, no class block), and as lambda-map files with a palette of ONE
           lambda through decompress_latents_mapped_batch (no fc table, a class block of zeros): the same symbols and the same
           payload words in all three.

Two clocks per case, as tools/window_bench.py.  wall: the host clock around a call that ends in a device synchronise -- upload,
launches and the status read included --, median of --reps calls after warm-up.  dev: device events around the launches alone,
on a staging buffer uploaded beforehand and with no status read (the offset scan and the window decode), median of --reps; the
loop has no dev column.  One JSON line per case."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import LAMBDAS, make_inputs
from tools.window_bench import device_ms, wall_ms, window_launches


def class_map(name, P, shape):
    i1, i2 = np.meshgrid(np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
    c = i1 * P // shape[1] if name == "smooth" else (i1 + i2) % P
    return np.broadcast_to(c, shape).astype(np.int64)


def mapped_launches(q, files, regions):
    """The launches of decompress_latents_mapped_batch(files, regions) on a staging buffer uploaded once."""
    plan = q._mapped_window_plan(files, regions, None)
    dev = torch.from_numpy(plan.host).to(q.device)
    return lambda: q._mapped_window_run(plan, dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lambda-indices", type=int, nargs=4, default=[17, 9, 25, 13], help="the palette: its first P entries")
    ap.add_argument("--files", type=int, nargs="*", default=[1, 24, 256])
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mapped_window_bench needs a ROCm device")
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    C, distinct, seg = 256, 24, 1024
    mu, sg = make_inputs(distinct * 32 * 48, C, 0)
    lv = (2 * np.log(sg)).astype(np.float32)
    q = ChannelwisePriorCDFQuantizer(C, 10)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C), mu.std(axis=0).astype(np.float64)))
    q.build_entropy_models_from_latents(mu, lv, LAMBDAS, add_n_smoothing=1, spread="logvar")
    palette = [LAMBDAS[i] for i in args.lambda_indices]
    res = []

    def report(r):
        print(json.dumps(r), flush=True)
        res.append(r)

    m, v = mu.reshape(distinct, 1, 32, 48, C), lv.reshape(distinct, 1, 32, 48, C)
    for P in (2, 4):
        for name in ("smooth", "checker"):
            cls = class_map(name, P, (1, 32, 48))
            kodak = [q.compress_latents_to_bytes_mapped(m[i], v[i], palette[:P], cls, segment=seg) for i in range(distinct)]
            for F in args.files:
                files = [kodak[i % distinct] for i in range(F)]
                want = torch.stack([q.decompress_latents(d, return_np=False) for d in files[:distinct]])
                got = q.decompress_latents_mapped_batch(files)
                assert torch.equal(got[:distinct], want) and torch.equal(got[-1], want[(F - 1) % distinct]), "the batch differs from the loop"
                report(dict(case="files", P=P, map=name, F=F, shape=[1, 32, 48, C], segment=seg, bytes=sum(len(d) for d in files),
                            loop_wall_ms=wall_ms(lambda: [q.decompress_latents(d, return_np=False) for d in files], args.reps),
                            batch_wall_ms=wall_ms(lambda: q.decompress_latents_mapped_batch(files), args.reps),
                            batch_dev_ms=device_ms(mapped_launches(q, files, None), args.reps)))
                del want, got

    # the same symbols three ways: the plain kernel, the mapped kernel without a class block, the mapped kernel with one
    zeros = np.zeros((1, 32, 48), np.int64)
    plain = [q.compress_latents_to_bytes(m[i], v[i], palette[0], segment=seg) for i in range(distinct)]
    single = [q.compress_latents_to_bytes_mapped(m[i], v[i], palette[:1], zeros, segment=seg) for i in range(distinct)]
    for F in args.files:
        a, b = [plain[i % distinct] for i in range(F)], [single[i % distinct] for i in range(F)]
        want = q.decompress_latents_batch(a)
        assert torch.equal(q.decompress_latents_mapped_batch(a), want) and torch.equal(q.decompress_latents_mapped_batch(b), want)
        report(dict(case="plain", F=F, shape=[1, 32, 48, C], segment=seg, symbols=F * 32 * 48 * C,
                    plain_kernel_wall_ms=wall_ms(lambda: q.decompress_latents_batch(a), args.reps),
                    mapped_kernel_wall_ms=wall_ms(lambda: q.decompress_latents_mapped_batch(a), args.reps),
                    mapped_kernel_class_block_wall_ms=wall_ms(lambda: q.decompress_latents_mapped_batch(b), args.reps),
                    plain_kernel_dev_ms=device_ms(window_launches(q, a, None), args.reps),
                    mapped_kernel_dev_ms=device_ms(mapped_launches(q, a, None), args.reps),
                    mapped_kernel_class_block_dev_ms=device_ms(mapped_launches(q, b, None), args.reps)))
        del want

    side, win = 256, (slice(None), slice(96, 160), slice(96, 160))
    mu, sg = make_inputs(side * side, C, 1)
    m, v = mu.reshape(1, side, side, C), (2 * np.log(sg)).astype(np.float32).reshape(1, side, side, C)
    data = q.compress_latents_to_bytes_mapped(m, v, palette[:2], class_map("smooth", 2, (1, side, side)), segment=seg)
    whole = q.decompress_latents(data, return_np=False)
    assert torch.equal(q.decompress_latents_mapped_window(data, win, return_np=False), whole[win]), "the window differs from the slice"
    assert torch.equal(q.decompress_latents_mapped_window(data, None, return_np=False), whole), "the whole window differs"
    plan = q._mapped_window_plan([data], [win], None)
    report(dict(case="window", P=2, map="smooth", shape=[1, side, side, C], window=[64, 64], segment=seg, bytes=len(data),
                segments_decoded=int(plan.n_sel), segments_per_channel=(side * side + seg - 1) // seg,
                whole_wall_ms=wall_ms(lambda: q.decompress_latents(data, return_np=False), args.reps),
                window_wall_ms=wall_ms(lambda: q.decompress_latents_mapped_window(data, win, return_np=False), args.reps),
                whole_by_window_wall_ms=wall_ms(lambda: q.decompress_latents_mapped_window(data, None, return_np=False), args.reps),
                window_dev_ms=device_ms(mapped_launches(q, [data], [win]), args.reps),
                whole_by_window_dev_ms=device_ms(mapped_launches(q, [data], [None]), args.reps)))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
