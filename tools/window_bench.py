"""Window and batch decode of latent files against the one-file path, at C = 256.

  files   a loop of decompress_latents(return_np=False) over F Kodak-shaped files [1, 32, 48, 256] (F = 1, 24, 256; 24
          distinct files, repeated for F = 256) against ONE decompress_latents_batch of the same files.
  window  one [1, 256, 256, 256] file decoded whole (decompress_latents) against a 64 x 64 window of it
          (decompress_latents_window), at segment 1024 and 64.

Two clocks per case.  wall: the host clock around a call that ends in a device synchronise -- upload, launches and the status
read included --, median of --reps calls after warm-up.  dev: device events around the launches alone, on buffers uploaded
beforehand and with no status read in between (the loop: unpack, decode and gather per file; the batch and the window: the
offset scan and the window decode), median of --reps.  One JSON line per case."""
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
        fn()
        torch.cuda.synchronize()
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


def one_file_launches(q, data):
    """The launches of decompress_latents(data) on a buffer uploaded once: unpack, decode, gather; no status read."""
    from vbq_amd import bitstream, ops
    h, _, _ = bitstream.parse(data)
    codec, _ = q._coder_tables(q._lambda_key(h.lamb), h.segment)
    tail = np.frombuffer(memoryview(data).cast("B"), dtype="<u2", count=h.n_sizes + h.n_words, offset=h.nbytes)
    buf = torch.from_numpy(tail.copy()).to(q.device)
    idx = torch.empty((h.C, h.n_rows), dtype=torch.uint16, device=q.device)
    status = torch.zeros(1, dtype=torch.uint32, device=q.device)

    def launch():
        words, sizes, _ = codec.unpack_device(buf[h.n_sizes:], buf[: h.n_sizes], h.n_rows, status)
        codec._decode(words, sizes, None, h.n_rows, idx, status)
        return ops.gather(idx[None], q._sorted_dev(), h.C, N=h.N, layout="cb", out_layout="bc")
    return launch


def window_launches(q, files, regions):
    """The launches of decompress_latents_batch(files, regions) on a staging buffer uploaded once."""
    plan = q._window_plan(files, regions, None)
    dev = torch.from_numpy(plan.host).to(q.device)
    return lambda: q._window_run(plan, dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lambda-index", type=int, default=17)
    ap.add_argument("--files", type=int, nargs="*", default=[1, 24, 256])
    ap.add_argument("--segments", type=int, nargs="*", default=[1024, 64])
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_bench needs a ROCm device")
    from vbq_amd import ChannelwisePriorCDFQuantizer, priors
    C, distinct = 256, 24
    mu, sg = make_inputs(distinct * 32 * 48, C, 0)
    lv = (2 * np.log(sg)).astype(np.float32)
    q = ChannelwisePriorCDFQuantizer(C, 10)
    q.build_code_points(priors.FactoredGaussianPrior(np.zeros(C), mu.std(axis=0).astype(np.float64)))
    q.build_entropy_models_from_latents(mu, lv, LAMBDAS, add_n_smoothing=1, spread="logvar")
    lamb = LAMBDAS[args.lambda_index]
    res = []

    def report(r):
        print(json.dumps(r), flush=True)
        res.append(r)

    m, v = mu.reshape(distinct, 1, 32, 48, C), lv.reshape(distinct, 1, 32, 48, C)
    kodak = [q.compress_latents_to_bytes(m[i], v[i], lamb, segment=1024) for i in range(distinct)]
    for F in args.files:
        files = [kodak[i % distinct] for i in range(F)]
        want = torch.stack([q.decompress_latents(d, return_np=False) for d in files[:distinct]])
        got = q.decompress_latents_batch(files)
        assert torch.equal(got[:distinct], want) and torch.equal(got[-1], want[(F - 1) % distinct]), "the batch differs from the loop"
        one = [one_file_launches(q, d) for d in kodak[: min(F, distinct)]]
        report(dict(case="files", F=F, shape=[1, 32, 48, C], segment=1024, bytes=sum(len(d) for d in files),
                    loop_wall_ms=wall_ms(lambda: [q.decompress_latents(d, return_np=False) for d in files], args.reps),
                    batch_wall_ms=wall_ms(lambda: q.decompress_latents_batch(files), args.reps),
                    loop_dev_ms=device_ms(lambda: [one[i % len(one)]() for i in range(F)], args.reps),
                    batch_dev_ms=device_ms(window_launches(q, files, None), args.reps)))
        del want, got

    side, win = 256, (slice(None), slice(96, 160), slice(96, 160))
    mu, sg = make_inputs(side * side, C, 1)
    m, v = mu.reshape(1, side, side, C), (2 * np.log(sg)).astype(np.float32).reshape(1, side, side, C)
    for seg in args.segments:
        data = q.compress_latents_to_bytes(m, v, lamb, segment=seg)
        whole = q.decompress_latents(data, return_np=False)
        assert torch.equal(q.decompress_latents_window(data, win, return_np=False), whole[win]), "the window differs from the slice"
        assert torch.equal(q.decompress_latents_window(data, None, return_np=False), whole), "the whole window differs"
        plan = q._window_plan([data], [win], None)
        report(dict(case="window", shape=[1, side, side, C], window=[64, 64], segment=seg, bytes=len(data),
                    segments_decoded=int(plan.n_sel), segments_per_channel=(side * side + seg - 1) // seg,
                    whole_wall_ms=wall_ms(lambda: q.decompress_latents(data, return_np=False), args.reps),
                    window_wall_ms=wall_ms(lambda: q.decompress_latents_window(data, win, return_np=False), args.reps),
                    whole_by_window_wall_ms=wall_ms(lambda: q.decompress_latents_window(data, None, return_np=False), args.reps),
                    whole_dev_ms=device_ms(one_file_launches(q, data), args.reps),
                    window_dev_ms=device_ms(window_launches(q, [data], [win]), args.reps),
                    whole_by_window_dev_ms=device_ms(window_launches(q, [data], [None]), args.reps)))
        del whole
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
