"""Device-event timings of the compressed-embedding byte string (vbq_amd.embeddings): compress_to_bytes, the load
(CompressedEmbeddings: upload + offsets), the full decode (tensor) and rows() of 1, 64 and 4096 random ids, on 100 000 x 100
and 400 000 x 300 matrices at one beta, for the default segment and for half / twice as many rows per segment.  Every call
ends in a device synchronise (the status word is read back), so the events bracket the whole call.  Prints one JSON line
per (shape, segment)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def _median_ms(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return round(sorted(t)[len(t) // 2], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--beta", type=float, default=17.0)
    ap.add_argument("--shapes", default="100000x100,400000x300")
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("embeddings_bitstream_bench needs a ROCm device")
    from vbq_amd import embeddings
    cp, _ = embeddings.make_code_book(1.0)
    res = []
    for spec in args.shapes.split(","):
        V, D = (int(x) for x in spec.split("x"))
        g = torch.Generator(device="cuda").manual_seed(V + D)
        means = torch.randn((V, D), generator=g, device="cuda")
        stds = torch.rand((V, D), generator=g, device="cuda") * 0.5 + 0.05
        want = embeddings.compress_coordinates(means, stds, args.beta, codepoints=cp)
        base = embeddings.default_segment(D) // D
        for per in sorted({max(1, base // 2), base, 2 * base}):
            seg = per * D
            data = embeddings.compress_to_bytes(means, stds, args.beta, cp, segment=seg)
            ce = embeddings.CompressedEmbeddings(data)
            assert torch.equal(ce.tensor().view(torch.int32), want.view(torch.int32)), "round trip differs"
            r = dict(shape=[V, D], beta=args.beta, segment=seg, default=seg == embeddings.default_segment(D), bytes=len(data),
                     bits_per_coordinate=round(ce.bits_per_coordinate, 4),
                     compress_ms=_median_ms(lambda: embeddings.compress_to_bytes(means, stds, args.beta, cp, segment=seg),
                                            args.reps),
                     load_ms=_median_ms(lambda: embeddings.CompressedEmbeddings(data), args.reps),
                     decode_all_ms=_median_ms(ce.tensor, args.reps))
            rng = np.random.default_rng(0)
            for k in (1, 64, 4096):
                ids = rng.integers(0, V, k)
                r[f"rows_{k}_ms"] = _median_ms(lambda: ce.rows(ids), args.reps)
            print(json.dumps(r), flush=True)
            res.append(r)
            del ce
        del means, stds, want
        torch.cuda.empty_cache()
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
