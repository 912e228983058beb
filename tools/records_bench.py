"""Device-event timings of the record file (vbq_amd.embeddings, "VBQr"): the pack launch, the load (RecordEmbeddings: upload
+ the validating pass), the full decode (tensor) and rows() of 1, 64 and 4096 random ids, on 100 000 x 100 and 400 000 x 300
matrices at N = 10 and total_bits = 1, 3 and 6 bits per coordinate; beside each, in the same run, the same calls on the rANS
file ("VBQe", CompressedEmbeddings, default segment) whose whole-file rate is nearest.  Every timed call ends in a device
synchronise.  Median of --reps after two warm-up calls.

The rank indices are synthetic -- per row, pairs of coordinates at (b + s, b - s) bits with random s and random codes, so every
row spends exactly total_bits -- because what is timed here is the format, not the budget DP (tools/budget_dp_bench.py times
that); --dp additionally times compress_to_records end to end.  The unpack's bytes are the records read plus the float32
values written; `frac_of_measured_copy` is that rate over the float4 copy rate bench.py records (HBM_COPY_MEASURED).
Prints one JSON line per (shape, rate)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

HBM_COPY_MEASURED = 6.29e12            # bench.py


def _median_ms(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        torch.cuda.synchronize()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return round(sorted(t)[len(t) // 2], 4)


def synthetic_indices(V, D, N, bits, gen):
    """u16 [V, D] rank indices whose bit lengths add up to bits * D in every row."""
    assert D % 2 == 0 and 0 <= bits <= N
    room = min(bits, N - bits)
    s = torch.randint(0, room + 1, (V, D // 2), generator=gen, device=gen.device)
    n = torch.stack([bits + s, bits - s], dim=2).reshape(V, D)
    j = torch.randint(0, 1 << N, (V, D), generator=gen, device=gen.device) & (torch.bitwise_left_shift(torch.ones_like(n), n) - 1)
    return (((2 * j + 1) << (N - n)) - 1).to(torch.uint16)


def _lookups(obj, V, reps):
    rng = np.random.default_rng(0)
    return {f"rows_{k}_ms": _median_ms(lambda ids=rng.integers(0, V, k): obj.rows(ids), reps) for k in (1, 64, 4096)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="100000x100,400000x300")
    ap.add_argument("--bits", default="1,3,6", help="total_bits per coordinate")
    ap.add_argument("--betas", default="0.001,0.03,0.3,3,30,300,3000", help="candidate betas of the rANS baseline")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--dp", action="store_true", help="also time compress_to_records (budget DP + pack + copy)")
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("records_bench needs a ROCm device")
    from vbq_amd import bitstream as bs, embeddings, ops, tables
    N = 10
    cp, _ = embeddings.make_code_book(1.0, N)
    srt = tables.level_major_to_sorted(cp.astype(np.float32))[None]
    res = []
    for spec in args.shapes.split(","):
        V, D = (int(x) for x in spec.split("x"))
        gen = torch.Generator(device="cuda").manual_seed(V + D)
        means = torch.randn((V, D), generator=gen, device="cuda")
        stds = torch.rand((V, D), generator=gen, device="cuda") * 0.5 + 0.05
        base = {}
        if not args.no_baseline:
            betas = [float(b) for b in args.betas.split(",")]
            nbytes = embeddings.coded_nbytes(means, stds, betas, cp)
            base = {b: 8.0 * int(nb) / (V * D) for b, nb in zip(betas, nbytes)}
        for bits in (int(b) for b in args.bits.split(",")):
            total = bits * D
            idx = synthetic_indices(V, D, N, bits, gen)
            st = torch.zeros(1, dtype=torch.uint32, device="cuda")
            words = ops.records_pack(idx, total, N, status=st)
            assert int(st.cpu().item()) == 0
            h = bs.RecordsHeader(N=N, shape=(V, D), C=1, total_bits=total)
            data = bs.write_records(h, srt, words.cpu().numpy())
            re_ = embeddings.RecordEmbeddings(data)
            want = torch.from_numpy(srt[0]).cuda()[idx.view(torch.int16).to(torch.int64) & 0xFFFF]
            assert torch.equal(re_.tensor(), want), "round trip differs"
            r = dict(format="VBQr", shape=[V, D], total_bits=total, record_words=h.record_words, bytes=len(data),
                     bits_per_coordinate=round(re_.bits_per_coordinate, 4),
                     pack_ms=_median_ms(lambda: ops.records_pack(idx, total, N), args.reps),
                     load_ms=_median_ms(lambda: embeddings.RecordEmbeddings(data), args.reps),
                     decode_all_ms=_median_ms(re_.tensor, args.reps))
            moved = 4 * V * h.record_words + 4 * V * D
            r["unpack_bytes"] = moved
            r["unpack_tb_per_s"] = round(moved / (r["decode_all_ms"] * 1e-3) / 1e12, 4)
            r["frac_of_measured_copy"] = round(moved / (r["decode_all_ms"] * 1e-3) / HBM_COPY_MEASURED, 4)
            r.update(_lookups(re_, V, args.reps))
            if args.dp:
                r["compress_to_records_ms"] = _median_ms(lambda: embeddings.compress_to_records(means, stds, total, cp, N),
                                                         max(3, args.reps // 4))
            print(json.dumps(r), flush=True)
            res.append(r)
            del re_, words, idx, want
            if base:
                beta = min(base, key=lambda b: abs(base[b] - r["bits_per_coordinate"]))
                e = embeddings.compress_to_bytes(means, stds, beta, cp)
                ce = embeddings.CompressedEmbeddings(e)
                q = dict(format="VBQe", shape=[V, D], beta=beta, segment=ce.header.segment, bytes=len(e),
                         bits_per_coordinate=round(ce.bits_per_coordinate, 4), nearest_to=r["bits_per_coordinate"],
                         load_ms=_median_ms(lambda: embeddings.CompressedEmbeddings(e), args.reps),
                         decode_all_ms=_median_ms(ce.tensor, args.reps))
                q.update(_lookups(ce, V, args.reps))
                print(json.dumps(q), flush=True)
                res.append(q)
                del ce
            torch.cuda.empty_cache()
        del means, stds
        torch.cuda.empty_cache()
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
