"""Device-event timings of the pooled lookup (vbq_bag.hip) on 100 000 x 300 and 400 000 x 300 record files at N = 10 and
total_bits = 1, 3 and 6 bits per coordinate, for four bag shapes (bags x ids per bag): 1 x 3, 4 096 x 16, 100 000 x 8 and
16 x 4 096, mode "sum", uniformly random ids.  Per (shape, rate, bag shape), in one process:

    fused_ms          ops.records_bag on device tensors: one launch, straight from the records
    dense_ms          ops.bag on the pre-decoded tensor(): the same kernel with the dense row loader
    parent_ms         the route that existed before: RecordEmbeddings.rows(ids) (host range check, upload, the unpack into a
                      [len(ids), K] matrix), then torch's reduction -- the bags here are equally long, so that is
                      .view(B, L, K).sum(1), the cheapest form a user can write
    parent_device_ms  the same without the host check: ops.records_unpack on device ids, then the reduction
    embedding_bag_ms  torch.nn.functional.embedding_bag on tensor() (needs the decoded matrix, as dense_ms does)
    api_ms            RecordEmbeddings.bag from host ids: the fused launch behind its host checks and uploads (against parent_ms)

Every timed call returns a device tensor and is followed by a device synchronise.  Median of --reps after two warm-up calls.
`*_bytes` is what each route must read and write at the least (fused: ids, offsets, the records listed, the result; dense: the
rows in place of the records; parent: the records read, the rows written and read back, the result).  `*_peak_bytes` is the
peak of torch's allocator over one call above what was allocated before it: the result plus every intermediate.  The rank
indices are synthetic (tools/records_bench.py): what is timed is the lookup, not the budget DP.  `fused_equals_dense` compares
the two sources bit for bit, `max_abs_diff_parent` the fused result against the parent's (torch sums in another order).  Prints
one JSON line per (shape, rate, bag shape)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.records_bench import _median_ms, synthetic_indices


def _peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="100000x300,400000x300")
    ap.add_argument("--bits", default="1,3,6", help="total_bits per coordinate")
    ap.add_argument("--bags", default="1x3,4096x16,100000x8,16x4096", help="bags x ids per bag")
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bag_bench needs a ROCm device")
    from vbq_amd import bitstream as bs, embeddings, ops, tables
    N = 10
    cp, _ = embeddings.make_code_book(1.0, N)
    srt = tables.level_major_to_sorted(cp.astype(np.float32))[None]
    res = []
    for spec in args.shapes.split(","):
        V, D = (int(x) for x in spec.split("x"))
        gen = torch.Generator(device="cuda").manual_seed(V + D)
        for bits in (int(b) for b in args.bits.split(",")):
            total = bits * D
            idx = synthetic_indices(V, D, N, bits, gen)
            words = ops.records_pack(idx, total, N)
            h = bs.RecordsHeader(N=N, shape=(V, D), C=1, total_bits=total)
            rec = embeddings.RecordEmbeddings(bs.write_records(h, srt, words.cpu().numpy()))
            del idx, words
            dense = rec.tensor()
            w, tab = rec._words, rec._table
            for B, L in ((int(x) for x in b.split("x")) for b in args.bags.split(",")):
                n = B * L
                ids = torch.randint(0, V, (n,), generator=gen, device="cuda")
                offsets = torch.arange(B + 1, device="cuda") * L
                ids_h, starts_h = ids.cpu().numpy(), offsets[:-1].cpu().numpy()
                routes = dict(
                    fused=lambda: ops.records_bag(w, D, N, total, tab, ids, offsets),
                    dense=lambda: ops.bag(dense, ids, offsets),
                    parent=lambda: rec.rows(ids_h).view(B, L, D).sum(1),
                    parent_device=lambda: ops.records_unpack(w, D, N, total, tab, ids)[0].view(B, L, D).sum(1),
                    embedding_bag=lambda: torch.nn.functional.embedding_bag(ids, dense, offsets[:-1], mode="sum"),
                    api=lambda: rec.bag(ids_h, starts_h))
                r = dict(shape=[V, D], total_bits=total, record_words=h.record_words, bags=B, ids_per_bag=L, mode="sum")
                for name, fn in routes.items():
                    r[name + "_ms"] = _median_ms(fn, args.reps)
                    r[name + "_peak_bytes"] = _peak_bytes(fn)
                lists, result = 8 * n + 8 * (B + 1), 4 * B * D
                r["fused_bytes"] = lists + 4 * n * h.record_words + result
                r["dense_bytes"] = lists + 4 * n * D + result
                r["parent_bytes"] = 8 * n + 4 * n * h.record_words + 2 * 4 * n * D + result
                a, b, c = routes["fused"](), routes["dense"](), routes["parent_device"]()
                r["fused_equals_dense"] = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
                r["max_abs_diff_parent"] = float((a - c).abs().max().item())
                print(json.dumps(r), flush=True)
                res.append(r)
                del a, b, c, ids, offsets
            del rec, dense, w, tab
            torch.cuda.empty_cache()
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
