"""Device-event timings of the scores of listed rows (vbq_amd/ext/vbqx_scores.hip) on a 100 000 x 100 record file at N = 10 and
3 bits per coordinate, cosine metric, uniformly random ids: word pairs (P = 353 and 3 000, one id per query, the queries are
rows themselves) and lists (Q x M = 1 x 64, 32 x 1 000, 1 024 x 1 000).  Per case, in one process:

    fused_ms          ops.records_scores on device tensors: one launch, straight from the records
    dense_ms          ops.scores on the pre-decoded tensor(): the same kernel with the dense row loader
    parent_ms         the route that existed before: ops.records_unpack of the listed rows into a [Q M, K] matrix, then torch
                      (the product with the queries summed over K, divided by 1e-8 + the rows' norms)
    gather_ms         the same torch reduction over tensor()[ids]: a gather from a resident decoded matrix
    api_ms            RecordEmbeddings.scores (lists) / .similarity (pairs) from host ids, behind their checks and uploads
    parent_api_ms     RecordEmbeddings.rows(ids) from host ids, then torch: what a user of the parent commit writes

Every timed call returns a device tensor and is followed by a device synchronise.  Median of --reps after two warm-up calls.
`*_peak_bytes` is the peak of torch's allocator over one call above what was allocated before it: the result plus every
intermediate.  The rank indices are synthetic (tools/records_bench.py): what is timed is the lookup, not the budget DP.
`fused_equals_dense` compares the two sources bit for bit, `max_abs_diff_parent` the fused result against the parent's (torch
sums in another order).  Prints one JSON line per case."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.bag_bench import _peak_bytes
from tools.records_bench import _median_ms, synthetic_indices


def _torch_scores(rows, q):
    """rows f32 [Q, M, K], q f32 [Q, K] -> [Q, M]."""
    return torch.einsum("qmk,qk->qm", rows, q) / (1e-8 + torch.sqrt((rows * rows).sum(-1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shape", default="100000x100")
    ap.add_argument("--bits", type=int, default=3, help="total_bits per coordinate")
    ap.add_argument("--pairs", default="353,3000")
    ap.add_argument("--lists", default="1x64,32x1000,1024x1000", help="queries x ids per query")
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scores_bench needs a ROCm device")
    from vbq_amd import bitstream as bs, embeddings, ops, tables
    N = 10
    V, K = (int(x) for x in args.shape.split("x"))
    total = args.bits * K
    cp, _ = embeddings.make_code_book(1.0, N)
    srt = tables.level_major_to_sorted(cp.astype(np.float32))[None]
    gen = torch.Generator(device="cuda").manual_seed(V + K)
    words = ops.records_pack(synthetic_indices(V, K, N, args.bits, gen), total, N)
    h = bs.RecordsHeader(N=N, shape=(V, K), C=1, total_bits=total)
    rec = embeddings.RecordEmbeddings(bs.write_records(h, srt, words.cpu().numpy()))
    del words
    dense = rec.tensor()
    w, tab = rec._words, rec._table
    cases = [("pairs", int(p), 1) for p in args.pairs.split(",")] + \
            [("lists",) + tuple(int(x) for x in s.split("x")) for s in args.lists.split(",")]
    res = []
    for kind, Q, M in cases:
        ids = torch.randint(0, V, (Q, M), generator=gen, device="cuda")
        ids_h = ids.cpu().numpy()
        if kind == "pairs":
            own = torch.randint(0, V, (Q,), generator=gen, device="cuda")
            own_h = own.cpu().numpy()
            q_raw = dense[own]
        else:
            q_raw = torch.randn((Q, K), generator=gen, device="cuda")
        q = embeddings._query_args(q_raw, K, "cosine", q_raw.device)
        routes = dict(
            fused=lambda: ops.records_scores(w, K, N, total, tab, q, ids, "cosine"),
            dense=lambda: ops.scores(dense, q, ids, "cosine"),
            parent=lambda: _torch_scores(ops.records_unpack(w, K, N, total, tab, ids.reshape(-1))[0].view(Q, M, K), q),
            gather=lambda: _torch_scores(dense[ids.reshape(-1)].view(Q, M, K), q))
        if kind == "pairs":
            routes["api"] = lambda: rec.similarity(own_h, ids_h[:, 0])
            routes["parent_api"] = lambda: _torch_scores(rec.rows(ids_h[:, 0])[:, None, :],
                                                         embeddings._query_args(rec.rows(own_h), K, "cosine", dense.device))
        else:
            routes["api"] = lambda: rec.scores(q_raw, ids_h)
            routes["parent_api"] = lambda: _torch_scores(rec.rows(ids_h.reshape(-1)).view(Q, M, K),
                                                         embeddings._query_args(q_raw, K, "cosine", dense.device))
        r = dict(kind=kind, shape=[V, K], total_bits=total, record_words=h.record_words, queries=Q, ids_per_query=M)
        for name, fn in routes.items():
            r[name + "_ms"] = _median_ms(fn, args.reps)
            r[name + "_peak_bytes"] = _peak_bytes(fn)
        a, b, c = routes["fused"](), routes["dense"](), routes["parent"]()
        r["fused_equals_dense"] = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
        r["max_abs_diff_parent"] = float((a - c).abs().max().item())
        r["result_bytes"], r["gathered_bytes"] = 4 * Q * M, 4 * Q * M * K
        print(json.dumps(r), flush=True)
        res.append(r)
        del a, b, c
        torch.cuda.empty_cache()
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
