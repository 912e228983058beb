"""Device-event timings of the nearest-row search (vbq_topk.hip) on 100 000 x 100 and 400 000 x 300 matrices at N = 10 and
total_bits = 1, 3 and 6 bits per coordinate, Q = 1, 32 and 256 queries, k = 10, cosine.  Per (shape, rate, Q), in one process:

    records_ms   RecordEmbeddings.most_similar: the records searched as they are stored
    dense_ms     most_similar on the pre-decoded tensor: the same kernel with the dense row loader
    parent_ms    the route that existed before the fused search: tensor() (the full decode), then the matrix divided by
                 1e-8 + its row norms, a matmul with the normalised queries and torch.topk, written out below
    parent_search_ms   the same without the decode (a caller that keeps the decoded matrix around)

Every timed call ends in a device synchronise.  Median of --reps after two warm-up calls.  `*_bytes` is what each route must
read and write at the least (records: the record words once per block of 32 queries; dense: the matrix once per block; parent:
the records read and the matrix written by the decode, the matrix read and written by the normalisation, read by the matmul,
and the Q x V scores written and read) and `*_frac_of_copy` the resulting rate over the float4 copy rate bench.py records.  The
rank indices are synthetic (tools/records_bench.py): what is timed is the search, not the budget DP.  The ids of the three
routes are compared once per configuration (`ids_agree`: the share of the fused ids the torch route returns as well; scores
within rounding may swap).  Prints one JSON line per (shape, rate, Q)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.records_bench import HBM_COPY_MEASURED, _median_ms, synthetic_indices


def parent_search(emb, q, k):
    """Cosine top-k as a user of the decoded matrix writes it: no fused kernel, the whole score matrix in memory."""
    normed = emb / (1e-8 + torch.sqrt(torch.sum(emb * emb, dim=1, keepdim=True)))
    qn = q / (1e-8 + torch.sqrt(torch.sum(q * q, dim=1, keepdim=True)))
    scores, ids = torch.topk(qn @ normed.T, k, dim=1)
    return ids, scores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="100000x100,400000x300")
    ap.add_argument("--bits", default="1,3,6", help="total_bits per coordinate")
    ap.add_argument("--queries", default="1,32,256")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_bench needs a ROCm device")
    from vbq_amd import _lib, bitstream as bs, embeddings, ops, tables
    N, k = 10, args.k
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
            rec_bytes, mat_bytes = 4 * V * h.record_words, 4 * V * D
            for Q in (int(x) for x in args.queries.split(",")):
                q = torch.randn((Q, D), generator=gen, device="cuda")
                blocks = (Q + 31) // 32
                ws = int(_lib.lib().vbq_topk_workspace_bytes(V, D, Q, k, 0))
                r = dict(shape=[V, D], total_bits=total, record_words=h.record_words, Q=Q, k=k, metric="cosine",
                         records_ms=_median_ms(lambda: rec.most_similar(q, k=k), args.reps),
                         dense_ms=_median_ms(lambda: embeddings.most_similar(dense, q, k=k), args.reps),
                         parent_ms=_median_ms(lambda: parent_search(rec.tensor(), q, k), args.reps),
                         parent_search_ms=_median_ms(lambda: parent_search(dense, q, k), args.reps),
                         workspace_bytes=ws, records_bytes=blocks * rec_bytes, dense_bytes=blocks * mat_bytes,
                         parent_bytes=rec_bytes + 4 * mat_bytes + 8 * Q * V)
                for name in ("records", "dense", "parent"):
                    r[name + "_frac_of_copy"] = round(r[name + "_bytes"] / (r[name + "_ms"] * 1e-3) / HBM_COPY_MEASURED, 4)
                a = rec.most_similar(q, k=k)[0]
                b = embeddings.most_similar(dense, q, k=k)[0]
                c = parent_search(dense, q, k)[0]
                r["records_equal_dense"] = bool(torch.equal(a, b))
                r["ids_agree"] = round(float((a[:, :, None] == c[:, None, :]).any(dim=2).float().mean().item()), 6)
                print(json.dumps(r), flush=True)
                res.append(r)
            del rec, dense
            torch.cuda.empty_cache()
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
