"""Device-event timings of the budget DP (vbq_budget_dp_f64) at the size it is for: every row of a [100000, 100] embedding matrix
at exactly `budget` raw bits, N = 10, budgets 100, 300 and 600.  Times the kernel alone on a prepared score table (median of
--reps warm launches between two device events) and quantize_rows_to_budget end to end; next to them the float64 NumPy restatement
(tests/budget_reference.py) on a sample of the same rows on this host, scaled to the full row count.  Also prints the launch
shape: threads per workgroup, LDS per workgroup and the workgroups one CU holds.  One JSON line per budget."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import budget_reference as BR


def _median_ms(fn, reps):
    for _ in range(3):
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


def launch_shape(K, N, budget):
    """What vbq_budget.hip's budget_plan decides (restated here for the report only)."""
    W = budget + 1
    threads = 64 if W <= 64 else (128 if W <= 128 else 256)
    values = (2 * W + 2 * (N + 1)) * 8 + 16
    bp = (K * W + 15) // 16 * 16
    in_lds = values + bp <= 160 * 1024
    lds = values + (bp if in_lds else 0)
    per_cu = min(160 * 1024 // lds, 32 // (threads // 64))
    return dict(threads=threads, lds_bytes=lds, back_pointers="lds" if in_lds else "workspace", workgroups_per_cu=per_cu)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--N", type=int, default=10)
    ap.add_argument("--budgets", type=int, nargs="+", default=[100, 300, 600])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--numpy-rows", type=int, default=64, help="rows of the sample the NumPy restatement is timed on")
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("budget_dp_bench needs a ROCm device")
    import vbq_amd
    from vbq_amd import ops, rows_budget
    R, K, N = args.rows, args.K, args.N
    g = torch.Generator(device="cuda").manual_seed(R + K)
    mu = torch.randn((R, K), generator=g, device="cuda")
    sg = torch.exp(-2 + 0.7 * torch.randn((R, K), generator=g, device="cuda")).clamp(1e-4, 10)
    tab = vbq_amd.gaussian_table(1.0, N=N)[0]
    scores, _ = rows_budget.level_candidates(mu, sg, torch.from_numpy(tab).cuda()[None], N)
    sample = scores[:, : args.numpy_rows].cpu().numpy()
    res = []
    for budget in args.budgets:
        bits, obj = ops.budget_dp(scores, K, budget)
        want_bits, want_obj = BR.budget_dp_rows(sample, budget)
        assert np.array_equal(bits[: args.numpy_rows].cpu().numpy(), want_bits), "kernel != restatement"
        assert obj[: args.numpy_rows].cpu().numpy().tobytes() == want_obj.tobytes(), "kernel != restatement"
        t0 = time.perf_counter()
        BR.budget_dp_rows(sample, budget)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        r = dict(shape=[R, K], N=N, budget=budget, **launch_shape(K, N, budget),
                 kernel_ms=_median_ms(lambda: ops.budget_dp(scores, K, budget), args.reps),
                 quantize_rows_to_budget_ms=_median_ms(lambda: vbq_amd.quantize_rows_to_budget(mu, sg, budget, table=tab, N=N),
                                                       max(3, args.reps // 4)),
                 numpy_rows=args.numpy_rows, numpy_sample_ms=round(numpy_ms, 2),
                 numpy_scaled_to_all_rows_s=round(numpy_ms * R / args.numpy_rows / 1e3, 1))
        print(json.dumps(r), flush=True)
        res.append(r)
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
