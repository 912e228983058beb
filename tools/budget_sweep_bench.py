"""Device-event timings of the budget sweep (vbqb_budget_sweep_f64) at the size it is for: every row of a [100000, 100] embedding
matrix, N = 10, one shared code book, at the budgets 100, 200, ..., 600 in ONE forward pass -- against the SUM of one
vbq_budget_dp_f64 launch per budget from the same run, and against the one launch at the largest budget.  Also the curve-only
pass at width K N + 1, and end to end: quantize_rows_to_budgets against the loop of quantize_rows_to_budget,
compress_to_records_sweep against the loop of compress_to_records.  Every time is the median of --reps warm runs between two
device events (end to end: of max(3, reps / 4)).  The sweep's slices are checked against the single launches before anything is
timed.  One JSON line per measurement."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


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


def launch_shape(K, N, width, S):
    """What vbqb_sweep.hip's sweep_plan decides (restated here for the report only)."""
    threads = 64 if width <= 64 else (128 if width <= 128 else 256)
    values = (2 * width + 2 * (N + 1)) * 8 + 16
    bp = (K * width + 15) // 16 * 16
    in_lds = values + bp <= 160 * 1024
    lds = values + (bp if S and in_lds else 0)
    per_cu = min(160 * 1024 // lds, 32 // (threads // 64))
    return dict(threads=threads, lds_bytes=lds, back_pointers=("lds" if in_lds else "workspace") if S else "none",
                workgroups_per_cu=per_cu)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--N", type=int, default=10)
    ap.add_argument("--budgets", type=int, nargs="+", default=[100, 200, 300, 400, 500, 600])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true", help="skip the end-to-end timings")
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("budget_sweep_bench needs a ROCm device")
    import vbq_amd
    from vbq_amd import embeddings as E, ops, rows_budget
    R, K, N, budgets = args.rows, args.K, args.N, sorted(set(args.budgets))
    g = torch.Generator(device="cuda").manual_seed(R + K)
    mu = torch.randn((R, K), generator=g, device="cuda")
    sg = torch.exp(-2 + 0.7 * torch.randn((R, K), generator=g, device="cuda")).clamp(1e-4, 10)
    tab = vbq_amd.gaussian_table(1.0, N=N)[0]
    scores, _ = rows_budget.level_candidates(mu, sg, torch.from_numpy(tab).cuda()[None], N)
    res = []

    def report(**r):
        print(json.dumps(r), flush=True)
        res.append(r)

    bits, obj, curve = ops.budget_dp_sweep(scores, K, budgets, curve_len=K * N + 1)
    for s, b in enumerate(budgets):
        one_bits, one_obj = ops.budget_dp(scores, K, b)
        assert torch.equal(bits[s], one_bits) and torch.equal(obj[s].view(torch.int64), one_obj.view(torch.int64)), b
        assert torch.equal(curve[:, b].view(torch.int64), one_obj.view(torch.int64)), b
    del bits, obj, curve, one_bits, one_obj
    single = {b: _median_ms(lambda: ops.budget_dp(scores, K, b), args.reps) for b in budgets}
    sweep = _median_ms(lambda: ops.budget_dp_sweep(scores, K, budgets), args.reps)
    loop = round(sum(single.values()), 4)
    report(what="kernel", shape=[R, K], N=N, budgets=budgets, **launch_shape(K, N, budgets[-1] + 1, len(budgets)),
           single_launch_ms=single, loop_ms=loop, largest_ms=single[budgets[-1]], sweep_ms=sweep,
           loop_over_sweep=round(loop / sweep, 3), sweep_over_largest=round(sweep / single[budgets[-1]], 3))
    report(what="curve_only", shape=[R, K], N=N, width=K * N + 1, **launch_shape(K, N, K * N + 1, 0),
           curve_ms=_median_ms(lambda: ops.budget_dp_sweep(scores, K, [], curve_len=K * N + 1), args.reps))
    report(what="sweep_with_curve", shape=[R, K], N=N, budgets=budgets, width=K * N + 1,
           **launch_shape(K, N, K * N + 1, len(budgets)),
           sweep_ms=_median_ms(lambda: ops.budget_dp_sweep(scores, K, budgets, curve_len=K * N + 1), args.reps))
    if not args.kernel_only:
        del scores
        reps = max(3, args.reps // 4)
        many = _median_ms(lambda: vbq_amd.quantize_rows_to_budgets(mu, sg, budgets, table=tab, N=N), reps)
        each = _median_ms(lambda: [vbq_amd.quantize_rows_to_budget(mu, sg, b, table=tab, N=N) for b in budgets], reps)
        report(what="quantize_rows", budgets=budgets, quantize_rows_to_budgets_ms=many, loop_of_quantize_rows_to_budget_ms=each,
               loop_over_sweep=round(each / many, 3))
        many = _median_ms(lambda: E.compress_to_records_sweep(mu, sg, budgets, tab, N), reps)
        each = _median_ms(lambda: [E.compress_to_records(mu, sg, b, tab, N) for b in budgets], reps)
        report(what="compress_to_records", budgets=budgets, compress_to_records_sweep_ms=many, loop_of_compress_to_records_ms=each,
               loop_over_sweep=round(each / many, 3))
        report(what="records_distortion_curve",
               records_distortion_curve_ms=_median_ms(lambda: E.records_distortion_curve(mu, sg, tab, N), reps))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
