"""Crops of resident latent files (vbq_amd.store.LatentStore) against decompress_latents_batch from bytes, at C = 256.

  kodak   F = 24 and 256 Kodak-shaped files [1, 32, 48, 256] (24 distinct latents, repeated for F = 256) at segment 1024 and 64;
          per step S = F samples, as 16 x 16 crops at seeded origins and as whole files.
  large   F = 16 files [1, 256, 256, 256] (4 distinct latents, repeated) at segment 1024; per step S = F crops of 64 x 64.

Three forms of the same step, alternating inside one process, the same seeded draws for all three:
  A  q.decompress_latents_batch([files[i] for i in ids], regions): headers parsed, staging buffer built and uploaded, offsets
     scanned, boxes planned on the host, status read -- every step;
  B  store.crops(ids, origins, extents) with ids and origins already on the device, then one store.check(status, ids);
  C  store.crops with ids and origins as host lists (two small uploads per step), then the same check.
Each form is timed in rounds of --steps steps between two device events with a synchronise after the second, after a warm-up
round, until it has run for at least --seconds; the figure is the mean time per step.  plan_us is vbqs_plan_boxes alone (events
around --reps launches on the step's device ids).  One JSON line per case."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import LAMBDAS, make_inputs


def timed_round(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for k in range(steps):
        fn(k)
    b.record()
    b.synchronize()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(forms, steps, seconds):
    """{name: mean ms per step}: a warm-up round of every form, then rounds in turn until every form has `seconds` of work."""
    for fn in forms.values():
        timed_round(fn, steps)
    total, rounds = {n: 0.0 for n in forms}, {n: 0 for n in forms}
    while min(total.values()) < 1e3 * seconds:
        for name, fn in forms.items():
            total[name] += timed_round(fn, steps)
            rounds[name] += 1
    return {n: round(total[n] / (rounds[n] * steps), 4) for n in forms}, rounds


def case(q, files, dims, box, whole, steps, seconds, reps, seed):
    from vbq_amd.store import LatentStore, plan_boxes
    F = len(files)
    store = LatentStore(q, files)
    rng = np.random.default_rng(seed)
    draws = []
    for _ in range(steps):
        ids = np.arange(F, dtype=np.int64) if whole else rng.integers(0, F, F).astype(np.int64)
        origins = np.stack([rng.integers(0, D - w + 1, F) for D, w in zip(dims, box)], axis=1).astype(np.int64)
        regions = None if whole else [(slice(None), slice(int(o[1]), int(o[1]) + box[1]), slice(int(o[2]), int(o[2]) + box[2]))
                                      for o in origins]
        draws.append((ids, origins, regions, torch.from_numpy(ids).to(q.device), torch.from_numpy(origins).to(q.device),
                      ids.tolist(), origins.tolist()))
    ids, origins, regions, d_ids, d_origins, _, _ = draws[0]
    want = q.decompress_latents_batch([files[i] for i in ids], regions)
    got, status = store.crops(d_ids, d_origins, box)
    store.check(status, d_ids)
    assert torch.equal(got.view(want.shape), want), "the store differs from the batch call"

    def form_a(k):
        ids, _, regions = draws[k][:3]
        return q.decompress_latents_batch([files[i] for i in ids], regions)

    def form_b(k):
        out, status = store.crops(draws[k][3], draws[k][4], box)
        store.check(status, draws[k][3])
        return out

    def form_c(k):
        out, status = store.crops(draws[k][5], draws[k][6], box)
        store.check(status, draws[k][5])
        return out
    ms, rounds = alternate({"A": form_a, "B": form_b, "C": form_c}, steps, seconds)
    n_sel = store._n_sel(box)
    desc = torch.empty((F, store._fields), dtype=torch.int64, device=q.device)
    segs = torch.empty((F, n_sel), dtype=torch.int32, device=q.device)
    status = torch.zeros(F, dtype=torch.uint32, device=q.device)
    plan = lambda k: plan_boxes(store._table, d_ids, d_origins, box, seg=store.segment, n_sel=n_sel, desc=desc, segs=segs, status=status)
    timed_round(plan, reps)
    plan_us = 1e3 * min(timed_round(plan, reps) for _ in range(3)) / reps
    return dict(F=F, S=F, box=list(box), n_sel=n_sel, resident_bytes=store.nbytes, file_bytes=sum(len(d) for d in files),
                A_batch_from_bytes_ms=ms["A"], B_store_device_ids_ms=ms["B"], C_store_host_lists_ms=ms["C"],
                B_speedup_over_A=round(ms["A"] / ms["B"], 2), C_speedup_over_A=round(ms["A"] / ms["C"], 2), plan_us=round(plan_us, 2), rounds=rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="steps per timed round (each with its own seeded draw)")
    ap.add_argument("--seconds", type=float, default=0.5, help="least time of work per form")
    ap.add_argument("--reps", type=int, default=200, help="launches per timing of the plan kernel alone")
    ap.add_argument("--lambda-index", type=int, default=17)
    ap.add_argument("--files", type=int, nargs="*", default=[24, 256])
    ap.add_argument("--segments", type=int, nargs="*", default=[1024, 64])
    ap.add_argument("--no-large", action="store_true")
    ap.add_argument("--out", help="also write the results to this JSON file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("store_bench needs a ROCm device")
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
    for seg in args.segments:
        kodak = [q.compress_latents_to_bytes(m[i], v[i], lamb, segment=seg) for i in range(distinct)]
        for F in args.files:
            files = [kodak[i % distinct] for i in range(F)]
            for box, whole in (((1, 16, 16), False), ((1, 32, 48), True)):
                report(dict(case="kodak", shape=[1, 32, 48, C], segment=seg, whole=whole,
                            **case(q, files, (1, 32, 48), box, whole, args.steps, args.seconds, args.reps, F + seg)))
    if not args.no_large:
        side, big = 256, 4
        mu, sg = make_inputs(big * side * side, C, 1)
        m = mu.reshape(big, 1, side, side, C)
        v = (2 * np.log(sg)).astype(np.float32).reshape(big, 1, side, side, C)
        large = [q.compress_latents_to_bytes(m[i], v[i], lamb, segment=1024) for i in range(big)]
        del mu, sg, m, v
        report(dict(case="large", shape=[1, side, side, C], segment=1024, whole=False,
                    **case(q, [large[i % big] for i in range(16)], (1, side, side), (1, 64, 64), False, args.steps, args.seconds,
                           args.reps, 16)))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
