#!/usr/bin/env python3
"""Control of tests/test_gpu_fast_solve_variants.py: its launches of k_quant_fast<N, 0 | 1 | 2> and k_quant_pruned<N, 1 | 2>
for N = 4 .. 12 (one code book and planes), compared with the C oracle, as a program of its own -- VBQ_FAST_DEBUG is read
once per process, so the test starts this file once per value:
    VBQ_FAST_DEBUG=0 python tools/fast_solve_control.py     as built: no mismatch
    VBQ_FAST_DEBUG=1 ...                                    every solve through the literal scan: no mismatch
    VBQ_FAST_DEBUG=2 ...                                    K1's flags off: mismatches at every depth
Prints one line per (depth, kernel, data family) that misses the oracle and, last, the same as one JSON object
{"<N> <kernel> <family>": mismatching elements or counts}; exit code 1 if there is any, else 0."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np

import fast_solve_runs as FR
import launch_plans as LP
from vbq_amd import ops

FORMS = ("one", "cb")


def main():
    bad = {}

    def note(d, kernel, n):
        if n:
            key = f"{d.N} {kernel} {d.name}"
            bad[key] = bad.get(key, 0) + int(n)

    def per_chunk(d, plan, got, want):
        for i, kernel in enumerate(plan):
            sl = slice(i * LP.MAX_LAMBDA_CHUNK, (i + 1) * LP.MAX_LAMBDA_CHUNK)
            note(d, kernel, np.count_nonzero(got[sl] != want[sl]))

    for N in sorted(LP.SOLVE_DEPTHS):
        for d in FR.data(N):
            for form in FORMS:
                for L in FR.INDEX_L + FR.PRUNED_L:
                    plan = FR.plan(d, L, form)
                    assert plan == (FR.index_plan(L) if L in FR.INDEX_L else FR.pruned_plan(L)), (N, d.name, L, form, plan)
                    per_chunk(d, plan, FR.quantize(ops, d, L, form)[0], FR.expected(d, L, form)[0])
                for L in FR.OUTPUT_L:
                    plan = FR.plan(d, L, form, want_zhat=True, want_bits=True)
                    assert plan == FR.output_plan(L), (N, d.name, L, form, plan)
                    got, want = FR.quantize(ops, d, L, form, want_zhat=True, want_bits=True), FR.expected(d, L, form)
                    miss = (got[0] != want[0]) | (got[1].view(np.uint32) != want[1].view(np.uint32)) | (got[2] != want[2])
                    per_chunk(d, plan, miss, np.zeros_like(miss))
                for L in FR.COUNT_L:
                    plan = FR.plan(d, L, form, counting=True)
                    if plan == ["K1t"]:                                # N = 10, raw lengths: not this file's kernel
                        continue
                    assert plan[0] == "K1<2>" and set(plan) <= {"K1<2>", "K1t"}, (N, d.name, L, form, plan)
                    per_chunk(d, plan, FR.level_counts(ops, d, L, form), FR.expected_counts(d, L, form))
    for key in sorted(bad, key=lambda k: (int(k.split()[0]), k)):
        print(f"{key}: {bad[key]} mismatches")
    print(json.dumps(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
