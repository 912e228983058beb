#!/usr/bin/env python3
"""Developer tool (CPU only): what K2's LDS atomics cost on the bench's own indices, by the bank-conflict model of vbq_hist.hip.

    python tools/k2_conflict_model.py [--channels 8] [--cutoffs 3,4] [--per-lambda]

Runs the two-pass build of the bench's Kodak-24 inputs through the C oracle for a few channels (pass 1, length table, pass 2)
and deals every row's octets to the lanes as k_hist_flat does with one workgroup on the row (512 threads: octet o goes to
thread o % 512).  The model: a ds_add wave-instruction costs the largest number of its active lanes that meet on one of the 64
banks (same address included); an instruction without active lanes costs nothing.  Counted per channel (its 32 rows):
  plain     eight adds per octet, word 4 * slot(q) + (lane & 3)
  shipped   hist_add8: the thread's indices equal to its first one merged, the lanes that agree with the wave leader merged
            into one add of one lane
  hot Lh    the ranks of bit levels <= Lh in lane-private words (bank = lane), everything else as plain, no merging
  floor     one unit per wave-instruction
It also prints the share of a row's indices that the hot ranks of each cut-off hold.  The model is a count of conflicts, not
a time: EXPERIMENTS.md has what the kernels measured.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import LAMBDAS, N_BITS, make_inputs_with_table  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402
from oracle import vbq_oracle as O  # noqa: E402

THREADS = 512


def slot(q):
    return (q ^ (q >> 6)) & 2047


def worst_bank(word, active):
    """word, active: [instr, 64] -> per instruction the largest number of active lanes on one bank."""
    n = word.shape[0]
    flat = (np.arange(n)[:, None] * 64 + (word & 63))[active]
    return np.bincount(flat, minlength=n * 64).reshape(n, 64).max(axis=1)


def row_costs(row, cutoffs):
    """One row of ranks (a multiple of 8 * THREADS long) -> {scheme: model units}."""
    n_it = row.size // (8 * THREADS)
    q = row.astype(np.int64).reshape(n_it, THREADS // 64, 64, 8)              # [iteration, wave, lane, index of the octet]
    lane = np.arange(64)[None, None, :, None]
    cold = 4 * slot(q) + (lane & 3)
    instr = lambda a: a.transpose(0, 1, 3, 2).reshape(-1, 64)                  # -> [wave-instruction, lane]
    everyone = np.ones(instr(cold).shape, bool)
    out = {"floor": everyone.shape[0], "plain": int(worst_bank(instr(cold), everyone).sum())}
    # hist_add8: index j > 0 is added where it differs from the thread's first; the first where it differs from the leader's
    s = slot(q)
    same = s[..., 0] == s[:, :, :1, 0]                                         # lane 0 of a full wave is the leader
    active = np.concatenate([~same[..., None], s[..., 1:] != s[..., :1]], axis=3)
    out["shipped"] = int(worst_bank(instr(cold), instr(active)).sum()) + same.shape[0] * same.shape[1]      # + the leader's add
    m = q + 1
    for lh in cutoffs:
        sh = N_BITS - lh
        hot = (m & ((1 << sh) - 1)) == 0
        word = np.where(hot, 8192 + (m >> sh) * 64 + lane, cold)
        out[f"hot{lh}"] = int(worst_bank(instr(word), everyone).sum())
        out[f"share{lh}"] = float(hot.mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--cutoffs", default="3,4")
    ap.add_argument("--per-lambda", action="store_true")
    args = ap.parse_args()
    cutoffs = [int(c) for c in args.cutoffs.split(",")]
    rows, C, L = 36864, 256, len(LAMBDAS)
    mu, sg, tab = make_inputs_with_table(rows, C, 1000)
    ch = np.arange(args.channels) * (C // args.channels)
    mu, sg, tab = np.ascontiguousarray(mu[:, ch]), np.ascontiguousarray(sg[:, ch]), np.ascontiguousarray(tab[ch])
    th = CO.max_threads()
    idx1 = CO.quantize(mu, sg, tab, LAMBDAS, N=N_BITS, threads=th)                                   # pass 1: [L, rows, C]
    lev = O.levels_of_sorted_ranks(N_BITS)
    level_len = np.empty((L, len(ch), N_BITS + 1), np.float32)
    for l in range(L):
        counts = np.stack([np.bincount(lev[idx1[l, :, c]], minlength=N_BITS + 1) for c in range(len(ch))])
        level_len[l] = np.arange(N_BITS + 1, dtype=np.float32)[None, :] + O.neg_log2_freq(counts, 1)
    idx2 = CO.quantize(mu, sg, tab, LAMBDAS, N=N_BITS, level_len=level_len, threads=th)              # pass 2
    keys = ["plain", "shipped"] + [f"hot{c}" for c in cutoffs]
    total = dict.fromkeys(["floor"] + keys, 0.0)
    print(f"{len(ch)} channels of the Kodak-24 build, model units per channel and lambda (averages over the channels)")
    print("lambda     " + "".join(f"{k:>10s}" for k in keys) + "".join(f"   share<={c}" for c in cutoffs))
    for l in range(L):
        acc = {}
        for c in range(len(ch)):
            for k, v in row_costs(idx2[l, :, c], cutoffs).items():
                acc[k] = acc.get(k, 0.0) + v / len(ch)
        for k in total:
            total[k] += acc[k]
        if args.per_lambda:
            print(f"{LAMBDAS[l]:<10.4g} " + "".join(f"{acc[k]:10.0f}" for k in keys) + "".join(f"{acc[f'share{c}']:11.2f}" for c in cutoffs))
    print("total      " + "".join(f"{total[k]:10.0f}" for k in keys))
    print("x floor    " + "".join(f"{total[k] / total['floor']:10.2f}" for k in keys) + f"   (floor {total['floor']:.0f})")


if __name__ == "__main__":
    main()
