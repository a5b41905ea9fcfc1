# -*- coding: utf-8 -*-
"""Times vqh_curve_filter (csrc/filter.hip) on one MI355X: B curves of one length, the fixture's walks of that length tiled.
HIP events around each launch pair (screen + compaction), warm-up, median / min / max over the repeats; prints one JSON line
per shape with the achieved pair evaluations per second (point pairs + segment pairs the two O(L^2) loops visit).

    python tools/gpu_filter_probe.py [--batch 4096] [--lengths 350 64] [--reps 50] [--warmup 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pytorch-vae_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--lengths", type=int, nargs="+", default=[350, 64])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    from vqvae_hip import curve_filter as F
    from vqvae_hip.lib import require_gpu
    require_gpu()
    fx = np.load(os.path.join(ROOT, "tests", "golden", "curve_filter.npz"), allow_pickle=False)
    offs = np.concatenate([[0], np.cumsum(fx["lengths"])])
    params = F.params_from_dict(json.loads(str(fx["param_sets"][1])))
    lines = []
    for L in args.lengths:
        rows = [k for k, (n, c) in enumerate(zip(fx["lengths"], fx["channels"])) if n == L and c == 6]
        assert rows, f"the fixture has no walk of length {L}"
        base = torch.from_numpy(np.stack([fx["curves"][offs[k]:offs[k + 1]] for k in rows]))
        x = base.repeat((args.batch + len(rows) - 1) // len(rows), 1, 1)[:args.batch].contiguous().cuda()
        lens = torch.full((args.batch,), L, dtype=torch.int32, device="cuda")
        times = []
        for it in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = F.filter_curves(x, lengths=lens, params=params)
            e1.record()
            e1.synchronize()
            if it >= args.warmup:
                times.append(e0.elapsed_time(e1) * 1e-3)
        ne, nes = params.neighbor_exclude, params.seg_neighbor_exclude
        tri = lambda n, ex: max(n - ex - 1, 0) * max(n - ex, 0) // 2          # pairs i < j with j - i > ex
        pairs = args.batch * (tri(L, ne) + tri(L - 1, nes))
        med = statistics.median(times)
        line = dict(probe="curve_filter", device=torch.cuda.get_device_name(0), B=args.batch, L=L, reps=args.reps,
                    seconds_median=med, seconds_min=min(times), seconds_max=max(times),
                    us_per_curve=med / args.batch * 1e6, curves_per_s=args.batch / med, pair_evals=pairs,
                    pair_evals_per_s=pairs / med, kept=int(res.n_keep.item()),
                    hbm_bytes=int(x.numel() * 4 + args.batch * (4 + 14 * 4 + 12 * 4 + 4)))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(l) for l in lines) + "\n")


if __name__ == "__main__":
    main()
