#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""Filter decoded curves by geometric and secondary-structure heuristics -- same flags, kept files, [summary] counters and
manifest records as the reference's prior/filter_curves.py, with the screening done on the GPU:

    python prior/filter_curves.py --recon_dir results/decoded_npy --out_dir results/decoded_npy_filtered \\
        --min_pairwise_dist 2.0 --neighbor_exclude 2 --min_length 2

The *.npy files are loaded on the host, packed into padded batches (by channel count, sorted by length) and screened by
vqvae_hip.curve_filter.filter_curves in a few launches; the accept order, --max_curves and the manifest merge are applied
on the host in the sorted file order."""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

SUMMARY_LABELS = ("total curves", "kept", "rejected (too short)", "rejected (too long)",
                  "rejected (bond length out-of-range)", "rejected (bond angle out-of-range)",
                  "rejected (point self-collision)", "rejected (segment self-intersection)", "rejected (ss heuristics)")
RECORD_FLOATS = ("rg", "bond_mean", "bond_std", "bond_min", "bond_max", "bond_frac_out", "angle_mean", "angle_std",
                 "angle_min", "angle_max", "angle_frac_out")
BATCH_CURVES = 4096


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--recon_dir", type=str, required=True, help="directory with the decoded *.npy curves")
    ap.add_argument("--out_dir", type=str, required=True, help="directory the kept curves are copied to")
    ap.add_argument("--samples_manifest", type=str, default="", help="optional samples manifest (jsonl) to merge by index")
    ap.add_argument("--filtered_manifest_out", type=str, default="", help="optional path of the filtered manifest (jsonl)")
    ap.add_argument("--min_length", type=int, default=32)
    ap.add_argument("--max_length", type=int, default=0, help="0 = no upper bound")
    ap.add_argument("--min_pairwise_dist", type=float, default=1.0,
                    help="curves with two non-neighbour points closer than this are rejected")
    ap.add_argument("--neighbor_exclude", type=int, default=2, help="pairs with |i-j| <= this are not collision-checked")
    ap.add_argument("--min_beta_run", type=int, default=0, help="> 0: longest beta run must reach this when beta exists")
    ap.add_argument("--min_beta_total", type=int, default=0, help="> 0: reject 0 < beta residues < this")
    ap.add_argument("--beta_channel", type=int, default=1, help="index of the beta channel among the three SS channels")
    ap.add_argument("--max_curves", type=int, default=0, help="stop after this many kept curves (0 = no cap)")
    ap.add_argument("--min_beta_sheet_fraction", type=float, default=0.0,
                    help="> 0: at least this fraction of beta residues must have a sheet partner")
    ap.add_argument("--max_isolated_beta_strands", type=int, default=-1,
                    help=">= 0: reject curves with more partner-less strands than this")
    ap.add_argument("--min_strand_len", type=int, default=3, help="shortest beta run that counts as a strand")
    return ap


def index_from_name(name):
    """'sample_prior_0003_recon.npy' -> 3: the last '_'-separated integer of the stem, a trailing '_recon' dropped."""
    stem = Path(name).stem
    if stem.endswith("_recon"):
        stem = stem[:-len("_recon")]
    for part in reversed(stem.split("_")):
        try:
            return int(part)
        except ValueError:
            pass
    return None


def load_manifest(path):
    """jsonl -> {index: record}; the index is the record's 'i', else the trailing integer of its 'indices_path' stem."""
    if not path:
        return {}
    p = Path(path)
    if not p.is_file():
        print(f"[warn] samples_manifest not found: {p}")
        return {}
    out = {}
    for line in p.read_text().splitlines():
        line = line.strip()
        if not line:
            continue
        try:
            rec = json.loads(line)
        except ValueError:
            continue
        idx = rec.get("i") if isinstance(rec, dict) else None
        if idx is None and isinstance(rec, dict):
            try:
                idx = int(Path(rec.get("indices_path", "")).stem.split("_")[-1])
            except (ValueError, TypeError):
                idx = None
        if idx is None:
            continue
        out[int(idx)] = rec
    print(f"[info] loaded {len(out)} records from {p}")
    return out


def merge_record(manifest, name, position, path, stats):
    """Manifest line of a kept curve: the original record of its index (or {'i': index or position}) + path + statistics."""
    idx = index_from_name(name)
    rec = dict(manifest[idx]) if idx is not None and idx in manifest else {"i": int(idx) if idx is not None else int(position)}
    rec["recon_path"] = str(path)
    rec["length_recon"] = int(stats["length_recon"])
    for k in RECORD_FLOATS:
        rec[k] = float(stats[k])
    for k in ("beta_total", "beta_max_run", "beta_in_sheet"):
        rec[k] = int(stats[k])
    rec["beta_sheet_fraction"] = float(stats["beta_sheet_fraction"])
    for k in ("beta_strands_total", "beta_strands_sheet", "beta_strands_isolated", "n_self_clash_pairs", "n_seg_clash_pairs"):
        rec[k] = int(stats[k])
    return rec


def pack_batches(curves, max_curves=BATCH_CURVES):
    """[(position, array [L, C])] -> [(positions, padded [n, Lmax, 3 or 6] fp32, lengths [n] int32)]: curves with SS channels
    (C >= 6, the first six kept) and without (xyz only) go to separate batches, each sorted by length."""
    out = []
    for with_ss in (False, True):
        group = [(pos, a) for pos, a in curves if (a.shape[1] >= 6) == with_ss]
        group.sort(key=lambda t: (t[1].shape[0], t[0]))
        ch = 6 if with_ss else 3
        for s in range(0, len(group), max_curves):
            part = group[s:s + max_curves]
            lmax = max(1, max(a.shape[0] for _, a in part))
            x = np.zeros((len(part), lmax, ch), np.float32)
            for r, (_, a) in enumerate(part):
                x[r, :a.shape[0]] = a[:, :ch]
            out.append(([pos for pos, _ in part], x, np.array([a.shape[0] for _, a in part], np.int32)))
    return out


def params_from_args(args):
    from vqvae_hip.curve_filter import FilterParams
    return FilterParams(min_length=args.min_length, max_length=args.max_length, min_pairwise_dist=args.min_pairwise_dist,
                        neighbor_exclude=args.neighbor_exclude, min_beta_run=args.min_beta_run,
                        min_beta_total=args.min_beta_total, beta_channel=args.beta_channel, max_curves=0,
                        min_beta_sheet_fraction=args.min_beta_sheet_fraction,
                        max_isolated_beta_strands=args.max_isolated_beta_strands, min_strand_len=args.min_strand_len)


def screen(arrays, params):
    """arrays: [(position, array)] -> {position: record dict} (one filter_curves call per packed batch)."""
    import torch
    from vqvae_hip.curve_filter import MAX_LEN, filter_curves
    from vqvae_hip.lib import VqhError
    stats, gpu = {}, []
    for pos, a in arrays:
        if a.shape[0] > MAX_LEN:
            if params.max_length > 0 and a.shape[0] > params.max_length:
                stats[pos] = {"reason": 2, "length_recon": a.shape[0]}
                continue
            raise VqhError(f"curve {pos}: length {a.shape[0]} > {MAX_LEN} supported by the GPU screen (set --max_length)")
        gpu.append((pos, a))
    for positions, x, lens in pack_batches(gpu):
        res = filter_curves(torch.from_numpy(x).cuda(), lengths=torch.from_numpy(lens).cuda(), params=params)
        for pos, rec in zip(positions, res.records()):
            stats[pos] = rec
    return stats


def main(argv=None):
    args = build_parser().parse_args(argv)
    recon_dir, out_dir = Path(args.recon_dir), Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    manifest = load_manifest(args.samples_manifest) if args.samples_manifest else {}
    files = sorted(recon_dir.glob("*.npy"))
    print(f"[info] found {len(files)} recon npy files in {recon_dir}")

    loaded = [np.load(str(p), allow_pickle=False) for p in files]
    usable = [(i, a) for i, a in enumerate(loaded) if a.ndim == 2 and a.shape[1] >= 3]
    stats = screen(usable, params_from_args(args)) if usable else {}

    counts = [0] * 9                       # total, kept, then reasons 1..7
    records = []
    for i, (path, curve) in enumerate(zip(files, loaded)):
        counts[0] += 1
        if i not in stats:
            continue                       # not a [L, >= 3] array: counted in the total only
        reason = int(stats[i]["reason"])
        if reason:
            counts[1 + reason] += 1
            continue
        records.append(merge_record(manifest, path.name, i, path, stats[i]))
        dst = out_dir / path.name
        if dst != path:
            np.save(str(dst), curve, allow_pickle=False)
        counts[1] += 1
        if args.max_curves > 0 and counts[1] >= args.max_curves:
            break
    for label, c in zip(SUMMARY_LABELS, counts):
        print(f"[summary] {label}: {c}")
    if args.filtered_manifest_out:
        mpath = Path(args.filtered_manifest_out)
        mpath.parent.mkdir(parents=True, exist_ok=True)
        with mpath.open("w") as f:
            for rec in records:
                f.write(json.dumps(rec) + "\n")
        print(f"[info] wrote filtered manifest with {len(records)} records to {mpath}")
    return counts, records


if __name__ == "__main__":
    main()
