#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""Decode code indices (or continuous latents) to curves with a trained VQVAE -- same flags, manifest fields and output names
as the reference's scripts/decode_with_vqvae.py, decoded in batches on the GPU:

    python scripts/decode_with_vqvae.py --vq_ckpt last.ckpt --vq_yaml configs/stage2_vq.yaml \\
        --samples_manifest results/prior_samples/manifest.jsonl --out_dir results/decoded_npy

A manifest record carries `target_len` (or `length`) and either `latent_path` (a continuous [N, D] latent, decoded as it is) or
`indices_path` (flattened codes [M*Q], t0_l0, t0_l1, ...: the residual levels are summed); `latent_path` wins when both are
present, as in the reference.  The output is <stem>_recon.npy of shape [target_len, 6].  Records are grouped by kind and by
the engine's length bucket of their target length and decoded --batch_size at a time, each sample under its own prefix mask."""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)


def build_parser():
    ap = argparse.ArgumentParser(description="Decode code indices or latents to curves with a trained VQVAE.")
    ap.add_argument("--vq_ckpt", type=str, required=True)
    ap.add_argument("--vq_yaml", type=str, required=True)
    ap.add_argument("--samples_manifest", type=str, required=True)
    ap.add_argument("--out_dir", type=str, required=True)
    ap.add_argument("--device", type=str, default="cuda")
    ap.add_argument("--limit", type=int, default=0)
    ap.add_argument("--check_latent_len", type=int, default=0)
    ap.add_argument("--batch_size", type=int, default=64, help="records decoded per call")
    return ap


def load_model(ckpt_path, yaml_path, device):
    from experiment import build_experiment_from_yaml
    exp, _ = build_experiment_from_yaml(yaml_path)
    ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)
    state = ckpt.get("state_dict", ckpt)
    state = {(k[len("model."):] if k.startswith("model.") else k): v for k, v in state.items()}
    exp.model.load_state_dict(state, strict=False)
    return exp.model.to(device).eval()


def read_records(manifest, limit, check_latent_len):
    """-> [(kind, array, target_len, stem)] of the usable records, in manifest order; the rest is reported like the reference."""
    with open(manifest) as f:
        records = [json.loads(line) for line in f if line.strip()]
    if limit > 0:
        records = records[:limit]
    out = []
    for r in records:
        tlen = int(r["target_len"]) if "target_len" in r else int(r.get("length", 0))
        if tlen <= 0:
            print(f"[warn] invalid target_len for record id={r.get('id', 'NA')}")
            continue
        kind, path = ("latent", r.get("latent_path", "")) if r.get("latent_path", "") else ("indices", r.get("indices_path", ""))
        if not path:
            print(f"[warn] record id={r.get('id', 'NA')} has neither latent_path nor indices_path")
            continue
        path = Path(path)
        if not path.exists():
            print(f"[warn] missing {kind}: {path}")
            continue
        arr = np.load(str(path), allow_pickle=False)
        if kind == "latent" and arr.ndim == 3 and arr.shape[0] == 1:
            arr = arr[0]
        if arr.ndim != (2 if kind == "latent" else 1):
            print(f"[warn] {kind} of shape {arr.shape} at {path}: skipped")
            continue
        if check_latent_len > 0 and int(arr.shape[0]) != int(check_latent_len):
            print(f"[warn] latent_len mismatch {arr.shape[0]} != {check_latent_len} at {path}")
        out.append((kind, arr, tlen, path.stem))
    return out


def decode_records(model, items, batch_size):
    """Yields (stem, recon [target_len, 6] on the host).  Groups: (kind, array shape, length bucket) -> chunks of batch_size."""
    eng = model._engine()
    dev = model.head_xyz.weight.device
    groups = {}
    for kind, arr, tlen, stem in items:
        if tlen > model.max_seq_len:
            print(f"[warn] target_len {tlen} > max_seq_len {model.max_seq_len} for {stem}: skipped")
            continue
        groups.setdefault((kind, arr.shape, eng.bucket_len(tlen)), []).append((arr, tlen, stem))
    for (kind, _, Lb), recs in groups.items():
        for o in range(0, len(recs), batch_size):
            chunk = recs[o:o + batch_size]
            lens = torch.tensor([t for _, t, _ in chunk])
            mask = (torch.arange(Lb)[None, :] < lens[:, None]).to(dev)
            stack = torch.from_numpy(np.stack([a for a, _, _ in chunk]))
            if kind == "latent":
                rec = model.decode(stack.float().to(dev), mask=mask)
            else:
                rec = model.decode_from_indices(stack.to(torch.int32).to(dev), mask=mask)
            rec = rec.cpu().numpy()
            for b, (_, tlen, stem) in enumerate(chunk):
                yield stem, rec[b, :tlen]


def main(argv=None):
    args = build_parser().parse_args(argv)
    model = load_model(args.vq_ckpt, args.vq_yaml, torch.device(args.device))
    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    items = read_records(args.samples_manifest, args.limit, args.check_latent_len)
    n_ok = 0
    for stem, recon in decode_records(model, items, max(1, int(args.batch_size))):
        np.save(str(out_dir / (stem + "_recon.npy")), np.ascontiguousarray(recon), allow_pickle=False)
        n_ok += 1
    print(f"Decoded {n_ok} sequences -> {out_dir}")


if __name__ == "__main__":
    main()
