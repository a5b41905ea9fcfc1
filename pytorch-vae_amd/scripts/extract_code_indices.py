#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""Extract prior-training data from a trained VQVAE -- same flags, file names, layout and manifest keys as the reference's
scripts/extract_code_indices.py, with the per-batch work done on the GPU:

    python scripts/extract_code_indices.py --ckpt last.ckpt --yaml configs/stage2_vq.yaml --out_dir results/codes --split train

Per sample:
    rank0/indices_npy/<sid>.npy      flattened code indices [M*Q] in the order t0_l0, t0_l1, ..., t1_l0, ...
    rank0/ze_npy/<sid>_ze.npy        encoder latents z_e [M, D]
    rank0/geo_npy/<sid>_geo.npy      per-position geometry [M*Q, 10]: centre, unit direction, SS means, radius
    manifest_rank0.jsonl -> manifest.jsonl, extract_meta.json

Per batch: one VQVAE.encode_to_indices call and one vqvae_hip.prior_export.latent_geometry call; codes, each row's largest id,
z_e and geo are copied to the host once each; the host only slices and saves.  Runs as rank 0 of a world of 1."""
import argparse
import hashlib
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

MANIFEST_KEYS = ("id", "indices_path", "latent_path", "latent_len", "latent_tokens", "target_len", "dtype", "rank", "geo_path",
                 "geo_dim")


def build_parser():
    ap = argparse.ArgumentParser(description="Extract VQ code indices, encoder latents (z_e) and latent geometry for a prior.")
    ap.add_argument("--ckpt", type=str, required=True)
    ap.add_argument("--yaml", type=str, required=True)
    ap.add_argument("--out_dir", type=str, required=True)
    ap.add_argument("--split", type=str, default="train", choices=["train", "val", "test"])
    ap.add_argument("--max_batches", type=int, default=-1)
    ap.add_argument("--device", type=str, default="cuda")
    ap.add_argument("--num_workers", type=int, default=4)
    ap.add_argument("--indices_dtype", type=str, default="int32", choices=["int16", "int32"])
    ap.add_argument("--save_every", type=int, default=1)
    ap.add_argument("--pin_memory", action="store_true")
    ap.add_argument("--expect_latent_len", type=int, default=0)
    return ap


def file_sha256(path, chunk=1 << 20):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(chunk), b""):
            h.update(block)
    return h.hexdigest()


def load_model(ckpt_path, yaml_path, device):
    """-> (experiment, model on `device` in eval mode) with the checkpoint's weights (keys with or without 'model.')."""
    from experiment import build_experiment_from_yaml
    exp, _ = build_experiment_from_yaml(yaml_path)
    ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)
    state = ckpt.get("state_dict", ckpt)
    state = {(k[len("model."):] if k.startswith("model.") else k): v for k, v in state.items()}
    exp.model.load_state_dict(state, strict=False)
    exp.model.to(device).eval()
    return exp, exp.model


def split_loader(exp, split, num_workers, pin_memory):
    exp.data_params["num_workers"] = int(num_workers)
    exp.data_params["pin_memory"] = bool(pin_memory)
    exp.setup(stage="fit" if split in ("train", "val") else "test")
    if split == "train":
        return exp.train_dataloader()
    if split == "val":
        return exp.val_dataloader()
    if not hasattr(exp, "test_dataloader"):
        raise RuntimeError("the experiment defines no test_dataloader()")
    return exp.test_dataloader()


def extract_batch(model, x, mask):
    """One batch on the GPU -> host arrays (codes [B, M*Q] int32, row_max [B], z_e [B, M, D], geo [B, M*Q, G]): four copies."""
    from vqvae_hip import prior_export
    dev = model.quantizer.embedding.device
    xg, mg = x.to(dev, non_blocking=True), mask.to(dev, non_blocking=True)
    codes, z_e, row_max = model.encode_to_indices(xg, mg, return_row_max=True)
    geo = prior_export.latent_geometry(xg, mask=mg, M=model.latent_n_tokens, Q=model.quantizer.num_quantizers)
    return codes.cpu().numpy(), row_max.cpu().numpy(), z_e.cpu().numpy(), geo.cpu().numpy()


def main(argv=None):
    args = build_parser().parse_args(argv)
    rank, world = 0, 1
    device = torch.device(args.device)
    ckpt_path, yaml_path, out_dir = Path(args.ckpt).resolve(), Path(args.yaml).resolve(), Path(args.out_dir).resolve()
    out_dir.mkdir(parents=True, exist_ok=True)
    meta = {"ckpt_path": str(ckpt_path), "yaml_path": str(yaml_path),
            "ckpt_sha256": file_sha256(str(ckpt_path)) if ckpt_path.exists() else "", "dtype": args.indices_dtype,
            "split": args.split, "world_size": world}
    with open(out_dir / "extract_meta.json", "w") as f:
        json.dump(meta, f, indent=2)

    exp, model = load_model(str(ckpt_path), str(yaml_path), device)
    loader = split_loader(exp, args.split, args.num_workers, args.pin_memory)
    rank_dir = out_dir / f"rank{rank}"
    idx_dir, ze_dir, geo_dir = rank_dir / "indices_npy", rank_dir / "ze_npy", rank_dir / "geo_npy"
    for d in (idx_dir, ze_dir, geo_dir):
        d.mkdir(parents=True, exist_ok=True)
    part_path = out_dir / f"manifest_rank{rank}.jsonl"

    def flush(lines):
        if lines:
            with open(part_path, "a") as f:
                f.write("\n".join(lines) + "\n")
        return []

    lines, batches, saved = [], 0, 0
    for batch_idx, batch in enumerate(loader):
        if args.max_batches > 0 and batch_idx >= args.max_batches:
            break
        x, mask = (batch["x"], batch["mask"]) if isinstance(batch, dict) else (batch[0], batch[1])
        codes, row_max, z_e, geo = extract_batch(model, x, mask)
        lengths = mask.sum(dim=1).tolist()
        n_flat = int(codes.shape[1])
        if args.expect_latent_len > 0 and n_flat != int(args.expect_latent_len):
            print(f"[warn][rank{rank}] latent_len mismatch: got {n_flat}, expect {args.expect_latent_len}")
        for b in range(codes.shape[0]):
            small = args.indices_dtype == "int16" and int(row_max[b]) < np.iinfo(np.int16).max
            dtype = np.int16 if small else np.int32
            sid = f"rank{rank}_sample_{batches:06d}_{b:03d}"
            idx_path, ze_path, geo_path = idx_dir / f"{sid}.npy", ze_dir / f"{sid}_ze.npy", geo_dir / f"{sid}_geo.npy"
            np.save(str(idx_path), codes[b].astype(dtype, copy=False), allow_pickle=False)
            np.save(str(ze_path), z_e[b], allow_pickle=False)
            np.save(str(geo_path), geo[b], allow_pickle=False)
            rec = dict(zip(MANIFEST_KEYS, (sid, str(idx_path), str(ze_path), n_flat, int(z_e.shape[1]), int(lengths[b]),
                                           np.dtype(dtype).name, rank, str(geo_path), int(geo.shape[2]))))
            lines.append(json.dumps(rec))
            saved += 1
        batches += 1
        if batches % max(1, args.save_every) == 0:
            lines = flush(lines)
    flush(lines)

    merged = out_dir / "manifest.jsonl"
    with open(merged, "w") as fout:
        for r in range(world):
            part = out_dir / f"manifest_rank{r}.jsonl"
            if part.exists():
                with open(part) as fin:
                    fout.writelines(line.rstrip("\n") + "\n" for line in fin if line.strip())
    print(f"[rank0] merged manifest -> {merged}")
    print(f"[rank{rank}] Done. Batches: {batches}, samples saved: {saved}, manifest: {part_path}")
    print(f"[rank{rank}] Indices dir: {idx_dir}")
    print(f"[rank{rank}] z_e dir: {ze_dir}")


if __name__ == "__main__":
    main()
