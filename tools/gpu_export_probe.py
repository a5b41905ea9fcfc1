# -*- coding: utf-8 -*-
"""Measures the export path at stage2_vq.yaml's shape (B = 128, L <= 350, synthetic data): whole-batch extraction time and
samples/s (host clock around work that ends in the device-to-host copies), the three export kernels (device events over
back-to-back launches) and, for context, the same batch through the existing public calls plus a host geometry loop."""
import json
import os
import sys
import time

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-vae_amd")
for p in (ROOT, PKG):
    sys.path.insert(0, p)
from dataset import synthetic_curve_batch  # noqa: E402
from models import vae_models  # noqa: E402
from vqvae_hip import prior_export as X  # noqa: E402

B, L, REPS = 128, 350, 10
cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "stage2_vq.yaml")))["model_params"]
cfg.update(print_init=False, codebook_init_path=None)
torch.manual_seed(0)
m = vae_models["VQVAE"](**cfg).to("cuda:0").eval()
M, Q, D = m.latent_n_tokens, m.quantizer.num_quantizers, m.code_dim
batches = [synthetic_curve_batch(B, L, 100 + i, ragged=True) for i in range(4)]


def host_geometry(x, L_, M_, Q_):
    x = x[:L_]
    bounds = np.linspace(0, L_, M_ + 1, dtype=np.int64)
    out = np.zeros((M_, 10), np.float32)
    for t in range(M_):
        s, e = int(bounds[t]), int(bounds[t + 1])
        if e <= s:
            e = min(L_, s + 1)
        seg = x[s:e]
        if seg.shape[0] == 0:
            continue
        ctr = seg[:, :3].mean(axis=0)
        out[t, :3] = ctr
        if seg.shape[0] >= 2:
            v = seg[-1, :3] - seg[0, :3]
            out[t, 3:6] = v / float(np.linalg.norm(v) + 1e-8)
        out[t, 6:9] = seg[:, 3:].mean(axis=0)
        out[t, 9] = np.sqrt(((seg[:, :3] - ctr) ** 2).sum(axis=1).mean())
    return np.repeat(out, Q_, axis=0)


def new_path(x, mask):
    xg, mg = x.cuda(non_blocking=True), mask.cuda(non_blocking=True)
    codes, z_e, row_max = m.encode_to_indices(xg, mg, return_row_max=True)
    geo = X.latent_geometry(xg, mask=mg, M=M, Q=Q)
    return codes.cpu().numpy(), row_max.cpu().numpy(), z_e.cpu().numpy(), geo.cpu().numpy()


def old_path(x, mask, with_geometry=True):
    xg, mg = x.cuda(non_blocking=True), mask.cuda(non_blocking=True)
    hf = m.encode(xg, mg)[0]
    z_e = m._tokenize_to_codes(hf, mg)
    idx = m.quantizer(z_e, do_ema_update=False, allow_reinit=False)[2]
    codes = idx.view(Q, B, M).permute(1, 2, 0).reshape(B, M * Q).cpu().numpy()
    ze = z_e.cpu().numpy()
    geo = None
    if with_geometry:
        xn, lens = x.numpy(), mask.sum(1).tolist()
        geo = np.stack([host_geometry(xn[b], int(lens[b]), M, Q) for b in range(B)])
    return codes, ze, geo


def clock(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        fn(*batches[i % len(batches)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def events(fn, n=200):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3          # microseconds per call


res = {"shape": {"B": B, "L": L, "M": M, "Q": Q, "D": D, "K_per": m.quantizer.K_per, "hidden": m.hidden_dim}}
# same results first (codes exact, geometry to fp32 round-off)
c_new, _, ze_new, geo_new = new_path(*batches[0])
c_old, ze_old, geo_old = old_path(*batches[0])
res["codes_equal"] = bool(np.array_equal(c_new, c_old))
res["codes_mismatch_fraction"] = float((c_new != c_old).mean())
res["z_e_max_abs_diff"] = float(np.abs(ze_new - ze_old).max())
res["geo_max_abs_diff_vs_host_fp32_loop"] = float(np.abs(geo_new - geo_old).max())
for i in range(len(batches)):                   # warm every shape
    new_path(*batches[i]); old_path(*batches[i], with_geometry=False)
t_new = [clock(new_path, REPS) for _ in range(3)]
t_old = [clock(old_path, REPS) for _ in range(3)]
t_old_nogeo = [clock(lambda x, k: old_path(x, k, False), REPS) for _ in range(3)]
res["new_seconds_per_batch"] = t_new
res["old_seconds_per_batch"] = t_old
res["old_without_host_geometry_seconds_per_batch"] = t_old_nogeo
res["new_samples_per_s"] = B / min(t_new)
res["old_samples_per_s"] = B / min(t_old)
# the three kernels alone
xg, mg = batches[0][0].cuda(), batches[0][1].cuda()
lens = mg.sum(1).to(torch.int32)
idx = torch.randint(0, m.quantizer.K, (Q * B * M,), device="cuda")
codes, _ = X.pack_codes(idx, Q, B, M)
emb = m.quantizer.embedding
res["us_latent_geometry"] = events(lambda: X.latent_geometry(xg, lengths=lens, M=M, Q=Q))
res["us_codes_pack"] = events(lambda: X.pack_codes(idx, Q, B, M))
res["us_codes_to_latent"] = events(lambda: X.codes_to_latent_async(codes, emb, Q))
res["codes_to_latent_bytes"] = int(B * M * (Q + 1) * D * 4)
res["us_host_geometry_loop"] = 1e6 * min(
    (lambda t0: (np.stack([host_geometry(batches[0][0].numpy()[b], int(lens[b]), M, Q) for b in range(B)]), time.perf_counter() - t0)[1])(
        time.perf_counter()) for _ in range(3))
print(json.dumps(res, indent=1))
