# -*- coding: utf-8 -*-
"""Generates tests/golden/prior_export.npz from the REAL reference scripts/extract_code_indices.py, scripts/decode_with_vqvae.py
and models/vq_vae.py (build container only):

    python tests/golden/make_golden_export.py /path/to/reference

The reference modules are imported from their paths and run; only data is stored (arrays and JSON strings).

(a) Geometry: seeded 3.8 A random walks (gen_inputs.smooth_curve_batch, C = 6) and, for every (M, Q, L) case, the output of the
    reference's compute_latent_geometry_for_sample (ref32) and this file's own restatement of it evaluated in fp64 throughout
    (ref64, the arbiter of tests/parity_util.py).  Asserted: the restatement uses numpy's own `bounds`, its fp32 evaluation
    reproduces the reference function, and the closed form of the bounds ((long long)(t * (L / M)) in fp64) equals numpy's.
(b) Model: for SMALL_VQ and SMALL_RVQ, a ragged batch (B = 5, L = 33: different from latent_tokens, so the script tokenizes
    itself) through the reference in eval mode: tokenize_and_quantize (codes, lengths, z_e), indices_to_latent and
    decode_one_from_indices per sample, each also evaluated in fp64 (the reference model cast to double).  The oracle is run
    on the same inputs and the script aborts if it disagrees.  Admission (asserted, next seed otherwise): fp32 and fp64
    indices agree at every position and the smallest fp64 gap between the best and the second-best distance, relative to the
    best distance, is at least 1e-4 -- so the tests compare indices exactly and leave nothing out.
(c) The argparse flags of both scripts, read with ast."""
import ast
import copy
import importlib.util
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_inputs as G  # noqa: E402
from gen_inputs import O  # noqa: E402

GEO_CASES = ((48, 1, 208), (8, 3, 3), (8, 1, 1), (8, 1, 8), (32, 4, 350), (64, 1, 257), (32, 1, 33), (3, 1, 7), (12, 2, 100),
             (4, 2, 2))
GEO_SEED = 4100
MODEL_B, MODEL_L = 5, 33
MIN_GAP = 1e-4
MODEL_CASES = (("small_vq", G.SMALL_VQ, 610), ("small_rvq", G.SMALL_RVQ, 640))


def load_by_path(root, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cli_flags(path):
    """Every add_argument flag of a script with its default / type / required / choices / action, as plain values."""
    flags = {}
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument":
            kw = {k.arg: k.value for k in node.keywords}
            flags[ast.literal_eval(node.args[0])] = {
                "default": ast.literal_eval(kw["default"]) if "default" in kw else None,
                "type": kw["type"].id if "type" in kw else None,
                "required": ast.literal_eval(kw["required"]) if "required" in kw else False,
                "choices": ast.literal_eval(kw["choices"]) if "choices" in kw else None,
                "action": ast.literal_eval(kw["action"]) if "action" in kw else None}
    return flags


# ------------------------------------------------------------------------------------------------ (a) geometry
def closed_form_bounds(L, M):
    """What the kernel evaluates: one fp64 divide, one fp64 multiply, truncation; the end point is L itself."""
    step = float(L) / float(M)
    return np.asarray([int(float(t) * step) for t in range(M)] + [L], np.int64)


def geometry_restated(x, L, M, Q, dtype):
    """compute_latent_geometry_for_sample restated: x [L, C] -> [M*Q, C + 4], every operation in `dtype`."""
    x = np.asarray(x[:L], dtype)
    C = x.shape[1]
    bounds = np.linspace(0, L, M + 1, dtype=np.int64)
    out = np.zeros((M, C + 4), dtype)
    for t in range(M):
        s, e = int(bounds[t]), int(bounds[t + 1])
        if e <= s:
            e = min(L, s + 1)
        seg = x[s:e]
        if seg.shape[0] == 0:
            continue
        ctr = seg[:, :3].mean(axis=0)
        out[t, 0:3] = ctr
        if seg.shape[0] >= 2:
            vec = seg[-1, :3] - seg[0, :3]
            out[t, 3:6] = vec / dtype(np.linalg.norm(vec) + 1e-8)
        out[t, 6:C + 3] = seg[:, 3:].mean(axis=0)
        out[t, C + 3] = np.sqrt((((seg[:, :3] - ctr) ** 2).sum(axis=1)).mean())
    return np.repeat(out, Q, axis=0), bounds


def geometry_cases(X):
    out, curves, offs = {}, [], [0]
    for k, (M, Q, L) in enumerate(GEO_CASES):
        x, _ = G.smooth_curve_batch(1, L + 7, GEO_SEED + k)          # a slice of a longer walk: not centred on the origin
        x = x[0, 3:3 + L].numpy().astype(np.float32)
        ref32 = X.compute_latent_geometry_for_sample(coords=x[:, :3], ss=x[:, 3:], valid_len=L, num_codes=M * Q,
                                                     num_quantizers=Q)
        assert ref32.dtype == np.float32 and ref32.shape == (M * Q, 10), (ref32.shape, ref32.dtype)
        mine32, bounds = geometry_restated(x, L, M, Q, np.float32)
        ref64, bounds64 = geometry_restated(x, L, M, Q, np.float64)
        assert np.array_equal(bounds, np.linspace(0, L, M + 1, dtype=np.int64)) and np.array_equal(bounds, bounds64)
        assert np.array_equal(bounds, closed_form_bounds(L, M)), f"closed-form bounds differ from numpy's at M={M} L={L}"
        # the restatement is the reference function: same values up to the order of the fp32 operations
        assert np.abs(mine32.astype(np.float64) - ref32).max() <= 1e-4, f"restatement != reference for case {(M, Q, L)}"
        assert np.abs(ref64 - ref32).max() <= 1e-4 * max(1.0, np.abs(ref64).max()), f"fp64 restatement off for case {(M, Q, L)}"
        out[f"geo{k}_ref32"] = ref32
        out[f"geo{k}_ref64"] = ref64
        curves.append(x)
        offs.append(offs[-1] + L)
        print(f"[geo] case {(M, Q, L)}: max |ref32 - ref64| {np.abs(ref64 - ref32).max():.2e}, "
              f"one-point segments {int(np.sum(np.diff(bounds) <= 1))}")
    out["geo_cases"] = np.asarray(GEO_CASES, np.int32)
    out["geo_curves"] = np.concatenate(curves).astype(np.float32)
    out["geo_offsets"] = np.asarray(offs, np.int32)
    out["geo_seed"] = np.int32(GEO_SEED)
    return out


# ------------------------------------------------------------------------------------------------ (b) model
def fp64_gap(z_e, emb, Q, K_per):
    """fp64 nearest search with the direct (z - e)^2 form: (indices level-major, smallest relative gap best -> second)."""
    res = z_e.reshape(-1, z_e.shape[-1]).double()
    emb = emb.double()
    levels, gap = [], float("inf")
    for lv in range(Q):
        tab = emb[lv * K_per:(lv + 1) * K_per]
        d = ((res[:, None, :] - tab[None]) ** 2).sum(-1)
        top = torch.topk(d, 2, dim=1, largest=False)
        gap = min(gap, float(((top.values[:, 1] - top.values[:, 0]) / top.values[:, 0].clamp_min(1e-300)).min()))
        levels.append(top.indices[:, 0] + lv * K_per)
        res = res - tab[top.indices[:, 0]]
    return torch.cat(levels), gap


def model_case(name, cfg_kw, seed, X, Dm, RefVQVAE):
    Q, K_per = int(cfg_kw.get("num_quantizers", 1)), int(cfg_kw["codebook_size"])
    M, D = int(cfg_kw["latent_tokens"]), int(cfg_kw["code_dim"])
    while True:
        sd0 = G.model_state(cfg_kw, seed)
        x, mask = G.curve_batch(MODEL_B, MODEL_L, seed + 100, ragged=True)
        ref = RefVQVAE(**cfg_kw)
        ref.load_state_dict(sd0, strict=True)
        ref.eval()
        ref64 = copy.deepcopy(ref).double().eval()
        with torch.no_grad():
            codes, lengths, z_e = X.tokenize_and_quantize(ref, x, mask)
            codes64, lengths64, z_e64 = X.tokenize_and_quantize(ref64, x.double(), mask)
        idx64, gap = fp64_gap(z_e64, ref64.quantizer.embedding, Q, K_per)
        own = idx64.view(Q, MODEL_B, M).permute(1, 2, 0).reshape(MODEL_B, M * Q)
        assert torch.equal(own, codes64), f"{name}: the generator's fp64 search differs from the reference's"
        if torch.equal(codes, codes64) and gap >= MIN_GAP:
            break
        print(f"[skip] {name} seed {seed}: indices agree {torch.equal(codes, codes64)}, gap {gap:.2e}")
        seed += 1
    assert codes.shape == (MODEL_B, M * Q) and z_e.shape == (MODEL_B, M, D) and np.array_equal(lengths, lengths64)
    # the oracle on the same inputs (eval mode, no dropout)
    orc = O.OracleVQVAE({k: v.clone() for k, v in sd0.items()}, drop_scale=0.0, **cfg_kw)
    orc.training = False
    with torch.no_grad():
        hf, _, _ = orc.encode(x, mask)
        z_o = orc.tokenize_to_codes(hf, mask)
        idx_o = orc.quantize(z_o, do_ema_update=False)[2]
    o_codes = idx_o.reshape(Q, MODEL_B, M).permute(1, 2, 0).reshape(MODEL_B, M * Q) if Q > 1 else idx_o.reshape(MODEL_B, M)
    assert float((z_o - z_e).abs().max()) <= 2e-5 * max(1.0, float(z_e.abs().max())), f"{name}: oracle z_e != reference"
    assert torch.equal(o_codes, codes), f"{name}: oracle codes != reference"
    out = {"seed": np.int32(seed), "x_sum": np.float64(G.checksum(x)),
           "state_sum": np.float64(G.checksum(torch.cat([v.reshape(-1).double() for v in sd0.values() if v.is_floating_point()]))),
           "codes": codes.numpy().astype(np.int32), "lengths": np.asarray(lengths, np.int32), "z_e": z_e.numpy(),
           "z_e_err64": np.float64((z_e64 - z_e.double()).abs().max()), "min_gap64": np.float64(gap)}
    zq, zq_err, rec_err = [], 0.0, 0.0
    for b in range(MODEL_B):
        c_b, L_b = codes[b].numpy(), int(lengths[b])
        with torch.no_grad():
            z32, z64 = Dm.indices_to_latent(ref, c_b), Dm.indices_to_latent(ref64, c_b)
            r32, r64 = Dm.decode_one_from_indices(ref, c_b, L_b), Dm.decode_one_from_indices(ref64, c_b, L_b)
            r_o = orc.decode(z32, torch.ones(1, L_b, dtype=torch.bool))
        assert z32.shape == (1, M, D) and r32.shape == (1, L_b, 6)
        assert float((r_o - r32).abs().max()) <= 2e-5 * max(1.0, float(r32.abs().max())), f"{name}: oracle decode != reference"
        zq.append(z32[0].numpy())
        zq_err = max(zq_err, float((z64 - z32.double()).abs().max()))
        rec_err = max(rec_err, float((r64 - r32.double()).abs().max()))
        out[f"recon{b}"] = r32[0].numpy()
    out["z_q"] = np.stack(zq)
    out["z_q_err64"], out["recon_err64"] = np.float64(zq_err), np.float64(rec_err)
    print(f"[model] {name}: seed {seed}, lengths {list(map(int, lengths))}, min fp64 gap {gap:.2e}, "
          f"z_e err64 {float(out['z_e_err64']):.2e}, z_q err64 {zq_err:.2e}, recon err64 {rec_err:.2e}")
    return {f"{name}_{k}": v for k, v in out.items()}


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    if not os.path.isdir(root):
        print("reference tree not present: nothing to do (the fixture is committed)")
        return
    warnings.filterwarnings("ignore")
    torch.set_num_threads(8)
    X = load_by_path(root, os.path.join("scripts", "extract_code_indices.py"), "ref_extract_code_indices")
    Dm = load_by_path(root, os.path.join("scripts", "decode_with_vqvae.py"), "ref_decode_with_vqvae")
    RefVQVAE = load_by_path(root, os.path.join("models", "vq_vae.py"), "ref_models_vq_vae").VQVAE
    out = geometry_cases(X)
    for name, cfg_kw, seed in MODEL_CASES:
        out.update(model_case(name, cfg_kw, seed, X, Dm, RefVQVAE))
    out["model_cases"] = np.asarray([n for n, _, _ in MODEL_CASES])
    out["flags_extract"] = np.asarray(json.dumps(cli_flags(os.path.join(root, "scripts", "extract_code_indices.py"))))
    out["flags_decode"] = np.asarray(json.dumps(cli_flags(os.path.join(root, "scripts", "decode_with_vqvae.py"))))
    # the ten manifest keys of the extraction script, read from the dict literal in its main()
    src = ast.parse(open(os.path.join(root, "scripts", "extract_code_indices.py")).read())
    keys = next([ast.literal_eval(k) for k in n.value.keys] for n in ast.walk(src)
                if isinstance(n, ast.Assign) and isinstance(n.value, ast.Dict) and getattr(n.targets[0], "id", "") == "rec")
    assert len(keys) == 10, keys
    out["manifest_keys"] = np.asarray(keys)
    path = os.path.join(HERE, "prior_export.npz")
    np.savez_compressed(path, **out)
    print(f"wrote prior_export.npz: {len(GEO_CASES)} geometry cases, {len(MODEL_CASES)} models, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
