# -*- coding: utf-8 -*-
"""-m gpu: the export of prior-training data (csrc/export.hip through vqvae_hip.prior_export, VQVAE.encode_to_indices /
decode_from_indices and the two CLIs under scripts/) against tests/golden/prior_export.npz, which
tests/golden/make_golden_export.py recorded from the reference's scripts/extract_code_indices.py, scripts/decode_with_vqvae.py
and models/vq_vae.py.  Code indices are compared exactly with nothing left out (the fixture admits only states whose fp64
best / second-best distance gap is >= 1e-4 relative); floats under the rule of tests/parity_util.py:
|got - ref32| <= max(1e-5 |ref32|, 4 |ref32 - ref64|) (+ its 1e-8 floor)."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import yaml

import gen_inputs as G
from conftest import PKG, load_golden
from parity_util import assert_tensor, scalar_tol

pytestmark = pytest.mark.gpu

WEIGHTS = dict(G.BASE_LOSS_WEIGHTS, xyz_tv_lambda=0.001, bond_length_weight=0.01)
CFGS = {"small_vq": G.SMALL_VQ, "small_rvq": G.SMALL_RVQ}


@pytest.fixture(scope="module")
def fx():
    return load_golden("prior_export")


@pytest.fixture(scope="module")
def X():
    from vqvae_hip import prior_export
    return prior_export


def _model(fx, name, train=False):
    from models import vae_models
    cfg = CFGS[name]
    m = vae_models["VQVAE"](**cfg)
    m.load_state_dict(G.model_state(cfg, int(fx[f"{name}_seed"])), strict=True)
    m = m.to("cuda:0")
    return m.train() if train else m.eval()


def _batch(fx, name):
    x, mask = G.curve_batch(5, 33, int(fx[f"{name}_seed"]) + 100, ragged=True)
    assert abs(G.checksum(x) - float(fx[f"{name}_x_sum"])) <= 1e-9 * max(1.0, abs(float(fx[f"{name}_x_sum"]))), "input drift"
    return x.cuda(), mask.cuda()


@pytest.fixture(scope="module")
def models(fx):
    return {name: _model(fx, name) for name in CFGS}


# ------------------------------------------------------------------------------------------------ latent_geometry
def test_latent_geometry_fixture_parity(fx, X):
    """Every fixture case; cases of equal (M, Q) share one padded batch, NaN in every padded position."""
    cases, offs = fx["geo_cases"].tolist(), fx["geo_offsets"]
    Lpad = max(L for _, _, L in cases) + 3
    for M, Q in sorted({(M, Q) for M, Q, _ in cases}):
        ks = [k for k, c in enumerate(cases) if (c[0], c[1]) == (M, Q)]
        x = torch.full((len(ks), Lpad, 6), float("nan"))
        lens = []
        for r, k in enumerate(ks):
            L = cases[k][2]
            x[r, :L] = torch.from_numpy(fx["geo_curves"][offs[k]:offs[k + 1]])
            lens.append(L)
        geo = X.latent_geometry(x.cuda(), lengths=torch.tensor(lens), M=M, Q=Q)
        assert geo.shape == (len(ks), M * Q, 10) and geo.dtype == torch.float32
        got = geo.cpu().numpy()
        for r, k in enumerate(ks):
            r32, r64 = fx[f"geo{k}_ref32"], fx[f"geo{k}_ref64"]
            g = got[r].astype(np.float64)
            assert np.isfinite(g).all(), cases[k]
            for i in np.ndindex(*r32.shape):
                tol = scalar_tol(r32[i], r64[i])
                assert abs(g[i] - r32[i]) <= tol, f"case {cases[k]} row {i[0]} col {i[1]}: {g[i]!r} vs {r32[i]!r} (tol {tol:.3e})"
            zero = (r32 == 0) & (r64 == 0)                       # what the reference defines as exactly zero
            assert (got[r][zero] == 0).all(), cases[k]
            rep = got[r].reshape(M, Q, 10)
            assert np.array_equal(rep.view(np.uint32), np.repeat(rep[:, :1], Q, 1).view(np.uint32)), cases[k]


def test_latent_geometry_empty_curve_mask_and_long_curves(fx, X):
    x = torch.full((3, 40, 6), float("nan"))
    x[1, :9] = torch.from_numpy(fx["geo_curves"][:9])
    x[2, :40] = torch.from_numpy(fx["geo_curves"][:40])
    lens = torch.tensor([0, 9, 40])
    geo = X.latent_geometry(x.cuda(), lengths=lens, M=8, Q=2)
    assert (geo[0] == 0).all() and torch.isfinite(geo).all()                  # L = 0: every row is zeros
    mask = torch.arange(40)[None, :] < lens[:, None]
    assert torch.equal(geo, X.latent_geometry(x.cuda(), mask=mask.cuda(), M=8, Q=2))
    assert torch.equal(geo[2:], X.latent_geometry(x[2:].cuda(), M=8, Q=2))    # no lengths: every curve is Lmax long
    # a curve too long for the LDS staging takes the direct-read path: same numbers as the staged one
    k = fx["geo_cases"].tolist().index([32, 4, 350])
    o = int(fx["geo_offsets"][k])
    cur = torch.from_numpy(fx["geo_curves"][o:o + 350])
    short = X.latent_geometry(cur[None].cuda(), M=32, Q=4)
    long = torch.full((1, 3000, 6), float("nan"))
    long[0, :350] = cur
    assert torch.equal(short, X.latent_geometry(long.cuda(), lengths=torch.tensor([350]), M=32, Q=4))


# ------------------------------------------------------------------------------------------------ pack_codes / codes_to_latent
@pytest.mark.parametrize("Q,B,M", [(1, 5, 7), (3, 5, 7), (4, 3, 33), (3, 2, 300)])
def test_pack_codes_is_the_reference_permutation(X, Q, B, M):
    assert (B * M) % 64
    g = torch.Generator().manual_seed(Q * 100 + M)
    idx = torch.randint(0, 40000, (Q * B * M,), generator=g)
    codes, row_max = X.pack_codes(idx.cuda(), Q, B, M)
    want = idx.view(Q, B, M).permute(1, 2, 0).reshape(B, M * Q)              # _ensure_batch_first_2d
    assert codes.dtype == torch.int32 and row_max.dtype == torch.int32
    assert torch.equal(codes.cpu().long(), want)
    assert torch.equal(row_max.cpu().long(), want.max(1).values)


def test_codes_to_latent(fx, X):
    from vqvae_hip.lib import VqhError
    g = torch.Generator().manual_seed(5)
    E = torch.randn(50, 16, generator=g).cuda()
    codes = torch.randint(0, 50, (3, 11), generator=g).cuda()
    z = X.codes_to_latent(codes, E, 1)
    assert z.shape == (3, 11, 16) and torch.equal(z, E[codes.long()])         # Q = 1: the codebook rows, bit for bit
    # Q = 3 against the reference's indices_to_latent (fixture), through the model's own codebook
    sd = G.model_state(G.SMALL_RVQ, int(fx["small_rvq_seed"]))
    emb = sd["quantizer.embedding"].cuda()
    z3 = X.codes_to_latent(torch.from_numpy(fx["small_rvq_codes"]).cuda(), emb, 3)
    assert_tensor(z3, fx["small_rvq_z_q"], float(fx["small_rvq_z_q_err64"]), "z_q (Q = 3)")
    # strided codebook views: lde > D on the 16-byte path (lde = 20) and on the scalar path (lde = 17, D = 15)
    big = torch.full((50, 20), float("nan"), device="cuda")
    big[:, :16] = E
    assert torch.equal(X.codes_to_latent(codes, big[:, :16], 1), z)
    odd = torch.full((50, 17), float("nan"), device="cuda")
    odd[:, :15] = E[:, :15]
    c2 = codes[:, :10]
    want = E[c2.long()][..., :15].reshape(3, 5, 2, 15)
    assert torch.equal(X.codes_to_latent(c2, odd[:, :15], 2), want[:, :, 0] + want[:, :, 1])
    # ids outside 0..K-1: VqhError naming the count; the rows stay finite (the bad id contributes zeros)
    bad = codes.clone()
    bad[0, 3], bad[2, 10] = 50, -1
    with pytest.raises(VqhError, match=r"\b2 code id"):
        X.codes_to_latent(bad, E, 1)
    zb, n_bad = X.codes_to_latent_async(bad, E, 1)
    assert int(n_bad.item()) == 2 and torch.isfinite(zb).all() and (zb[0, 3] == 0).all() and (zb[2, 10] == 0).all()
    keep = torch.ones(3, 11, dtype=torch.bool, device="cuda")
    keep[0, 3] = keep[2, 10] = False
    assert torch.equal(zb[keep], z[keep])


# ------------------------------------------------------------------------------------------------ the model methods
def _frozen(m):
    eng, q = m._engine(), m.quantizer
    return [t.clone() for t in (q.embedding, q.ema_embedding, q.ema_cluster_size, eng.flat_m, eng.flat_v, eng.rng, eng.flat_p)] \
        + [torch.tensor(eng.opt_step)]


@pytest.mark.parametrize("name", ["small_vq", "small_rvq"])
def test_encode_to_indices_matches_the_reference_and_leaves_state_alone(fx, models, name):
    m = models[name]
    x, mask = _batch(fx, name)
    before = _frozen(m)
    codes, z_e = m.encode_to_indices(x, mask)
    assert codes.dtype == torch.int32 and codes.shape == fx[f"{name}_codes"].shape and z_e.dtype == torch.float32
    assert torch.equal(codes.cpu(), torch.from_numpy(fx[f"{name}_codes"]))
    assert_tensor(z_e, fx[f"{name}_z_e"], float(fx[f"{name}_z_e_err64"]), f"{name} z_e")
    m.train()                                         # dropout stays off whatever self.training says
    try:
        codes_t, z_e_t, row_max = m.encode_to_indices(x, mask, return_row_max=True)
    finally:
        m.eval()
    assert torch.equal(codes_t, codes) and torch.equal(z_e_t, z_e) and torch.equal(row_max.long(), codes.max(1).values.long())
    for a, b in zip(before, _frozen(m)):
        assert torch.equal(a, b)


def test_encode_to_indices_needs_a_quantizer():
    from models import vae_models
    from vqvae_hip.lib import VqhError
    m = vae_models["VQVAE"](**G.SMALL_AE).to("cuda:0").eval()
    x, mask = G.curve_batch(2, 12, 3)
    with pytest.raises(VqhError):
        m.encode_to_indices(x.cuda(), mask.cuda())
    with pytest.raises(VqhError):
        m.decode_from_indices(torch.zeros(2, 8, dtype=torch.int32))


@pytest.mark.parametrize("name", ["small_vq", "small_rvq"])
def test_encode_to_indices_between_forward_and_backward(fx, name):
    x, mask = _batch(fx, name)
    x2, mask2 = G.curve_batch(3, 20, 9, ragged=True)

    def step(interleave):
        m = _model(fx, name, train=True)
        m.training_steps = 1
        m._engine().drop_scale = 0.0
        out = m(x, mask)
        if interleave:
            m.encode_to_indices(x, mask)              # same shape as the step in flight, then another one
            m.encode_to_indices(x2.cuda(), mask2.cuda())
        ld = m.loss_function(*out, **WEIGHTS)
        ld["loss"].backward()
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in ld.items()}, m._engine().flat_g.clone(), m.quantizer.embedding.clone()
    ld_a, g_a, e_a = step(False)
    ld_b, g_b, e_b = step(True)
    assert ld_a.keys() == ld_b.keys()
    for k in ld_a:
        assert torch.equal(ld_a[k], ld_b[k]), k
    assert torch.equal(g_a, g_b) and torch.equal(e_a, e_b) and float(g_a.abs().sum()) > 0


@pytest.mark.parametrize("name", ["small_vq", "small_rvq"])
def test_decode_from_indices(fx, models, name):
    m = models[name]
    codes = torch.from_numpy(fx[f"{name}_codes"]).cuda()
    lens = fx[f"{name}_lengths"].tolist()
    err64 = float(fx[f"{name}_recon_err64"])
    batched = m.decode_from_indices(codes, target_len=lens)
    assert batched.shape == (5, max(lens), 6)
    as_tensor = m.decode_from_indices(codes, target_len=torch.tensor(lens))
    assert torch.equal(as_tensor, batched)
    for b, L in enumerate(lens):
        one = m.decode_from_indices(codes[b:b + 1], target_len=L)
        assert one.shape == (1, L, 6)
        assert_tensor(one[0], fx[f"{name}_recon{b}"], err64, f"{name} single-record decode {b}")
        assert_tensor(batched[b, :L], fx[f"{name}_recon{b}"], err64, f"{name} batched decode {b}")
        assert_tensor(batched[b, :L], one[0], err64, f"{name} batched vs single {b}")
    flat = m.decode_from_indices(codes[1].cpu().long(), target_len=lens[1])         # 1-D codes, int target_len
    assert flat.shape == (1, lens[1], 6)
    assert torch.equal(flat, m.decode_from_indices(codes[1:2], target_len=lens[1]))


# ------------------------------------------------------------------------------------------------ the CLIs
def _script(name):
    spec = importlib.util.spec_from_file_location("vqh_scripts_" + name, os.path.join(PKG, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_round_trip(fx, X, models, tmp_path, capsys):
    from dataset import SyntheticCurveDataset, pad_collate
    tmp = str(tmp_path)
    name, mp = "small_rvq", dict(G.SMALL_RVQ)
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "stage2_vq.yaml")))
    cfg["model_params"] = dict(mp, name="export-round-trip")
    syn = {"n": 16, "n_val": 7, "max_len": 40, "min_len": 9, "seed": 3}
    cfg["data_params"].update(train_batch_size=4, val_batch_size=4, num_workers=0, pin_memory=False, synthetic=syn)
    ypath, ckpt = os.path.join(tmp, "m.yaml"), os.path.join(tmp, "m.ckpt")
    yaml.safe_dump(cfg, open(ypath, "w"))
    sd = G.model_state(mp, int(fx[f"{name}_seed"]))
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}}, ckpt)
    out = os.path.join(tmp, "codes")
    _script("extract_code_indices").main(["--ckpt", ckpt, "--yaml", ypath, "--out_dir", out, "--split", "val", "--num_workers", "0",
                                          "--indices_dtype", "int16", "--save_every", "2"])
    recs = [json.loads(line) for line in open(os.path.join(out, "manifest.jsonl"))]
    assert open(os.path.join(out, "manifest_rank0.jsonl")).read() == open(os.path.join(out, "manifest.jsonl")).read()
    meta = json.load(open(os.path.join(out, "extract_meta.json")))
    assert meta["split"] == "val" and meta["world_size"] == 1 and meta["dtype"] == "int16" and len(meta["ckpt_sha256"]) == 64
    ds = SyntheticCurveDataset(7, 40, 9, seed=4)                              # the experiment's validation set
    m, M, Q = models[name], 8, 3
    assert [r["id"] for r in recs] == [f"rank0_sample_{k // 4:06d}_{k % 4:03d}" for k in range(7)]
    all_codes = []
    for k0 in (0, 4):
        x, mask = pad_collate([ds[i] for i in range(k0, min(k0 + 4, 7))])
        codes, z_e = m.encode_to_indices(x.cuda(), mask.cuda())
        geo = X.latent_geometry(x.cuda(), mask=mask.cuda(), M=M, Q=Q)
        for b in range(x.shape[0]):
            r = recs[k0 + b]
            assert list(r.keys()) == [str(k) for k in fx["manifest_keys"]]
            sid = r["id"]
            assert r["indices_path"] == os.path.join(out, "rank0", "indices_npy", sid + ".npy")
            assert r["latent_path"] == os.path.join(out, "rank0", "ze_npy", sid + "_ze.npy")
            assert r["geo_path"] == os.path.join(out, "rank0", "geo_npy", sid + "_geo.npy")
            assert (r["latent_len"], r["latent_tokens"], r["target_len"], r["dtype"], r["rank"], r["geo_dim"]) == \
                (M * Q, M, int(mask[b].sum()), "int16", 0, 10)
            ci, ze, ge = np.load(r["indices_path"]), np.load(r["latent_path"]), np.load(r["geo_path"])
            assert ci.dtype == np.int16 and ci.shape == (M * Q,) and np.array_equal(ci, codes[b].cpu().numpy())
            assert ze.dtype == np.float32 and ze.shape == (M, 16) and np.array_equal(ze, z_e[b].cpu().numpy())
            assert ge.dtype == np.float32 and ge.shape == (M * Q, 10) and np.array_equal(ge, geo[b].cpu().numpy())
            all_codes.append(codes[b])
    # decode the manifest with latent_path removed: outputs equal decode_from_indices on the same codes
    stripped = os.path.join(tmp, "indices_only.jsonl")
    with open(stripped, "w") as f:
        for r in recs:
            f.write(json.dumps({k: v for k, v in r.items() if k != "latent_path"}) + "\n")
    dec = os.path.join(tmp, "decoded")
    _script("decode_with_vqvae").main(["--vq_ckpt", ckpt, "--vq_yaml", ypath, "--samples_manifest", stripped, "--out_dir", dec,
                                       "--batch_size", "3"])
    assert "Decoded 7 sequences" in capsys.readouterr().out
    err64 = float(fx[f"{name}_recon_err64"])
    for r, c in zip(recs, all_codes):
        got = np.load(os.path.join(dec, r["id"] + "_recon.npy"))
        assert got.dtype == np.float32 and got.shape == (r["target_len"], 6)
        want = m.decode_from_indices(c, target_len=r["target_len"])[0]
        assert_tensor(got, want, err64, f"decoded {r['id']}")
    # with latent_path present the continuous latent is decoded as it is
    dec2 = os.path.join(tmp, "decoded_latent")
    _script("decode_with_vqvae").main(["--vq_ckpt", ckpt, "--vq_yaml", ypath, "--samples_manifest",
                                       os.path.join(out, "manifest.jsonl"), "--out_dir", dec2, "--limit", "2"])
    for r in recs[:2]:
        got = np.load(os.path.join(dec2, r["id"] + "_ze_recon.npy"))
        ze = torch.from_numpy(np.load(r["latent_path"])).cuda()[None]
        want = m.decode(ze, mask=torch.ones(1, r["target_len"], dtype=torch.bool, device="cuda"))[0]
        assert_tensor(got, want, err64, f"latent-decoded {r['id']}")
