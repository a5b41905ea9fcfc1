# -*- coding: utf-8 -*-
"""-m gpu: the curve validity screen (csrc/filter.hip through vqvae_hip.curve_filter, VQVAE.sample_filtered and the
prior/filter_curves.py CLI) against tests/golden/curve_filter.npz, which tests/golden/make_golden_filter.py recorded from the
reference's own functions and main().  Integer columns are compared exactly with no case left out (the fixture admits only
curves whose compared quantities stay 1e-4 relative away from every threshold); float columns under the rule of
tests/parity_util.py: |got - ref32| <= max(1e-5 |ref32|, 4 |ref32 - ref64|) (+ its 1e-8 floor)."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import gen_inputs as G
from conftest import PKG, load_golden
from parity_util import scalar_tol

pytestmark = pytest.mark.gpu

LPAD = 350
# walks (make_golden_filter.walk) whose fp64 pair counts are the same at thresholds t (1 - 1e-5) and t (1 + 1e-5): checked on
# the CPU when the test was written, asserted again below, so the sandwich is an equality with nothing excluded
SANDWICH = ((350, (3003, 3006, 3007, 3009, 3010, 3018, 3019, 3021)), (257, (3030, 3031)))
SANDWICH_EPS = 1e-5


@pytest.fixture(scope="module")
def fx():
    return load_golden("curve_filter")


@pytest.fixture(scope="module")
def F():
    from vqvae_hip import curve_filter
    return curve_filter


def _cli():
    spec = importlib.util.spec_from_file_location("vqh_prior_filter_curves", os.path.join(PKG, "prior", "filter_curves.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _split(fx):
    out, o = [], 0
    for L, c in zip(fx["lengths"], fx["channels"]):
        out.append(np.ascontiguousarray(fx["curves"][o:o + L, :c]))
        o += L
    return out


@pytest.fixture(scope="module")
def batch(fx):
    """All fixture curves in one batch padded to 350, NaN in every padded position and in the channels a curve lacks."""
    curves = _split(fx)
    x = torch.full((len(curves), LPAD, 6), float("nan"))
    for k, c in enumerate(curves):
        x[k, :c.shape[0], :c.shape[1]] = torch.from_numpy(c)
    return x.cuda(), torch.from_numpy(fx["lengths"]).cuda()


def _params(F, fx, p, **over):
    return F.params_from_dict(dict(json.loads(str(fx["param_sets"][p])), **over))


def _assert_floats(got, r32, r64, cols, what):
    got = np.asarray(got, np.float64)
    for idx in np.ndindex(*r32.shape):
        tol = scalar_tol(r32[idx], r64[idx])
        assert abs(got[idx] - r32[idx]) <= tol, (f"{what} row {idx[0]} {cols[idx[-1]]}: got {got[idx]!r} vs {r32[idx]!r} "
                                                 f"(ref64 {r64[idx]!r}, tol {tol:.3e})")


@pytest.mark.parametrize("p", [0, 1, 2])
def test_fixture_parity(F, fx, batch, p):
    x, lens = batch
    res = F.filter_curves(x, lengths=lens, params=_params(F, fx, p))
    ints = res.ints.cpu().numpy()
    bad = np.argwhere(ints != fx["ints"][p])
    assert bad.size == 0, [(str(fx["names"][r]), F.INT_COLUMNS[c], int(ints[r, c]), int(fx["ints"][p][r, c])) for r, c in bad[:10]]
    _assert_floats(res.floats.cpu().numpy(), fx["f32"][p], fx["f64"][p], F.FLOAT_COLUMNS, f"set {p}")
    kept = fx[f"main{p}_kept"]
    assert int(res.n_keep.item()) == len(kept)
    keep_idx = res.keep_idx.cpu().numpy()
    assert np.array_equal(keep_idx[:len(kept)], kept) and (keep_idx[len(kept):] == -1).all()
    assert res.ints.dtype == torch.int32 and res.keep_idx.dtype == torch.int32 and res.floats.dtype == torch.float32


def test_prefix_mask_and_default_lengths(F, fx, batch):
    x, lens = batch
    a = F.filter_curves(x, lengths=lens, params=_params(F, fx, 1))
    mask = torch.arange(LPAD, device=x.device)[None, :] < lens[:, None]
    b = F.filter_curves(x, mask=mask, params=_params(F, fx, 1))
    assert torch.equal(a.ints, b.ints) and torch.equal(a.floats, b.floats) and torch.equal(a.keep_idx, b.keep_idx)
    full = [k for k, L in enumerate(fx["lengths"]) if L == LPAD]
    c = F.filter_curves(x[full], params=_params(F, fx, 1))                  # no lengths: every curve is Lmax long
    assert torch.equal(c.ints, a.ints[full]) and torch.equal(c.floats, a.floats[full])


@pytest.mark.parametrize("cap", [5, 10 ** 6])
def test_tiled_grid_and_compaction(F, fx, batch, cap):
    x, lens = batch
    n, reps = x.shape[0], 13                                                  # 13 x 61 = 793 workgroups > 256 CUs
    one = F.filter_curves(x, lengths=lens, params=_params(F, fx, 1))
    res = F.filter_curves(x.repeat(reps, 1, 1), lengths=lens.repeat(reps), params=_params(F, fx, 1, max_curves=cap))
    assert torch.equal(res.ints.view(reps, n, -1), one.ints[None].expand(reps, -1, -1))
    assert torch.equal(res.floats.view(reps, n, -1), one.floats[None].expand(reps, -1, -1))
    kept = fx["main1_kept"]
    want = np.concatenate([kept + r * n for r in range(reps)])[:cap]
    assert int(res.n_keep.item()) == len(want)
    keep_idx = res.keep_idx.cpu().numpy()
    assert np.array_equal(keep_idx[:len(want)], want) and (keep_idx[len(want):] == -1).all()
    assert (np.diff(want) > 0).all()
    if cap == 5:
        assert np.array_equal(want, fx["main1_cap5_kept"])                    # what the reference's --max_curves 5 kept


def _fp64_counts(curve, pr, scale_lo, scale_hi):
    """(point clashes ordered, segment clashes, beta_in_sheet) in torch fp64 on the CPU with every distance threshold t
    replaced by t * scale ('lo' narrows each accepted range, 'hi' widens it) -> two triples."""
    x = torch.from_numpy(curve[:, :3]).double()
    L = x.shape[0]
    i, j = torch.triu_indices(L, L, pr.neighbor_exclude + 1)
    d = (x[i] - x[j]).norm(dim=-1)
    t = torch.linspace(0.0, 1.0, pr.seg_num_samples, dtype=torch.float64)
    pts = x[:-1, None, :] + (x[1:] - x[:-1])[:, None, :] * t[None, :, None]
    si, sj = torch.triu_indices(L - 1, L - 1, 1 + pr.seg_neighbor_exclude)
    dmin = torch.cat([(pts[si[s:s + 8192], :, None, :] - pts[sj[s:s + 8192], None, :, :]).norm(dim=-1).flatten(1).min(1).values
                      for s in range(0, si.numel(), 8192)])
    beta = torch.from_numpy(curve[:, 3 + pr.beta_channel] > pr.ss_threshold)
    runs = "".join("b" if v else "." for v in beta.tolist()).split(".")
    has_strand = any(len(r) >= pr.min_strand_len for r in runs)
    out = []
    for lo in (True, False):
        s_in, s_out = (scale_lo, scale_hi) if lo else (scale_hi, scale_lo)      # s_in scales "closer than" thresholds
        pt = 2 * int((d < pr.min_pairwise_dist * s_in).sum())
        seg = int((dmin < pr.seg_min_dist * s_in).sum())
        pair = beta[i] & beta[j] & (d >= pr.sheet_min_dist * s_out) & (d <= pr.sheet_max_dist * s_in)
        partner = torch.zeros(L, dtype=torch.bool)
        partner[i[pair]] = True
        partner[j[pair]] = True
        out.append((pt, seg, int(partner.sum()) if has_strand else 0))
    return out


def test_fp64_sandwich_at_full_length(F, fx):
    import make_golden_filter as M
    pr = _params(F, fx, 1)
    curves = [M.walk(seed, L) for L, seeds in SANDWICH for seed in seeds]
    x = torch.full((len(curves), LPAD, 6), float("nan"))
    for k, c in enumerate(curves):
        x[k, :c.shape[0]] = torch.from_numpy(c)
    lens = torch.tensor([c.shape[0] for c in curves], dtype=torch.int32)
    res = F.filter_curves(x.cuda(), lengths=lens.cuda(), params=pr)
    got = res.ints.cpu().numpy()[:, [6, 7, 10]]
    total = np.zeros(3, np.int64)
    for k, c in enumerate(curves):
        lo, hi = _fp64_counts(c, pr, 1.0 - SANDWICH_EPS, 1.0 + SANDWICH_EPS)
        assert lo == hi, f"curve {k}: the fp64 counts differ between the two thresholds {lo} vs {hi}: choose another seed"
        assert tuple(got[k]) == lo, f"curve {k}: GPU {tuple(got[k])} vs fp64 {lo}"
        total += lo
    assert (total > 0).all(), total                                            # each of the three pair tests fires somewhere


def test_logits_give_the_rows_of_their_argmax(F, fx, batch):
    x, lens = batch
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(x.shape[0], LPAD, 3, generator=g)
    logits[:, 3::7, 1] = logits[:, 3::7].max(-1).values                       # exact ties: the first maximum must win
    logits[:, 5::11, 2] = logits[:, 5::11].max(-1).values
    k = int(fx["logits_index"])
    n = int(fx["lengths"][k])
    logits[k, :n] = torch.from_numpy(fx["logits_curve"][:, 3:6])
    onehot = torch.nn.functional.one_hot(logits.argmax(-1), 3).float()
    xl, xo = x.clone(), x.clone()
    xl[..., 3:6] = logits.cuda()
    xo[..., 3:6] = onehot.cuda()
    for p in (1, 2):
        a = F.filter_curves(xl, lengths=lens, params=_params(F, fx, p), ss_logits=True)
        b = F.filter_curves(xo, lengths=lens, params=_params(F, fx, p))
        assert torch.equal(a.ints, b.ints) and torch.equal(a.floats, b.floats) and torch.equal(a.keep_idx, b.keep_idx)
        assert int(b.ints[:, 8].max()) > 8 and int(b.ints[:, 11].max()) > 0  # beta residues and strands exist
        assert np.array_equal(a.ints[k].cpu().numpy(), fx["ints"][p][k])      # the fixture's tie curve, as the reference saw it


def test_graph_capture_and_replay(F, fx, batch):
    x, lens = batch
    pr = _params(F, fx, 1)
    sx, sl = x.clone(), lens.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        F.filter_curves(sx, lengths=sl, params=pr)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = F.filter_curves(sx, lengths=sl, params=pr)
    perm = torch.arange(x.shape[0] - 1, -1, -1, device=x.device)
    sx.copy_(x[perm])
    sl.copy_(lens[perm])
    for t in (res.ints, res.floats, res.keep_idx, res.n_keep):
        t.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    eager = F.filter_curves(x[perm].contiguous(), lengths=lens[perm].contiguous(), params=pr)
    assert torch.equal(res.ints, eager.ints) and torch.equal(res.floats, eager.floats)
    assert torch.equal(res.keep_idx, eager.keep_idx) and torch.equal(res.n_keep, eager.n_keep)
    assert int(eager.n_keep.item()) == len(fx["main1_kept"])


def test_sample_filtered(F):
    from models import vae_models
    cfg = dict(G.SMALL_VQ)
    m = vae_models["VQVAE"](**cfg)
    m.load_state_dict(G.model_state(cfg, 321), strict=True)
    m = m.to("cuda:0").eval()
    # a screen that cannot reject anything: the first round fills the request
    lax = F.FilterParams(min_length=1, bond_min_allowed=-1.0, bond_max_allowed=1e30, bond_frac_out_max=2.0,
                         angle_min_allowed=-1.0, angle_max_allowed=181.0, angle_frac_out_max=2.0, min_pairwise_dist=0.0,
                         seg_min_dist=0.0)
    torch.manual_seed(11)
    curves, stats = m.sample_filtered(7, "cuda:0", out_len=24, params=lax, max_rounds=2)
    assert curves.shape == (7, 24, 6) and stats["ints"].shape == (7, 14) and stats["floats"].shape == (7, 12)
    assert torch.equal(curves[..., 3:].sum(-1), torch.ones(7, 24, device=curves.device)) and bool(curves[..., 3:].max() == 1)
    again = F.filter_curves(curves, params=lax)
    assert int(again.ints[:, 1].abs().sum()) == 0 and torch.equal(again.ints, stats["ints"])
    assert torch.equal(again.floats, stats["floats"]) and lax.max_curves == 0
    # the reference's defaults on an untrained model: whatever passes is returned, nothing is required to pass
    torch.manual_seed(12)
    strict = F.FilterParams(min_length=2)
    curves, stats = m.sample_filtered(5, "cuda:0", out_len=24, params=strict, max_rounds=3)
    n = curves.shape[0]
    assert n <= 5 and curves.shape[1:] == (24, 6) and stats["ints"].shape == (n, 14) and stats["floats"].shape == (n, 12)
    if n:
        assert int(F.filter_curves(curves, params=strict).ints[:, 1].abs().sum()) == 0


@pytest.mark.parametrize("p", [0, 1, 2])
def test_cli_end_to_end(F, fx, tmp_path, capsys, p):
    cli = _cli()
    rdir, odir = tmp_path / "recon", tmp_path / "out"
    rdir.mkdir()
    names = [str(n) for n in fx["file_names"]]
    for name, c in zip(names, _split(fx)):
        np.save(str(rdir / name), c)
    (tmp_path / "samples.jsonl").write_text("\n".join(str(s) for s in fx["samples_manifest"]) + "\n\nnot json\n")
    argv = ["--recon_dir", str(rdir), "--out_dir", str(odir), "--samples_manifest", str(tmp_path / "samples.jsonl"),
            "--filtered_manifest_out", str(tmp_path / "filtered.jsonl")]
    for k, v in json.loads(str(fx["param_overrides"][p])).items():
        argv += [f"--{k}", str(v)]
    cli.main(argv)
    out = capsys.readouterr().out
    summary = [int(line.rsplit(":", 1)[1]) for line in out.splitlines() if line.startswith("[summary]")]
    assert summary == fx[f"main{p}_summary"].tolist()
    kept = fx[f"main{p}_kept"].tolist()
    assert sorted(os.listdir(odir)) == [names[k] for k in kept]
    for k in kept[:3]:
        assert np.array_equal(np.load(str(odir / names[k])), np.load(str(rdir / names[k])))
    recs = [json.loads(line) for line in (tmp_path / "filtered.jsonl").read_text().splitlines()]
    want = [json.loads(str(s)) for s in fx[f"main{p}_records"]]
    assert len(recs) == len(want) == len(kept)
    col = {c: i for i, c in enumerate(F.FLOAT_COLUMNS)}
    for k, got, ref in zip(kept, recs, want):
        assert list(got) == list(ref), names[k]
        for key, v in ref.items():
            if key == "recon_path":
                assert os.path.basename(got[key]) == v
            elif key in col:
                tol = scalar_tol(fx["f32"][p][k, col[key]], fx["f64"][p][k, col[key]])
                assert abs(got[key] - v) <= tol, (names[k], key, got[key], v, tol)
            else:
                assert got[key] == v and type(got[key]) is type(v), (names[k], key, got[key], v)
    if p == 1:                                                                # --max_curves: the reference stops reading there
        cli.main(argv + ["--max_curves", "5", "--out_dir", str(tmp_path / "out5")])
        out = capsys.readouterr().out
        summary = [int(line.rsplit(":", 1)[1]) for line in out.splitlines() if line.startswith("[summary]")]
        assert summary == fx["main1_cap5_summary"].tolist()
        assert sorted(os.listdir(tmp_path / "out5")) == [names[k] for k in fx["main1_cap5_kept"]]
