# -*- coding: utf-8 -*-
"""-m gpu: StepEngine.side_pass -- an inference pass next to a step in flight -- and its two users' contract: whatever runs
inside (a failure, the quantizer's stand-alone call) leaves the following loss_function + backward bit-identical.  Also pins
that the removed second-stream weight-gradient experiment left nothing behind: its environment variable is inert."""
import os
import subprocess
import sys

import pytest
import torch

import gen_inputs as G
from conftest import GOLD, PKG, REPO

pytestmark = pytest.mark.gpu

WEIGHTS = dict(G.BASE_LOSS_WEIGHTS, xyz_tv_lambda=0.001, bond_length_weight=0.01)
CFGS = {"small_vq": G.SMALL_VQ, "small_rvq": G.SMALL_RVQ}
SEED = 31


def _model(name):
    from models import vae_models
    cfg = CFGS[name]
    m = vae_models["VQVAE"](**cfg)
    m.load_state_dict(G.model_state(cfg, SEED), strict=True)
    m = m.to("cuda:0").train()
    m.training_steps = 1
    m._engine().drop_scale = 0.0
    return m


def _step(name, between):
    """forward -> between(m) -> loss_function -> backward on a fresh model; everything a later comparison needs."""
    x, mask = G.curve_batch(5, 33, SEED + 100, ragged=True)
    x, mask = x.cuda(), mask.cuda()
    m = _model(name)
    out = m(x, mask)
    between(m)
    ld = m.loss_function(*out, **WEIGHTS)
    ld["loss"].backward()
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in ld.items()}, m._engine().flat_g.clone(), m.quantizer.embedding.clone()


def _assert_same_step(a, b):
    (ld_a, g_a, e_a), (ld_b, g_b, e_b) = a, b
    assert ld_a.keys() == ld_b.keys()
    for k in ld_a:
        assert torch.equal(ld_a[k], ld_b[k]), k
    assert torch.equal(g_a, g_b) and torch.equal(e_a, e_b) and float(g_a.abs().sum()) > 0


@pytest.fixture(scope="module")
def plain():
    return {name: _step(name, lambda m: None) for name in CFGS}


def test_side_pass_restores_on_failure(plain):
    def fail_inside(m):
        eng = m._engine()
        key, ctx = eng.arena.key, eng.ctx
        flags = (eng.train, eng.defer_ema, eng._pending_ema)
        assert ctx is not None
        with pytest.raises(ZeroDivisionError):
            with eng.side_pass(("probe", 1, 1)):
                assert eng.arena.key == ("probe", 1, 1) and eng.ctx == {} and eng.ctx is not ctx
                assert (eng.train, eng.defer_ema) == (False, False)
                eng.T("probe.buf", 7).zero_()
                1 / 0
        assert eng.arena.key == key and eng.arena is eng.arenas[key] and eng.buf is eng.arena.buf
        assert (eng.train, eng.defer_ema, eng._pending_ema) == flags and eng.ctx is ctx
    _assert_same_step(plain["small_vq"], _step("small_vq", fail_inside))


@pytest.mark.parametrize("name", ["small_vq", "small_rvq"])
def test_quantizer_call_between_forward_and_backward(plain, name):
    cfg = CFGS[name]
    g = torch.Generator().manual_seed(SEED + 7)
    zs = [torch.randn(B, cfg["latent_tokens"], cfg["code_dim"], generator=g).cuda() for B in (5, 3)]   # the step's B, another

    def quantize(m):
        for z in zs:
            z_st, z_q, idx, stats = m.quantizer(z, do_ema_update=False)
            assert z_q.shape == z.shape and torch.isfinite(z_st).all()
    _assert_same_step(plain[name], _step(name, quantize))


_CHILD = """
import sys
sys.path[:0] = {paths!r}
import torch
import gen_inputs as G
from models import vae_models
m = vae_models["VQVAE"](**G.SMALL_VQ)
m.load_state_dict(G.model_state(G.SMALL_VQ, {seed}), strict=True)
m = m.to("cuda:0").train()
eng = m._engine()
eng.drop_scale = 0.0
x, mask = G.curve_batch(5, 33, {seed} + 100, ragged=True)
x, mask = x.cuda(), mask.cuda()
modes = []
for _ in range(3):
    m.train_step(x, mask, {weights!r}, 1e-3, 0.01, 1.0)
    modes.append(eng.last_step_mode)
torch.cuda.synchronize()
assert modes == ["eager", "capture", "graph"], modes
assert not hasattr(eng, "overlap_wgrad")
torch.save(eng.flat_p.cpu(), sys.argv[1])
"""


def test_overlap_variable_is_inert(tmp_path):
    code = _CHILD.format(paths=[REPO, PKG, GOLD], seed=SEED, weights=WEIGHTS)
    got = []
    for val in (None, "1"):                           # one child after the other
        env = {k: v for k, v in os.environ.items() if k != "VQH_OVERLAP_WGRAD"}
        if val is not None:
            env["VQH_OVERLAP_WGRAD"] = val
        out = str(tmp_path / f"flat_p_{val}.pt")
        r = subprocess.run([sys.executable, "-c", code, out], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        got.append(torch.load(out, weights_only=True))
    assert torch.equal(got[0], got[1]) and float(got[0].abs().sum()) > 0
