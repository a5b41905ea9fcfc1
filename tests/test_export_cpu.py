# -*- coding: utf-8 -*-
"""CPU-side checks of the prior-data export (csrc/export.hip, vqvae_hip.prior_export, scripts/extract_code_indices.py and
scripts/decode_with_vqvae.py): the ABI of the three entry points, the committed fixture against the live reference (where the
reference tree is present), the closed form of the segment bounds against numpy, and the CLIs' flags against the reference's."""
import ast
import importlib.util
import json
import os
import re

import numpy as np
import pytest

from abi_util import header_protos
from conftest import GOLD, PKG, load_golden

REF = "/root/reference"
SIGS = {"vqh_codes_pack": "piiippp", "vqh_codes_to_latent": "piiipiiippp", "vqh_latent_geometry": "piiipiipp"}


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _source_sig(name):
    src = open(os.path.join(PKG, "csrc", "export.hip")).read()
    m = re.search(r'extern "C"\s+int\s+' + name + r"\s*\(([^)]*)\)\s*\{", src)
    assert m, f"{name} is not defined in csrc/export.hip"
    code = ""
    for a in m.group(1).split(","):
        a = a.strip()
        code += "p" if ("*" in a or a.startswith("hipStream_t")) else {"int": "i", "float": "f"}[a.split()[0]]
    return code


def test_header_ctypes_table_and_source_agree_on_the_three_signatures():
    from vqvae_hip import lib
    hdr = header_protos()
    for name, sig in SIGS.items():
        assert hdr.get(name) == sig, f"{name}: header {hdr.get(name)} vs {sig}"
        assert lib._PROTOS.get(name) == sig, f"{name}: ctypes table {lib._PROTOS.get(name)} vs {sig}"
        assert name in lib.EXPORTS
        assert _source_sig(name) == sig
        assert hasattr(lib.lib(), name)
    assert lib.lib().vqh_abi_version() == 1


def test_python_surface_refuses_host_tensors():
    """No CPU fallback: without a GPU require_gpu raises, with one the host tensors themselves are refused."""
    import torch
    from vqvae_hip import prior_export as X
    from vqvae_hip.lib import VqhError
    with pytest.raises(VqhError):
        X.latent_geometry(torch.zeros(1, 4, 6), M=2)
    with pytest.raises(VqhError):
        X.pack_codes(torch.zeros(8, dtype=torch.int64), 1, 2, 4)
    with pytest.raises(VqhError):
        X.codes_to_latent(torch.zeros(2, 4, dtype=torch.int32), torch.zeros(8, 4), 1)


def test_closed_form_bounds_equal_numpy_linspace():
    """What the kernel evaluates -- (long long)((double)t * ((double)L / (double)M)) for t < M, L for t = M -- against
    np.linspace(0, L, M + 1, dtype=int64), in pure Python floats (IEEE fp64, one divide, one multiply, truncation)."""
    int_div_differs = []
    for M in (8, 32, 48, 64):
        for L in range(1, 351):
            want = np.linspace(0, L, M + 1, dtype=np.int64).tolist()
            step = float(L) / float(M)
            got = [int(float(t) * step) for t in range(M)] + [L]
            assert got == want, (M, L)
            if [(t * L) // M for t in range(M + 1)] != want:
                int_div_differs.append((M, L))
    assert int_div_differs == [(48, 208)]          # why the kernel may not use integer division; the fixture holds this shape


def test_fixture_is_self_consistent():
    fx = load_golden("prior_export")
    cases = fx["geo_cases"].tolist()
    for need in ((48, 1, 208), (8, 3, 3), (8, 1, 1), (8, 1, 8), (32, 4, 350), (64, 1, 257), (32, 1, 33)):
        assert list(need) in cases
    offs = fx["geo_offsets"]
    assert offs[-1] == fx["geo_curves"].shape[0] and fx["geo_curves"].shape[1] == 6
    for k, (M, Q, L) in enumerate(cases):
        assert offs[k + 1] - offs[k] == L
        r32, r64 = fx[f"geo{k}_ref32"], fx[f"geo{k}_ref64"]
        assert r32.shape == r64.shape == (M * Q, 10) and r32.dtype == np.float32 and r64.dtype == np.float64
        assert np.array_equal(r32.reshape(M, Q, 10), np.repeat(r32.reshape(M, Q, 10)[:, :1], Q, 1))
    for name in fx["model_cases"]:
        codes, z_e, lens = fx[f"{name}_codes"], fx[f"{name}_z_e"], fx[f"{name}_lengths"]
        assert codes.dtype == np.int32 and codes.shape[0] == z_e.shape[0] == len(lens) == 5 and lens.max() == 33
        assert codes.shape[1] % z_e.shape[1] == 0 and float(fx[f"{name}_min_gap64"]) >= 1e-4
        for b, L in enumerate(lens):
            assert fx[f"{name}_recon{b}"].shape == (L, 6)
    assert len(fx["manifest_keys"]) == 10
    assert os.path.getsize(os.path.join(GOLD, "prior_export.npz")) < (1 << 20)


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not present on this machine")
def test_fixture_matches_the_live_reference():
    import torch
    fx = load_golden("prior_export")
    X = _load(os.path.join(REF, "scripts", "extract_code_indices.py"), "ref_extract_code_indices_t")
    offs = fx["geo_offsets"]
    for k, (M, Q, L) in enumerate(fx["geo_cases"].tolist()):
        x = fx["geo_curves"][offs[k]:offs[k + 1]]
        ref = X.compute_latent_geometry_for_sample(coords=x[:, :3], ss=x[:, 3:], valid_len=L, num_codes=M * Q, num_quantizers=Q)
        assert np.array_equal(ref, fx[f"geo{k}_ref32"]), (M, Q, L)
    # the [Q, B, M] -> [B, M, Q] permutation the pack kernel is tested against
    Q, B, M = 3, 5, 7
    idx = torch.arange(Q * B * M)
    got = X._ensure_batch_first_2d(idx, torch.ones(B, 4, dtype=torch.bool), num_quantizers=Q, latent_tokens=M)
    assert torch.equal(got, idx.view(Q, B, M).permute(1, 2, 0).reshape(B, M * Q))
    gen = _load(os.path.join(GOLD, "make_golden_export.py"), "make_golden_export_t")
    for script, key in (("extract_code_indices.py", "flags_extract"), ("decode_with_vqvae.py", "flags_decode")):
        assert gen.cli_flags(os.path.join(REF, "scripts", script)) == json.loads(str(fx[key]))


def _flags(path):
    out = {}
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument":
            kw = {k.arg: k.value for k in node.keywords}
            out[ast.literal_eval(node.args[0])] = {
                "default": ast.literal_eval(kw["default"]) if "default" in kw else None,
                "type": kw["type"].id if "type" in kw else None,
                "required": ast.literal_eval(kw["required"]) if "required" in kw else False,
                "choices": ast.literal_eval(kw["choices"]) if "choices" in kw else None,
                "action": ast.literal_eval(kw["action"]) if "action" in kw else None}
    return out


@pytest.mark.parametrize("script,key,extra", [("extract_code_indices.py", "flags_extract", ()),
                                              ("decode_with_vqvae.py", "flags_decode", ("--batch_size",))])
def test_cli_flags_equal_the_reference(script, key, extra):
    fx = load_golden("prior_export")
    want = json.loads(str(fx[key]))
    got = _flags(os.path.join(PKG, "scripts", script))
    assert set(got) - set(want) == set(extra)
    for flag, spec in want.items():
        assert got.get(flag) == spec, (flag, got.get(flag), spec)
    mod = _load(os.path.join(PKG, "scripts", script), "vqh_cli_" + script[:-3])
    ns = mod.build_parser().parse_args([a for f, s in want.items() if s["required"] for a in (f, "x")])
    for flag, spec in want.items():
        if not spec["required"]:
            assert getattr(ns, flag.lstrip("-")) == (False if spec["action"] == "store_true" else spec["default"]), flag
    if extra:
        assert ns.batch_size == 64


def test_manifest_keys_equal_the_reference():
    fx = load_golden("prior_export")
    mod = _load(os.path.join(PKG, "scripts", "extract_code_indices.py"), "vqh_cli_extract_keys")
    assert list(mod.MANIFEST_KEYS) == [str(k) for k in fx["manifest_keys"]]
