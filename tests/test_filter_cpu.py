# -*- coding: utf-8 -*-
"""CPU side of the curve validity screen (vqh_curve_filter / vqvae_hip.curve_filter / prior/filter_curves.py): ABI agreement,
defaults, CLI flags and host helpers against tests/golden/curve_filter.npz (recorded from the reference by
tests/golden/make_golden_filter.py)."""
import dataclasses
import importlib.util
import json
import os
import re

import numpy as np
import pytest

from abi_util import HDR, header_protos
from conftest import PKG, load_golden

REF_ROOT = "/root/reference"


@pytest.fixture(scope="module")
def fx():
    return load_golden("curve_filter")


def _cli():
    spec = importlib.util.spec_from_file_location("vqh_prior_filter_curves", os.path.join(PKG, "prior", "filter_curves.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fixture_curves(fx):
    """-> list of [L, C] fp32 arrays (C = 3 or 6) in fixture order."""
    out, o = [], 0
    for L, c in zip(fx["lengths"], fx["channels"]):
        out.append(np.ascontiguousarray(fx["curves"][o:o + L, :c]))
        o += L
    return out


def _struct_fields(text, name):
    """[(ctype, field)] of `struct name { ... }` in C source text."""
    body = re.search(r"struct\s+" + name + r"\s*\{(.*?)\}", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/|//[^\n]*", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            out += [(ctype, n.strip()) for n in names.split(",")]
    return out


def test_header_source_and_ctypes_agree_on_curve_filter():
    import ctypes
    from vqvae_hip import curve_filter as F
    from vqvae_hip import lib
    hdr = header_protos()
    assert hdr.get("vqh_curve_filter") == "piiipipppppp"
    assert lib._PROTOS.get("vqh_curve_filter") == hdr["vqh_curve_filter"]
    assert "vqh_curve_filter" in lib.EXPORTS
    src = open(os.path.join(PKG, "csrc", "filter.hip")).read()
    m = re.search(r'extern "C"\s+int\s+vqh_curve_filter\s*\(([^)]*)\)\s*\{', src)
    assert m, "vqh_curve_filter is not defined in csrc/filter.hip"
    assert len(m.group(1).split(",")) == len(hdr["vqh_curve_filter"])
    h_fields, s_fields = _struct_fields(open(HDR).read(), "vqh_filter_params_t"), _struct_fields(src, "vqh_filter_params_t")
    assert h_fields == s_fields
    ct = {ctypes.c_double: "double", ctypes.c_int: "int"}
    assert [(ct[t], n) for n, t in F.FilterParamsT._fields_] == h_fields
    assert {n for _, n in h_fields} == {f.name for f in dataclasses.fields(F.FilterParams)}
    for text in (open(HDR).read(), src):
        assert int(re.search(r"#define\s+VQH_FILTER_MAX_LEN\s+(\d+)", text).group(1)) == F.MAX_LEN
    L = lib.lib()
    assert hasattr(L, "vqh_curve_filter")
    assert L.vqh_abi_version() == 1


def test_filter_params_defaults_equal_the_reference_constants(fx):
    from vqvae_hip.curve_filter import FLOAT_COLUMNS, INT_COLUMNS, FilterParams
    p = FilterParams()
    consts = json.loads(str(fx["main_constants"]))
    mine = {"SEG_NUM_SAMPLES": "seg_num_samples", "THRESHOLD": "ss_threshold", "SEG_NEIGHBOR_EXCLUDE": "seg_neighbor_exclude"}
    assert len(consts) == 16
    for k, v in consts.items():
        assert getattr(p, mine.get(k, k.lower())) == v, k
    flags = json.loads(str(fx["cli_flags"]))
    for flag, spec in flags.items():
        name = flag.lstrip("-")
        if hasattr(p, name):
            assert getattr(p, name) == spec["default"], flag
    assert sorted(f.name for f in dataclasses.fields(FilterParams)) == sorted(
        [mine.get(k, k.lower()) for k in consts] + [f.lstrip("-") for f in flags if hasattr(p, f.lstrip("-"))])
    assert tuple(fx["int_columns"]) == INT_COLUMNS and tuple(fx["float_columns"]) == FLOAT_COLUMNS


def test_cli_parser_has_exactly_the_reference_flags(fx):
    flags = json.loads(str(fx["cli_flags"]))
    ap = _cli().build_parser()
    acts = {a.option_strings[0]: a for a in ap._actions if a.option_strings and a.option_strings[0] != "-h"}
    assert set(acts) == set(flags)
    for flag, spec in flags.items():
        a = acts[flag]
        assert a.required == spec["required"], flag
        assert a.type.__name__ == spec["type"], flag
        if not spec["required"]:
            assert a.default == spec["default"] and type(a.default) is type(spec["default"]), flag


def test_host_helpers_reproduce_the_recorded_names_and_records(fx, tmp_path, capsys):
    cli = _cli()
    names = [str(n) for n in fx["file_names"]]
    assert [(-1 if cli.index_from_name(n) is None else cli.index_from_name(n)) for n in names] == fx["name_index"].tolist()
    assert (fx["name_index"] == -1).sum() >= 3
    mpath = tmp_path / "samples.jsonl"
    mpath.write_text("\n".join(str(s) for s in fx["samples_manifest"]) + "\n\nnot json\n")
    manifest = cli.load_manifest(str(mpath))
    assert cli.load_manifest(str(tmp_path / "missing.jsonl")) == {}
    n_rec = 0
    for p in range(3):
        kept = fx[f"main{p}_kept"].tolist()
        for k, line in zip(kept, fx[f"main{p}_records"]):
            want = json.loads(str(line))
            got = cli.merge_record(manifest, names[k], k, names[k], want)      # the record's own statistics go back in
            assert got == want and list(got) == list(want), names[k]
            n_rec += 1
    assert n_rec > 30
    # batch packing: every curve once, padded with zeros, SS curves and xyz-only curves apart, lengths kept
    curves = fixture_curves(fx)
    batches = cli.pack_batches(list(enumerate(curves)), max_curves=25)
    seen = []
    for positions, x, lens in batches:
        assert x.dtype == np.float32 and lens.dtype == np.int32 and x.shape[0] == len(positions) <= 25
        assert x.shape[1] == lens.max() and list(lens) == sorted(lens)
        for r, pos in enumerate(positions):
            assert x.shape[2] == curves[pos].shape[1] and lens[r] == curves[pos].shape[0]
            assert np.array_equal(x[r, :lens[r]], curves[pos]) and not x[r, lens[r]:].any()
        seen += positions
    assert sorted(seen) == list(range(len(curves)))


def test_product_filter_fails_loudly_without_gpu(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from vqvae_hip.curve_filter import filter_curves
    from vqvae_hip.lib import VqhError
    with pytest.raises(VqhError):
        filter_curves(torch.zeros(2, 8, 6))


def test_fixture_still_matches_the_reference_functions(fx):
    if not os.path.isfile(os.path.join(REF_ROOT, "prior", "filter_curves.py")):
        pytest.skip("the reference tree is not on this machine")
    import make_golden_filter as M
    ref, path = M.load_reference(REF_ROOT)
    consts, flags = M.main_constants_and_flags(path)
    assert consts == json.loads(str(fx["main_constants"])) and flags == json.loads(str(fx["cli_flags"]))
    psets = [json.loads(str(s)) for s in fx["param_sets"]]
    ev = M.Evaluator(ref, consts)
    curves = fixture_curves(fx)
    pick = [k for k, c in enumerate(curves) if c.shape[0] <= 130]             # the L = 350 segment loops take seconds each
    for k in pick:
        for p, ps in enumerate(psets):
            i32, f32 = ev.columns((k, 32), curves[k], ps)
            i64, f64 = ev.columns((k, 64), curves[k].astype(np.float64), ps)
            assert np.array_equal(i32, fx["ints"][p, k]) and np.array_equal(i64, fx["ints"][p, k])
            np.testing.assert_allclose(f32, fx["f32"][p, k], rtol=1e-6, atol=0)
            np.testing.assert_allclose(f64, fx["f64"][p, k], rtol=1e-12, atol=0)
