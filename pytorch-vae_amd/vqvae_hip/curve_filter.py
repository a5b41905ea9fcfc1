# -*- coding: utf-8 -*-
"""GPU validity screen of decoded curves: the batched counterpart of the reference's prior/filter_curves.py.

filter_curves() screens a padded batch [B, Lmax, C] in one call of vqh_curve_filter (csrc/filter.hip): bond / angle sanity,
point and segment self-collision, beta strand / sheet heuristics, the accept / reject decision and the compaction of the kept
indices all stay on the device.  Unlike the script, which stops at a curve's first failing check, every statistic is computed
for every curve; `reason` records the decision.  There is no CPU fallback: without a GPU the call raises VqhError."""
import ctypes as C
import dataclasses
from dataclasses import dataclass

import torch

from . import lib as _L

INT_COLUMNS = ("length", "reason", "bond_num", "bond_out", "angle_num", "angle_out", "n_self_clash_pairs", "n_seg_clash_pairs",
               "beta_total", "beta_max_run", "beta_in_sheet", "beta_strands_total", "beta_strands_sheet", "beta_strands_isolated")
FLOAT_COLUMNS = ("bond_mean", "bond_std", "bond_min", "bond_max", "bond_frac_out", "angle_mean", "angle_std", "angle_min",
                 "angle_max", "angle_frac_out", "rg", "beta_sheet_fraction")
REASONS = ("kept", "too_short", "too_long", "bond", "angle", "point_collision", "segment_clash", "ss_rules")
MAX_LEN = 2048                      # VQH_FILTER_MAX_LEN

_DOUBLES = ("bond_min_allowed", "bond_max_allowed", "bond_good_min", "bond_good_max", "bond_frac_out_max",
            "angle_min_allowed", "angle_max_allowed", "angle_good_min", "angle_good_max", "angle_frac_out_max",
            "min_pairwise_dist", "seg_min_dist", "sheet_min_dist", "sheet_max_dist", "ss_threshold", "min_beta_sheet_fraction")
_INTS = ("min_length", "max_length", "neighbor_exclude", "seg_neighbor_exclude", "seg_num_samples", "min_beta_run",
         "min_beta_total", "beta_channel", "max_isolated_beta_strands", "min_strand_len", "max_curves")


class FilterParamsT(C.Structure):
    """vqh_filter_params_t of include/vqvae_hip.h"""
    _fields_ = [(n, C.c_double) for n in _DOUBLES] + [(n, C.c_int) for n in _INTS]


@dataclass
class FilterParams:
    """Defaults = the reference CLI's defaults plus the constants hard-coded in its main()."""
    min_length: int = 32
    max_length: int = 0                       # 0 = no upper bound
    min_pairwise_dist: float = 1.0
    neighbor_exclude: int = 2
    min_beta_run: int = 0
    min_beta_total: int = 0
    beta_channel: int = 1
    max_curves: int = 0                       # 0 = no cap
    min_beta_sheet_fraction: float = 0.0
    max_isolated_beta_strands: int = -1       # < 0 = rule off
    min_strand_len: int = 3
    bond_min_allowed: float = 2.2
    bond_max_allowed: float = 7.5
    bond_good_min: float = 2.0
    bond_good_max: float = 7.2
    bond_frac_out_max: float = 0.90
    angle_min_allowed: float = 10.0
    angle_max_allowed: float = 180.0
    angle_good_min: float = 30.0
    angle_good_max: float = 180.0
    angle_frac_out_max: float = 0.90
    seg_min_dist: float = 1.3
    seg_neighbor_exclude: int = 1
    seg_num_samples: int = 5
    sheet_min_dist: float = 4.0
    sheet_max_dist: float = 6.0
    ss_threshold: float = 0.5

    def to_struct(self) -> FilterParamsT:
        return FilterParamsT(**{n: float(getattr(self, n)) for n in _DOUBLES}, **{n: int(getattr(self, n)) for n in _INTS})


@dataclass
class FilterResult:
    ints: torch.Tensor          # [B, 14] int32, INT_COLUMNS
    floats: torch.Tensor        # [B, 12] fp32, FLOAT_COLUMNS
    keep_idx: torch.Tensor      # [B] int32: kept indices ascending, then -1
    n_keep: torch.Tensor        # [1] int32 (device)

    def records(self):
        """Host dicts, one per curve, with the reference manifest's key names (plus `reason` and the counts)."""
        ints, floats = self.ints.cpu().tolist(), self.floats.cpu().tolist()
        out = []
        for iv, fv in zip(ints, floats):
            rec = dict(zip(INT_COLUMNS, iv))
            rec.update(zip(FLOAT_COLUMNS, fv))
            rec["length_recon"] = rec.pop("length")
            out.append(rec)
        return out


def filter_curves(curves, lengths=None, mask=None, params=None, ss_logits=False) -> FilterResult:
    """curves [B, Lmax, C >= 3] fp32 on the GPU; lengths [B] (or the model's prefix mask [B, Lmax]; default: all Lmax)."""
    _L.require_gpu()
    if params is None:
        params = FilterParams()
    if curves.dim() != 3 or curves.shape[2] < 3 or curves.shape[1] < 1:
        raise _L.VqhError(f"filter_curves: curves must be [B, Lmax >= 1, C >= 3], got {tuple(curves.shape)}")
    if not curves.is_cuda:
        raise _L.VqhError("filter_curves: curves must live on the GPU (there is no CPU fallback)")
    B, Lmax, Cc = curves.shape
    if Lmax > MAX_LEN:
        raise _L.VqhError(f"filter_curves: Lmax {Lmax} > {MAX_LEN}")
    dev = curves.device
    curves = curves.float().contiguous()
    if lengths is None:
        lengths = mask.sum(1) if mask is not None else torch.full((B,), Lmax, device=dev)
    lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int32).contiguous()
    if lengths.shape != (B,):
        raise _L.VqhError(f"filter_curves: lengths must be [{B}], got {tuple(lengths.shape)}")
    res = FilterResult(torch.empty(B, len(INT_COLUMNS), dtype=torch.int32, device=dev),
                       torch.empty(B, len(FLOAT_COLUMNS), dtype=torch.float32, device=dev),
                       torch.empty(B, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
    st = params.to_struct()
    with torch.cuda.device(dev):
        _L.call("vqh_curve_filter", curves, B, Lmax, Cc, lengths, int(bool(ss_logits)), C.addressof(st), res.ints, res.floats,
                res.keep_idx, res.n_keep)
    return res


def params_from_dict(d) -> FilterParams:
    names = {f.name for f in dataclasses.fields(FilterParams)}
    return FilterParams(**{k: v for k, v in d.items() if k in names})
