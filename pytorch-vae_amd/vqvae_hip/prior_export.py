# -*- coding: utf-8 -*-
"""GPU export of prior-training data: the device side of the reference's scripts/extract_code_indices.py and
scripts/decode_with_vqvae.py (csrc/export.hip).

pack_codes()      level-major quantizer ids -> per-sample code rows [B, M*Q] int32 (+ each row's largest id)
codes_to_latent() code rows -> z_q [B, M, D]: codebook lookup with the sum over the residual levels
latent_geometry() per-latent geometry descriptors [B, M*Q, C + 4] of a padded batch of curves

Everything stays on the device; there is no CPU fallback: without a GPU the calls raise VqhError."""
import torch

from . import lib as _L

GEO_MAX_CHANNELS = 60


def geo_columns(C=6):
    """Column names of a geo row for curves with C channels (G = C + 4)."""
    return (["center_x", "center_y", "center_z", "dir_x", "dir_y", "dir_z"] + [f"ss_mean_{c}" for c in range(C - 3)] + ["radius"])


def pack_codes(idx, Q, B, M):
    """idx: the quantizer's ids, int64 on the GPU, Q*B*M of them level-major ([B, M] for Q = 1).
    -> (codes [B, M*Q] int32 in the order t0_l0, t0_l1, ..., row_max [B] int32)."""
    _L.require_gpu()
    Q, B, M = int(Q), int(B), int(M)
    if Q < 1 or B < 0 or M < 1:
        raise _L.VqhError(f"pack_codes: need Q >= 1, B >= 0, M >= 1 (got Q={Q}, B={B}, M={M})")
    if not torch.is_tensor(idx) or not idx.is_cuda or idx.dtype != torch.int64:
        raise _L.VqhError("pack_codes: idx must be an int64 tensor on the GPU (there is no CPU fallback)")
    if idx.numel() != Q * B * M:
        raise _L.VqhError(f"pack_codes: idx holds {idx.numel()} ids, expected Q*B*M = {Q * B * M}")
    idx = idx.contiguous()
    codes = torch.empty(B, M * Q, dtype=torch.int32, device=idx.device)
    row_max = torch.empty(B, dtype=torch.int32, device=idx.device)
    with torch.cuda.device(idx.device):
        _L.call("vqh_codes_pack", idx, Q, B, M, codes, row_max)
    return codes, row_max


def codes_to_latent_async(codes, embedding, Q):
    """codes_to_latent without the host read: -> (z_q [B, M, D], n_bad [1] int32 on the device)."""
    _L.require_gpu()
    Q = int(Q)
    if not torch.is_tensor(codes) or not codes.is_cuda or codes.dim() != 2:
        raise _L.VqhError("codes_to_latent: codes must be a [B, M*Q] integer tensor on the GPU (there is no CPU fallback)")
    if codes.dtype.is_floating_point or codes.dtype == torch.bool:
        raise _L.VqhError(f"codes_to_latent: codes must be integers, got {codes.dtype}")
    if Q < 1 or codes.shape[1] < Q or codes.shape[1] % Q:
        raise _L.VqhError(f"codes_to_latent: row length {codes.shape[1]} is not a positive multiple of Q = {Q}")
    if (embedding.dim() != 2 or embedding.dtype != torch.float32 or embedding.device != codes.device
            or embedding.stride(1) != 1 or embedding.stride(0) < embedding.shape[1]):
        raise _L.VqhError("codes_to_latent: embedding must be an fp32 [K, D] matrix with contiguous rows on the codes' device")
    B, M = int(codes.shape[0]), int(codes.shape[1]) // Q
    K, D = int(embedding.shape[0]), int(embedding.shape[1])
    codes = codes.to(torch.int32).contiguous()
    zq = torch.empty(B, M, D, dtype=torch.float32, device=codes.device)
    n_bad = torch.empty(1, dtype=torch.int32, device=codes.device)
    with torch.cuda.device(codes.device):
        _L.call("vqh_codes_to_latent", codes, B, M, Q, embedding, int(embedding.stride(0)), K, D, zq, n_bad)
    return zq, n_bad


def codes_to_latent(codes, embedding, Q):
    """codes [B, M*Q] integers, embedding [K, D] fp32 (row stride >= D) -> z_q [B, M, D] = sum over the Q levels of the code
    vectors, fp32 in ascending level.  Raises VqhError when an id lies outside 0..K-1 (one host read of the counter)."""
    zq, n_bad = codes_to_latent_async(codes, embedding, Q)
    bad = int(n_bad.item())
    if bad:
        raise _L.VqhError(f"codes_to_latent: {bad} code id(s) outside 0..{int(embedding.shape[0]) - 1}")
    return zq


def latent_geometry(x, lengths=None, mask=None, M=None, Q=1):
    """x [B, Lmax, C >= 3] fp32 on the GPU; lengths [B] (or the model's prefix mask [B, Lmax]; default: all Lmax).
    -> geo [B, M*Q, C + 4] fp32: centre, unit direction, SS means, radius of each of the M segments, each row Q times."""
    _L.require_gpu()
    if M is None:
        raise _L.VqhError("latent_geometry: M (latent tokens per curve) is required")
    M, Q = int(M), int(Q)
    if not torch.is_tensor(x) or x.dim() != 3 or x.shape[1] < 1 or not 3 <= x.shape[2] <= GEO_MAX_CHANNELS:
        raise _L.VqhError(f"latent_geometry: x must be [B, Lmax >= 1, 3 <= C <= {GEO_MAX_CHANNELS}], "
                          f"got {tuple(x.shape) if torch.is_tensor(x) else type(x)}")
    if not x.is_cuda:
        raise _L.VqhError("latent_geometry: x must live on the GPU (there is no CPU fallback)")
    if M < 1 or Q < 1:
        raise _L.VqhError(f"latent_geometry: need M >= 1 and Q >= 1 (got M={M}, Q={Q})")
    B, Lmax, Cc = x.shape
    dev = x.device
    x = x.float().contiguous()
    if lengths is None:
        lengths = mask.sum(1) if mask is not None else torch.full((B,), Lmax, device=dev)
    lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int32).contiguous()
    if lengths.shape != (B,):
        raise _L.VqhError(f"latent_geometry: lengths must be [{B}], got {tuple(lengths.shape)}")
    geo = torch.empty(B, M * Q, Cc + 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _L.call("vqh_latent_geometry", x, B, Lmax, Cc, lengths, M, Q, geo)
    return geo
